"""CPU tests of the drop-in boundary (no GPU, no compute calls): libts2d.so loads and exports every symbol that
include/ts2d.h declares; the Python package mirrors the reference's interface (names, field order, errors)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts2d.h")
HEADERS = [os.path.join(ROOT, "include", n) for n in sorted(os.listdir(os.path.join(ROOT, "include"))) if n.endswith(".h")]


@pytest.fixture(scope="module")
def lib(hip_lib_built):
    from diff_triangle_rasterization_2D import _abi  # every signature is declared there, once; bound here on a CDLL of this module's own
    return _abi.bind(ctypes.CDLL(hip_lib_built))


def _declared_functions():
    names = set()
    for h in HEADERS:  # every header under include/: ts2d.h (rasterizer), ts_loss.h (photometric loss), ts_knn.h (nearest neighbours)
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        names |= set(re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso)_[a-z0-9_]+)\s*\(", src))
    return sorted(names)


def test_header_declares_the_expected_entry_points():
    names = _declared_functions()
    for must in ("ts2d_forward_bin", "ts2d_forward_render", "ts2d_backward", "ts2d_geometry_state_bytes",
                 "ts2d_binning_state_bytes", "ts2d_image_state_bytes", "ts2d_backward_scratch_bytes", "ts2d_last_error",
                 "ts2d_version", "ts2d_forward_speculative", "ts2d_binning_capacity", "ts2d_instance_capacity_hint", "ts2d_sh_grad_expand", "tsl_workspace_bytes",
                 "tsl_photometric_forward", "tsl_photometric_backward", "tsk_workspace_bytes", "tsk_mean_dist3",
                 "tsk_nearest_other", "tsm_training_statistic", "tso_adam_step"):
        assert must in names


def test_library_exports_every_declared_symbol(lib):
    for name in _declared_functions():
        assert hasattr(lib, name), f"libts2d.so does not export {name}"


def test_product_library_reads_no_environment_and_has_one_blend_path(hip_lib_built):
    """libts2d.so carries one blend kernel family per variant (the lane-group kernels) and no run-time switch: the measurement
    kernels of earlier rounds and their TS2D_BLEND / TS2D_BWD / TS2D_ABLATE variables were removed and must not come back, nor
    the side-stream colour kernel of round 6."""
    import subprocess
    blob = open(hip_lib_built, "rb").read()
    for name in (b"TS2D_BLEND", b"TS2D_BWD", b"TS2D_ABLATE"):
        assert name not in blob, name
    syms = subprocess.run(["nm", "--defined-only", hip_lib_built], capture_output=True, text=True).stdout  # static table: the launchers are not exported
    launchers = sorted(set(re.findall(r"ts_launch_render\w*?(?=RK)", syms)))
    assert launchers, "nm found no blend launchers"
    assert all("group" in n for n in launchers), launchers
    assert "preprocess_colour" not in syms


def test_product_library_exports_only_the_declared_c_abi(hip_lib_built):
    """libts2d.so is built with -fvisibility=hidden: its dynamic symbol table holds the entry points that include/*.h declares and nothing
    else of ours -- no internal ts_* C++ symbol, no test hook (ts2d_test_*, ts2d_debug_*, ts2d_lab_*: csrc/ts2d_lab.h, lab library only),
    no rocPRIM."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", hip_lib_built], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = [n for n in exported if not n.startswith("__hip_")]  # __hip_cuid_*: the toolchain's per-object markers
    declared = set(_declared_functions())
    assert set(ours) == declared, (sorted(set(ours) - declared), sorted(declared - set(ours)))
    everything = subprocess.run(["nm", "-D", hip_lib_built], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    assert not re.search(r"ts2d_(test|debug|lab)_", everything)


def test_binning_capacity_inverts_the_size_query(lib):
    """The layout of a binning buffer follows from its size: capacity(bytes(N)) >= N, bytes(capacity(b)) <= b, monotone."""
    last = -1
    for n in (0, 1, 63, 4096, 4097, 262_145, 4_610_735, 50_000_000):
        b = lib.ts2d_binning_state_bytes(n, 1920, 1080)
        c = lib.ts2d_binning_capacity(b, 1920, 1080)
        assert c >= n and lib.ts2d_binning_state_bytes(c, 1920, 1080) <= b
        assert lib.ts2d_binning_state_bytes(c + 1, 1920, 1080) > b  # the LARGEST count that fits
        assert c >= last
        last = c
    assert lib.ts2d_binning_capacity(0, 1920, 1080) == 0 and lib.ts2d_binning_capacity(100, 64, 64) == 0


def test_state_size_queries_are_monotone_and_aligned(lib):
    a, b = lib.ts2d_geometry_state_bytes(1000), lib.ts2d_geometry_state_bytes(2000)
    assert 1000 * 64 <= a < b  # at least the 64-byte render record per triangle
    assert lib.ts2d_image_state_bytes(1920, 1080) >= 1920 * 1080 * 8 + 120 * 68 * 8
    assert lib.ts2d_backward_scratch_bytes(1000) >= 1000 * 64
    assert lib.ts2d_geometry_state_bytes(0) < 4096


def test_null_arguments_are_rejected_not_crashed(lib):
    rc = lib.ts2d_forward_bin(None, None, 0, None, None, None, None)
    assert rc == 1 and b"null" in lib.ts2d_last_error()


def test_triangle_count_beyond_the_id_bits_is_refused(lib):
    """The instance lists keep four bits of each value for the quadrant mask (csrc/ts2d_support.h): 2^28 triangles are a capacity error of the
    argument check, before any memory is touched."""
    from diff_triangle_rasterization_2D import _C
    cam, geom = _C._Camera(), _C._Geometry()
    cam.width, cam.height = 64, 64
    geom.P, geom.C, geom.M, geom.gamma = 1 << 28, 3, 0, 1.0
    n = ctypes.c_int64(0)
    rc = lib.ts2d_forward_bin(ctypes.byref(cam), ctypes.byref(geom), 0, None, None, ctypes.byref(n), None)
    assert rc == 3 and b"2^28" in lib.ts2d_last_error()  # TS2D_ERR_CAPACITY


# ---- Python surface: same names / order / errors as R2D/diff_triangle_rasterization_2D/__init__.py ----------
REFERENCE_SETTINGS_FIELDS = ("image_width", "image_height", "tanfovx", "tanfovy", "viewmatrix", "projmatrix", "campos",
                             "sh_degree", "gamma", "scale_modifier", "background_depth", "background", "back_culling",
                             "rich_info", "debug")  # reference __init__.py:28-46


def _settings(**kw):
    from diff_triangle_rasterization_2D import TriangleRasterizationSettings
    base = dict(image_width=32, image_height=32, tanfovx=0.3, tanfovy=0.3, viewmatrix=torch.eye(4), projmatrix=torch.eye(4),
                campos=torch.zeros(3), sh_degree=0, gamma=1.0, scale_modifier=1.0, background_depth=10.0,
                background=torch.zeros(3), back_culling=False, rich_info=True, debug=False)
    base.update(kw)
    return TriangleRasterizationSettings(**base)


def test_settings_namedtuple_matches_reference(hip_lib_built):
    from diff_triangle_rasterization_2D import TriangleRasterizationSettings
    assert TriangleRasterizationSettings._fields == REFERENCE_SETTINGS_FIELDS


def test_rasterizer_module_surface(hip_lib_built):
    from diff_triangle_rasterization_2D import TriangleRasterizer
    rs = _settings()
    r = TriangleRasterizer(rs)
    assert isinstance(r, torch.nn.Module) and r.raster_settings is rs  # read by triangle_renderer.py:77
    v, c2d, op = torch.rand(4, 3, 3), torch.zeros(4, 2), torch.rand(4, 1)
    with pytest.raises(Exception, match="excatly one"):  # reference __init__.py:180-181 (sic)
        r(v, c2d, op)
    with pytest.raises(Exception, match="excatly one"):
        r(v, c2d, op, shs=torch.rand(4, 1, 3), feature=torch.rand(4, 3))


def test_argument_checks_mirror_reference_errors(hip_lib_built):
    """extension_interface.cu:53-81: the same conditions raise RuntimeError with the same messages; tensors on the CPU
    are refused loudly (there is no CPU fallback in the product path)."""
    from diff_triangle_rasterization_2D import _C
    E = torch.Tensor([])

    def call(vertex=None, shs=None, feature=E, opacity=None, gamma=1.0, background=None, view=None):
        vertex = torch.rand(4, 3, 3) if vertex is None else vertex
        shs = torch.rand(4, 1, 3) if shs is None else shs
        opacity = torch.rand(4, 1) if opacity is None else opacity
        background = torch.zeros(3) if background is None else background
        view = torch.eye(4) if view is None else view
        return _C.rasterize_triangles(32, 32, 0.3, 0.3, view, torch.eye(4), torch.zeros(3), 0, gamma, 1.0, 10.0, background,
                                      vertex, shs, feature, opacity, False, True, False)

    with pytest.raises(RuntimeError, match=r"vertex must have dimensions \(num_points, 3, 3\)"):
        call(vertex=torch.rand(4, 3, 2))
    with pytest.raises(RuntimeError, match="num_channels can't be larger than MAX_CHANNELS"):
        call(shs=E, feature=torch.rand(4, 5), background=torch.zeros(5))
    with pytest.raises(RuntimeError, match="background must have the same number of channels"):
        call(background=torch.zeros(2))
    with pytest.raises(RuntimeError, match="gamma must be larger than 0"):
        call(gamma=-1.0)
    with pytest.raises(RuntimeError, match="input tensors must be contiguous"):
        call(view=torch.arange(16.0).view(4, 4).t())  # a transposed view, like camera.py:112 before .contiguous()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call()


def test_missing_library_fails_loudly(tmp_path, hip_lib_built):
    """The product must not degrade silently when the HIP library is absent, nor when the library is there but its torch extension is not."""
    import shutil
    import subprocess
    import sys
    pkg_src = os.path.join(ROOT, "triangle-splatting_amd", "diff_triangle_rasterization_2D")
    pkg = tmp_path / "diff_triangle_rasterization_2D"
    shutil.copytree(pkg_src, pkg, ignore=shutil.ignore_patterns("*.so", "__pycache__"))

    def imported():
        return subprocess.run([sys.executable, "-c", "import diff_triangle_rasterization_2D"], cwd=tmp_path, capture_output=True,
                              text=True, env={**os.environ, "PYTHONPATH": str(tmp_path)})
    r = imported()
    assert r.returncode != 0 and "libts2d.so" in r.stderr and "no CPU fallback" in r.stderr
    shutil.copy(hip_lib_built, pkg / "libts2d.so")  # the library, but no bindings/ beside the package
    r = imported()
    assert r.returncode != 0 and "_ts2d_torch_C.so" in r.stderr and "triangle-splatting_amd/build.py" in r.stderr


def _build_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ts2d_build", os.path.join(ROOT, "triangle-splatting_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_compiled_binding_is_built_with_the_library_and_loaded_by_the_package(hip_lib_built):
    """bindings/_ts2d_torch_C.so (torch C++ extension with the reference's ext.cpp signatures, linked against libts2d.so) builds
    without a GPU and exports the reference's two entry points (R2D/ext.cpp:4-9) plus the package's own two (`*_ex`: the same calls with the
    variant / capacity / preallocated-output arguments the package adds; diff_triangle_rasterization_2D/_C.py binds them)."""
    import importlib.util
    import torch  # noqa: F401
    build = _build_module()
    build.build()
    so = build.EXT
    spec = importlib.util.spec_from_file_location("_ts2d_torch_C", so)
    ext = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ext)
    assert sorted(n for n in dir(ext) if not n.startswith("_")) == ["rasterize_triangles", "rasterize_triangles_backward", "rasterize_triangles_backward_ex",
                                                                    "rasterize_triangles_ex"]
    from diff_triangle_rasterization_2D import _C
    assert os.path.samefile(_C._ext.__file__, so)
    with pytest.raises(RuntimeError):  # CPU tensors: the checks pass, the library refuses host pointers or the device guard raises
        z = torch.zeros
        ext.rasterize_triangles(8, 8, 0.3, 0.3, z(4, 4), z(4, 4), z(3), 0, 1.0, 1.0, 1.0, z(3), z(2, 3, 3), z(2, 1, 3), torch.empty(0), z(2, 1),
                                False, True, False)


_CHILD = """
import torch
from diff_triangle_rasterization_2D import _C
z = torch.zeros
try:
    _C.rasterize_triangles(8, 8, 0.3, 0.3, z(4, 4), z(4, 4), z(3), 0, 1.0, 1.0, 1.0, z(3), z(2, 3, 3), z(2, 1, 3), torch.empty(0), z(2, 1), False, True, False)
except RuntimeError as e:
    print("refused:", e)
print(open("/proc/self/maps").read())
"""


def _run_on_library(lib):
    import subprocess
    import sys
    env = {**os.environ, "PYTHONPATH": os.path.join(ROOT, "triangle-splatting_amd"), "TS2D_LIBRARY_PATH": str(lib)}
    return subprocess.run([sys.executable, "-c", _CHILD], capture_output=True, text=True, env=env)


def test_the_extension_calls_the_library_the_package_loaded(tmp_path, hip_lib_built):
    """TS2D_LIBRARY_PATH swaps the library under the extension too: the extension needs libts2d.so by name, every library build.py links has that
    soname, so the dynamic loader takes the one _C.py loaded first.  The product file is never mapped."""
    import shutil
    copy = tmp_path / "libts2d_copy.so"
    shutil.copy(hip_lib_built, copy)
    r = _run_on_library(copy)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "refused:" in r.stdout and "no CPU fallback" in r.stdout
    mapped = {l.split()[-1] for l in r.stdout.splitlines() if l.split()}  # the path ends each line of /proc/self/maps that has one
    assert os.path.realpath(copy) in mapped and os.path.realpath(_build_module().EXT) in mapped
    assert os.path.realpath(hip_lib_built) not in mapped


def test_a_library_without_the_soname_is_refused(tmp_path, hip_lib_built):
    """A library linked without the soname libts2d.so would leave the extension on the product library, a second instance: the import fails."""
    import subprocess
    build = _build_module()
    lib = tmp_path / "libts2d_nosoname.so"
    subprocess.run([build.hipcc(), "-shared", "-fPIC", f"--offload-arch={build.ARCH}", "-o", str(lib), *build.objects()], check=True)
    r = _run_on_library(lib)
    assert r.returncode != 0 and "lacks the soname libts2d.so" in r.stderr and "triangle-splatting_amd/build.py" in r.stderr


def _struct_mirrors():
    """C struct name -> its ctypes mirror, under the names the product modules use them by."""
    from diff_triangle_rasterization_2D import _C
    from diff_recon_hip import optim
    return {"ts2d_camera": _C._Camera, "ts2d_geometry": _C._Geometry, "ts2d_forward_out": _C._ForwardOut, "ts2d_loss_grads": _C._LossGrads,
            "ts2d_backward_out": _C._BackwardOut, "ts2d_state": _C._State, "tso_adam_slice": optim._Slice, "tso_row_slice": optim._RowSlice,
            "tso_sh_factored_step": optim._ShFactoredStep}


def test_ctypes_structures_match_the_c_headers(tmp_path, hip_lib_built):
    """The ctypes mirrors of the C ABI's structs (diff_triangle_rasterization_2D/_abi.py) against the headers themselves:
    a probe compiled with gcc from include/*.h prints sizeof / offsetof of every field; a field added to a header but not to its mirror (or
    the other way round) fails here, without a GPU."""
    import subprocess
    from diff_triangle_rasterization_2D import _C
    from diff_recon_hip import optim
    mirrors = _struct_mirrors()
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ts2d.h"', '#include "ts_optim.h"', 'int main(void) {']
    for cname, mirror in mirrors.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in mirror._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out.splitlines()}
    for cname, mirror in mirrors.items():
        assert got[(cname, "size")] == ctypes.sizeof(mirror), cname
        for fname, _ in mirror._fields_:
            assert got[(cname, fname)] == getattr(mirror, fname).offset, (cname, fname)
    # and the header has no field the mirror lacks: the sizes above already say so for trailing fields; count the declarators for the rest
    for cname, mirror, header in [("ts2d_geometry", _C._Geometry, "ts2d.h"), ("tso_adam_slice", optim._Slice, "ts_optim.h")]:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        body = re.search(r"typedef struct " + cname + r"\s*\{(.*?)\}\s*" + cname + r"\s*;", text, flags=re.S).group(1)
        declared = [n for stmt in body.split(";") for n in re.findall(r"\**\s*([A-Za-z_]\w*)\s*(?:,|$)", stmt.strip().split(None, 1)[-1] if stmt.strip() else "")]
        assert len(declared) == len(mirror._fields_), (cname, declared, [f for f, _ in mirror._fields_])


def test_binning_state_bytes_grow_with_the_capacity_and_invert(lib):
    """The forward and the backward both carve the binning state from the BUFFER'S SIZE (ts2d_binning_capacity inverts ts2d_binning_state_bytes by
    bisection), so the bytes must never shrink when the capacity grows -- also across the capacities at which the instance sort changes its chunk
    length (csrc/ts2d_common.h: ts_instance_chunk; the tables are sized for the shortest chunks at every capacity for exactly this reason)."""
    for W, H in ((1920, 1080), (256, 256), (37, 5)):
        caps = sorted(set(list(range(0, 70000, 997)) + list(range(2_499_000, 2_501_001, 125)) + [1 << k for k in range(4, 27)] +
                          [(1 << k) + 1 for k in range(4, 27)] + [4_610_000, 12_600_000, 23_000_000]))
        prev = -1
        for n in caps:
            b = lib.ts2d_binning_state_bytes(n, W, H)
            assert b >= 16 * n and b >= prev, (n, b, prev)
            prev = b
        for n in (0, 1, 1023, 1024, 1025, 65_537, 2_499_999, 2_500_000, 2_500_001, 4_610_000):
            b = lib.ts2d_binning_state_bytes(n, W, H)
            cap = lib.ts2d_binning_capacity(b, W, H)
            assert cap >= n and lib.ts2d_binning_state_bytes(cap, W, H) <= b, (n, b, cap)  # the largest capacity whose carving fits the buffer


# ---- every ctypes signature against its prototype ---------------------------------------------------------------------------------------
LAB_HEADER = os.path.join(ROOT, "triangle-splatting_amd", "csrc", "ts2d_lab.h")
_C_SCALARS = {"int": ("signed", ctypes.sizeof(ctypes.c_int)), "int32_t": ("signed", 4), "int64_t": ("signed", 8), "uint8_t": ("unsigned", 1),
              "uint32_t": ("unsigned", 4), "uint64_t": ("unsigned", 8), "size_t": ("unsigned", ctypes.sizeof(ctypes.c_size_t)),
              "unsigned long long": ("unsigned", ctypes.sizeof(ctypes.c_ulonglong)), "float": ("floating", 4), "double": ("floating", 8)}


def _c_type(decl, named):
    """(base type without qualifiers, number of `*`) of one C99 declarator: a return type (named = False) or a parameter with its name."""
    stars = decl.count("*")
    words = [w for w in decl.replace("*", " ").split() if w != "const"]
    if named and len(words) > 1:
        words = words[:-1]  # the parameter's name
    return " ".join(words), stars


def _prototypes(path):
    """name -> (return type, [parameter types]) of every ts2d_ / tsl_ / tsk_ / tsm_ / tso_ prototype of a header, comments and directives stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^[ \t]*#[^\n]*$", "", text, flags=re.M)
    found = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\n*]*?)\b((?:ts2d|tsl|tsk|tsm|tso)_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = [" ".join(p.split()) for p in params.split(",")]
        assert name not in found, name
        found[name] = (_c_type(" ".join(ret.split()), False), [] if params == ["void"] else [_c_type(p, True) for p in params])
    return found


def _scalar_kind(ct):
    code = getattr(ct, "_type_", None)
    if not isinstance(code, str) or code not in "bhilqBHILQfd":
        return None
    return ("floating" if code in "fd" else "signed" if code.islower() else "unsigned", ctypes.sizeof(ct))


def _mismatch(c, ct, mirrors):
    """Why the ctypes type `ct` does not stand for the C type c = (base, stars), or None when it does.  c_int32 IS c_int here, so scalars are
    compared by kind and size; a typed pointer must point at the mirror of that very C type."""
    base, stars = c
    if stars == 0:
        if base == "void":
            return None if ct is None else f"void, got {ct}"
        return None if ct is not None and _scalar_kind(ct) == _C_SCALARS[base] else f"{base} is {_C_SCALARS[base]}, got {ct}"
    if ct is ctypes.c_void_p:
        return None
    if ct is ctypes.c_char_p:
        return None if (base, stars) == ("char", 1) else f"c_char_p for {base} {'*' * stars}"
    pointee = getattr(ct, "_type_", None)
    if not isinstance(ct, type) or not issubclass(ct, ctypes._Pointer):
        return f"{base} {'*' * stars} needs a pointer, got {ct}"
    if stars > 1:
        return None if pointee is ctypes.c_void_p else f"an array of pointers is POINTER(c_void_p), got POINTER({pointee})"
    if base in mirrors:
        return None if pointee is mirrors[base] else f"{base} * points at {mirrors[base].__name__}, got POINTER({pointee.__name__})"
    if base in _C_SCALARS:
        return None if _scalar_kind(pointee) == _C_SCALARS[base] else f"{base} * points at {_C_SCALARS[base]}, got POINTER({pointee})"
    return f"no typed pointer stands for {base} *"


def _signature_problems(proto, signature, mirrors):
    (c_ret, c_params), (restype, argtypes) = proto, signature
    problems = []
    why = _mismatch(c_ret, restype, mirrors)
    if why:
        problems.append(f"restype: {why}")
    if len(c_params) != len(argtypes):
        return problems + [f"arity: the header has {len(c_params)} parameters, the table {len(argtypes)}"]
    for i, (c, ct) in enumerate(zip(c_params, argtypes)):
        why = _mismatch(c, ct, mirrors)
        if why:
            problems.append(f"argument {i}: {why}")
    return problems


def test_ctypes_signatures_match_the_c_headers(lib):
    """diff_triangle_rasterization_2D/_abi.py declares restype / argtypes of the whole C ABI once; here every entry is held against its
    prototype in include/*.h (and csrc/ts2d_lab.h): the same set of names, the same arity, every scalar of the same kind and size, every typed
    pointer at the mirror of that very C type.  A float where the header says double, or one pointer too few, would be a wild kernel argument."""
    from diff_triangle_rasterization_2D import _abi
    mirrors = _struct_mirrors()
    product = {}
    for h in HEADERS:
        protos = _prototypes(h)
        assert not set(protos) & set(product), sorted(set(protos) & set(product))
        product.update(protos)
    lab = _prototypes(LAB_HEADER)
    assert set(product) == set(_declared_functions()) and len(product) == 76, len(product)  # the parser skipped no prototype
    assert set(product) == set(_abi.SIGNATURES), sorted(set(product) ^ set(_abi.SIGNATURES))
    assert set(lab) == set(_abi.LAB_SIGNATURES), sorted(set(lab) ^ set(_abi.LAB_SIGNATURES))
    for protos, table in ((product, _abi.SIGNATURES), (lab, _abi.LAB_SIGNATURES)):
        for name, proto in protos.items():
            assert _signature_problems(proto, table[name], mirrors) == [], name
    for name, (restype, argtypes) in _abi.SIGNATURES.items():  # and bind() sets both attributes, explicitly, on every function
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # the comparator itself: three corruptions of one entry, each must be reported
    restype, argtypes = _abi.SIGNATURES["tso_adam_step"]
    proto = product["tso_adam_step"]
    assert _signature_problems(proto, (restype, argtypes), mirrors) == []
    as_float = [ctypes.c_float if a is ctypes.c_double else a for a in argtypes]
    assert as_float != list(argtypes) and any("double" in p for p in _signature_problems(proto, (restype, as_float), mirrors))
    assert any("arity" in p for p in _signature_problems(proto, (restype, list(argtypes)[:-1]), mirrors))
    wrong_struct = [ctypes.POINTER(mirrors["ts2d_camera"])] + list(argtypes)[1:]
    assert any("tso_adam_slice" in p for p in _signature_problems(proto, (restype, wrong_struct), mirrors))
