"""CPU tests of the TSDF volume and the marching tetrahedra (no GPU): the numpy reference keeps the promises of include/ts_volume.h (closed,
oriented, order-independent), the kernel carries the reference's tables, libts_volume.so is a library of its own with exactly the C ABI of
the header, and every argument check answers before any HIP call."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ref_volume as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_volume.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tsv_extract", "tsv_extract_workspace_bytes", "tsv_field", "tsv_integrate", "tsv_last_error"]
DIMS, CENTRE = (12, 12, 12), (5.3, 5.6, 5.45)


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_volume", ("diff_triangle_rasterization_2D", "_abi.py"))


VOLUME_SIGNATURES = _abi_module().VOLUME_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def volume_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_volume.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_volume.so"
    return path


@pytest.fixture(scope="module")
def lib(volume_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_volume(ctypes.CDLL(volume_path))


def _header_prototypes():
    """name -> number of parameters of every tsv_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


def _mesh(field, dims=DIMS):
    tri, cell = ref.extract(field, dims, (0, 0, 0), 1.0)
    verts, faces = ref.weld_exact(tri)
    return tri, cell, verts, ref.topology(faces)


# ---- the reference holds the contract's promises -------------------------------------------------------------------------------------------
def test_flip_table_is_derived_and_every_case_is_consistent():
    assert ref.FLIP == (0x4d24, 0x32da, 0x32da, 0x4d24, 0x4d24, 0x32da)
    assert ref.TRIANGLES_OF_CASE == (0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0)
    for bits in ref.FLIP:  # a case and its complement have opposite normals: the single triangles list the same vertices in the same order,
        for mask in range(1, 15):  # the quads list them the other way round already
            same_order = ref.TRIANGLES_OF_CASE[mask] == 1
            assert ((bits >> mask & 1) != (bits >> (15 - mask) & 1)) == same_order
    for tet in ref.TETS:  # a path 0 -> 7 along three axes, corners ascending
        assert tet[0] == 0 and tet[3] == 7 and list(tet) == sorted(tet)
        assert all(bin(tet[m + 1] - tet[m]).count("1") == 1 for m in range(3))


def test_kernel_carries_the_reference_tables():
    text = open(os.path.join(ROOT, "triangle-splatting_amd", "csrc", "volume.hip")).read()

    def numbers(name):
        body = re.search(name + r"(?:\[\d+\])?\s*=\s*\{?([^;]*?)\}?;", text, flags=re.S).group(1)
        return [int(x.rstrip("u"), 16) for x in re.findall(r"0x[0-9a-fA-F]+u?", body)]

    assert tuple(numbers("FLIP_BITS")) == ref.FLIP
    assert numbers("CASE_COUNTS") == [sum(n << (2 * m) for m, n in enumerate(ref.TRIANGLES_OF_CASE))]
    assert numbers("TET_CORNERS") == [sum(c << (4 * p) for p, c in enumerate(tet)) for tet in ref.TETS]
    want = []
    for mask in range(16):
        word, shift = 0, 0
        for tri in ref.case_triangles(mask):
            for p, q in tri:
                word |= (min(p, q) | max(p, q) << 2) << shift
                shift += 4
        want.append(word)
    assert numbers("CASE_EDGES") == want


def test_sphere_is_closed_oriented_and_inscribed():
    tri, cell, verts, topo = _mesh(ref.sphere_field(DIMS, CENTRE, 3.7))
    assert len(tri) == 1548 and len(verts) == 776 and topo["edges"] == 2322
    assert topo["boundary"] == 0 and topo["nonmanifold"] == 0  # every edge is used by exactly two faces
    assert topo["directed_repeats"] == 0                        # ... once in each direction: consistently oriented
    assert topo["euler"] == 2
    volume, analytic = ref.signed_volume(tri), 4.0 / 3.0 * np.pi * 3.7 ** 3
    print("signed volume", volume, "analytic", analytic)
    assert volume > 0 and 0.93 * analytic < volume < analytic  # outward normals; the polyhedron is inscribed
    assert abs(volume - 204.38) < 0.01
    assert (np.diff(cell) >= 0).all() and tri.dtype == np.float32


def test_torus_is_closed_with_euler_zero():
    tri, _, _, topo = _mesh(ref.torus_field(DIMS, CENTRE, 3.4, 1.3))
    assert len(tri) == 1372
    assert topo["boundary"] == 0 and topo["nonmanifold"] == 0 and topo["directed_repeats"] == 0 and topo["euler"] == 0
    assert ref.signed_volume(tri) > 0


def test_nan_samples_open_the_surface_without_breaking_it():
    f = ref.sphere_field(DIMS, CENTRE, 3.7).reshape(12, 12, 12).copy()
    f[:, :, :6] = np.nan  # samples i < 6
    tri, _, verts, topo = _mesh(f.reshape(-1))
    assert len(tri) > 0 and topo["boundary"] > 0 and topo["nonmanifold"] == 0 and topo["directed_repeats"] == 0
    assert (verts[:, 0] >= 6).all()
    f[:, :, 6:] = np.inf
    assert len(ref.extract(f.reshape(-1), DIMS, (0, 0, 0), 1.0)[0]) == 0


def test_shared_edges_get_the_same_bits_off_the_origin_too():
    """An origin and spacing that are no powers of two: the vertex is still a function of the edge alone."""
    f = ref.sphere_field((9, 8, 7), (3.9, 3.4, 2.8), 2.3)
    tri, _ = ref.extract(f, (9, 8, 7), (0.1, -0.7, 3.3), 0.3, iso=0.05)
    _, faces = ref.weld_exact(tri)
    topo = ref.topology(faces)
    assert len(tri) > 100 and topo["boundary"] == 0 and topo["nonmanifold"] == 0 and topo["euler"] == 2


def test_fusion_of_six_views_carving_closes_the_sphere():
    s, w, dims, origin, h = ref.fuse_sphere(carve=True)
    s2, w2, *_ = ref.fuse_sphere(order=(5, 3, 1, 4, 2, 0), carve=True)
    assert np.array_equal(s, s2) and np.array_equal(w, w2)  # integers: any order
    tri, _ = ref.extract(ref.field(s, w), dims, origin, h)
    topo = ref.topology(ref.weld_exact(tri)[1])
    assert topo["boundary"] == 0 and topo["nonmanifold"] == 0 and topo["directed_repeats"] == 0 and topo["euler"] == 2
    volume, analytic = ref.signed_volume(tri), 4.0 / 3.0 * np.pi * 0.6 ** 3
    print("fused volume", volume, "analytic", analytic)
    assert abs(volume - 0.880) < 0.001 and abs(analytic - 0.905) < 0.001


def test_fusion_without_carving_stays_open():
    s, w, dims, origin, h = ref.fuse_sphere(carve=False)
    s2, w2, *_ = ref.fuse_sphere(order=(2, 0, 4, 1, 5, 3), carve=False)
    assert np.array_equal(s, s2) and np.array_equal(w, w2)
    tri, _ = ref.extract(ref.field(s, w), dims, origin, h)
    topo = ref.topology(ref.weld_exact(tri)[1])
    assert topo["boundary"] == 456 and topo["nonmanifold"] == 0  # what the flag is for


def test_integrate_skips_what_the_header_says():
    dims, n = (4, 3, 2), 24
    M = ref.look_at_view((0, 0, -3))
    depth = np.full((8, 8), 3.0, np.float32)
    s, w = np.zeros(n, np.int64), np.zeros(n, np.int32)
    assert ref.integrate(s, w, dims, (-0.2, -0.1, -0.05), 0.1, 0.4, M, 0.45, 0.45, 8, 8, depth) == n
    assert (w == 1).all() and (s != 0).any() and (np.abs(s) <= 1 << 20).all()
    for bad in (np.nan, np.inf, -1.0):
        s[:], w[:] = 0, 0
        assert ref.integrate(s, w, dims, (-0.2, -0.1, -0.05), 0.1, 0.4, M, 0.45, 0.45, 8, 8, np.full((8, 8), bad, np.float32)) == 0
    zero = np.zeros((8, 8), np.float32)
    assert ref.integrate(s, w, dims, (-0.2, -0.1, -0.05), 0.1, 0.4, M, 0.45, 0.45, 8, 8, zero) == 0
    assert ref.integrate(s, w, dims, (-0.2, -0.1, -0.05), 0.1, 0.4, M, 0.45, 0.45, 8, 8, zero, flags=ref.CARVE_UNCOVERED) == n
    assert (s == 1 << 20).all()
    assert ref.integrate(s, w, dims, (-0.2, -0.1, -0.05), 0.1, 0.4, M, 0.45, 0.45, 8, 8, depth, mask=np.zeros((8, 8), np.uint8)) == 0
    assert ref.integrate(s, w, dims, (-0.2, -0.1, -0.05), 0.1, 0.4, M, 0.45, 0.45, 8, 8, np.full((8, 8), 2.0, np.float32)) == 0  # behind: sd < -trunc
    w[:5] = ref.INT32_MAX
    assert ref.integrate(s, w, dims, (-0.2, -0.1, -0.05), 0.1, 0.4, M, 0.45, 0.45, 8, 8, depth) == n - 5
    assert ref.integrate(s, w, dims, (-0.2, -0.1, -5.0), 0.1, 0.4, M, 0.45, 0.45, 8, 8, depth) == 0  # z <= 0: behind the camera
    f = ref.field(np.array([1 << 19, 3 << 20, 0], np.int64), np.array([1, 4, 0], np.int32), 2)
    assert np.isnan(f[0]) and f[1] == 0.75 and np.isnan(f[2])


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(volume_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsv_last_error.restype = ctypes.c_char_p; "
            "l.tsv_extract_workspace_bytes.restype = ctypes.c_size_t; print(l.tsv_extract_workspace_bytes(100, 100, 100) >= 1000000, "
            "repr(l.tsv_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, volume_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(volume_path):
    out = subprocess.run(["nm", "-D", "--defined-only", volume_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", volume_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", volume_path], capture_output=True, text=True).stdout
    assert "libts_volume.so" in dynamic
    for other in ("libts2d.so", "libts_geom.so", "libts_bvh.so", "libts_ray.so"):
        assert other not in dynamic


def test_header_text_stays_out_of_the_other_libraries_lists_and_defines_no_struct():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr)_[a-z0-9_]+)\s*\(", text)
    assert "struct" not in text
    full = open(HEADER).read()
    for word in ("(0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7) (0,4,5,7) (0,4,6,7)", "-ffp-contract=off", "TSV_CARVE_UNCOVERED", "INT32_MAX", "2^27",
                 "function of the edge alone"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(VOLUME_SIGNATURES)
    for name, arity in declared.items():
        assert len(VOLUME_SIGNATURES[name][1]) == arity, name
    assert declared["tsv_integrate"] == 20 and declared["tsv_extract"] == 16
    abi = _abi_module()
    tables = [abi.SIGNATURES, abi.LAB_SIGNATURES, abi.GEOM_SIGNATURES, abi.BVH_SIGNATURES, abi.RAY_SIGNATURES, abi.VOLUME_SIGNATURES]
    for a in range(len(tables)):
        for b in range(a + 1, len(tables)):
            assert not set(tables[a]) & set(tables[b])  # no signature table overlaps another
    assert VOLUME_SIGNATURES["tsv_extract"][1][9] == ctypes.c_int64 and VOLUME_SIGNATURES["tsv_integrate"][1][3:8] == [ctypes.c_float] * 5


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_volume", ("build.py",))
    assert list(build.VOLUME_SOURCES) == ["volume.hip", "api_volume.hip"]
    assert "-ffp-contract=off" in build.VOLUME_SOURCES["volume.hip"]
    assert build.volume_units() == ["volume", "api_volume"]
    cmd = build.volume_command("volume", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert build.volume_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("volume", "api_volume")]  # no product object is reused
    for others in (build.units(), build.geom_units(), build.bvh_units(), build.ray_units()):
        assert not {"volume", "api_volume"} & set(others)  # its own library only
    assert build.VOLUME_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_volume.so")
    for header in ("ts_volume_launch.h", os.path.join("..", "..", "include", "ts_volume.h")):
        assert header in build.HEADERS
    with pytest.raises(ValueError):
        build.volume_command("mesh_ray")


def test_built_objects_carry_the_flags(volume_path):
    build = _load("ts2d_build_volume2", ("build.py",))
    assert "-ffp-contract=off" in open(os.path.join(build.OBJ_DIR, "volume.o.cmd")).read()  # what the object on disk was compiled with
    assert "-soname,libts_volume.so" in open(build.VOLUME_LIB + ".cmd").read()


def test_size_query_is_monotone_and_covers_counts_and_sums(lib):
    prev = -1
    for n in (1, 2, 3, 7, 16, 40, 100, 255, 256, 257, 400, 512):
        got = lib.tsv_extract_workspace_bytes(n, n, n)
        samples = n ** 3
        blocks = -(-samples // 256)
        assert got >= samples + 4 * blocks + 4 * -(-blocks // 1024) and got >= prev, (n, got, prev)
        prev = got
    assert lib.tsv_extract_workspace_bytes(512, 512, 512) == lib.tsv_extract_workspace_bytes(1 << 27, 1, 1)  # a function of the sample count


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    big = 1 << 40
    nan, inf = float("nan"), float("inf")

    def refused(rc, word, code=INVALID):
        assert rc == code, rc
        text = lib.tsv_last_error()
        assert text and word.encode() in text, text

    def integrate(nx=4, ny=4, nz=4, h=0.1, trunc=0.4, view=P, tx=0.5, ty=0.5, W=8, H=8, depth=P, mask=None, flags=0, s=P, w=P, updated=None):
        return lib.tsv_integrate(nx, ny, nz, 0.0, 0.0, 0.0, h, trunc, view, tx, ty, W, H, depth, mask, flags, s, w, updated, None)

    def field(nx=4, ny=4, nz=4, s=P, w=P, min_weight=1, out=P):
        return lib.tsv_field(nx, ny, nz, s, w, min_weight, out, None)

    def extract(nx=4, ny=4, nz=4, h=0.1, fld=P, iso=0.0, capacity=10, tri=P, cell=None, total=P, ws=P, ws_bytes=big):
        return lib.tsv_extract(nx, ny, nz, 0.0, 0.0, 0.0, h, fld, iso, capacity, tri, cell, total, ws, ws_bytes, None)

    for call in (integrate, field, extract):
        for dims in ({"nx": 0}, {"ny": -1}, {"nz": 0}, {"nx": -(2 ** 31)}):
            refused(call(**dims), ">= 1")
        refused(call(nx=1 << 14, ny=1 << 13, nz=2), "2^27", CAPACITY)  # 2^28 samples
        refused(call(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1), "2^27", CAPACITY)
        refused(call(nx=(1 << 27) + 1, ny=1, nz=1), "2^27", CAPACITY)
    for call in (integrate, extract):
        for bad in (0.0, -0.1, nan, inf, -inf):
            refused(call(h=bad), "h must be finite and > 0")
    for bad in (0.0, -1.0, nan, inf):
        refused(integrate(trunc=bad), "trunc must be finite and > 0")
        refused(integrate(tx=bad), "tan_fovx")
        refused(integrate(ty=bad), "tan_fovy")
    refused(integrate(W=0), "W and H")
    refused(integrate(H=-3), "W and H")
    refused(integrate(W=1 << 16, H=1 << 15), "2^31 - 1", CAPACITY)
    refused(integrate(flags=2), "flags")
    refused(integrate(flags=-1), "flags")
    for name in ("view", "depth", "s", "w"):
        refused(integrate(**{name: None}), "null")
    for name in ("s", "w", "out"):
        refused(field(**{name: None}), "null")
    refused(field(min_weight=0), "min_weight")
    refused(field(min_weight=-5), "min_weight")
    refused(extract(fld=None), "null")
    refused(extract(total=None), "null")
    refused(extract(tri=None), "triangles is null")
    refused(extract(ws=None), "workspace is null")
    refused(extract(capacity=-1), "capacity")
    refused(extract(iso=nan), "iso")
    refused(extract(iso=inf), "iso")
    need = lib.tsv_extract_workspace_bytes(40, 30, 20)
    refused(extract(nx=40, ny=30, nz=20, ws_bytes=need - 1), "workspace too small")
    assert str(need).encode() in lib.tsv_last_error()
    assert lib.tsv_extract_workspace_bytes(1 << 9, 1 << 9, 1 << 9) > 1 << 27  # the largest grid has a size


def test_missing_library_is_an_import_error_and_the_package_still_imports(tmp_path, volume_path):
    """Without libts_volume.so, diff_recon_hip.volume raises and names the build command; everything else still imports."""
    src = os.path.dirname(volume_path)
    pkg = tmp_path / "diff_recon_hip"
    pkg.mkdir()
    for name in os.listdir(src):
        if name.endswith(".py") or name in ("libts_geom.so", "libts_bvh.so", "libts_ray.so"):
            shutil.copy(os.path.join(src, name), pkg / name)
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([str(tmp_path), os.path.join(ROOT, "triangle-splatting_amd")])}
    code = ("import diff_recon_hip, sys\n"
            "assert str(diff_recon_hip.__file__).startswith(sys.argv[1]), diff_recon_hip.__file__\n"
            "print('others', callable(diff_recon_hip.weld_mesh), callable(diff_recon_hip.ray_cast))\n"
            "try:\n    diff_recon_hip.TSDFVolume\nexcept ImportError as e:\n    print('lazy', e)\n"
            "import diff_recon_hip.volume\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, env=env)
    assert "others True True" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert "lazy" in r.stdout and "libts_volume.so" in r.stdout
    assert r.returncode != 0 and "ImportError" in r.stderr
    assert "libts_volume.so" in r.stderr and "no CPU fallback" in r.stderr and "triangle-splatting_amd/build.py" in r.stderr


def test_package_re_exports_the_feature(volume_path):
    import diff_recon_hip
    from diff_recon_hip import volume
    for name in ("TSDFVolume", "extract_isosurface", "fuse_mesh"):
        assert getattr(diff_recon_hip, name) is getattr(volume, name)
    assert diff_recon_hip.volume is volume
    import inspect
    assert list(inspect.signature(volume.TSDFVolume.__init__).parameters)[1:] == ["origin", "voxel_size", "dims", "trunc", "device"]
    assert list(inspect.signature(volume.TSDFVolume.integrate).parameters)[1:5] == ["cam", "depth", "mask", "carve_uncovered"]
    assert list(inspect.signature(volume.TSDFVolume.extract).parameters)[1:] == ["min_weight", "iso", "weld"]
    assert list(inspect.signature(volume.extract_isosurface).parameters)[:4] == ["field", "origin", "voxel_size", "iso"]
    assert list(inspect.signature(volume.fuse_mesh).parameters)[:5] == ["views", "vertices", "faces", "resolution", "trunc"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        volume.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), 0.4, device="cpu")


def test_example_refuses_extract_mesh_without_eval_mesh():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), "--extract-mesh", "32"], capture_output=True, text=True)
    assert r.returncode == 2 and "--extract-mesh fuses the mesh of --eval-mesh" in r.stderr
