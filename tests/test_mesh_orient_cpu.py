"""CPU tests of the consistent orientation (no GPU): the numpy reference finds the same pieces and flips by a union-find over the doubled
graph and by a breadth-first walk that carries a parity, and keeps the promises of include/ts_orient.h on every fixture; a scrambled sphere
comes back as it was; a Moebius strip is one non-orientable piece; libts_orient.so is a library of its own with exactly the C ABI of the
header, and every argument check answers before any HIP call."""
import ctypes
import functools
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_manifold
import ref_mesh_orient as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_orient.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tsw_last_error", "tsw_orient", "tsw_workspace_bytes"]
MAX_FACES = 715827882


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_orient", ("diff_triangle_rasterization_2D", "_abi.py"))


ORIENT_SIGNATURES = _abi_module().ORIENT_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def orient_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_orient.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_orient.so"
    return path


@pytest.fixture(scope="module")
def lib(orient_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_orient(ctypes.CDLL(orient_path))


def _header_prototypes():
    """name -> number of parameters of every tsw_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsw_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


# ---- the fixtures: computed once, never changed ---------------------------------------------------------------------------------------------------
def _positions(V):
    return np.random.default_rng(V).uniform(-1, 1, (V, 3)).astype(np.float32)


def _indexed(builder):
    V, f = builder()[:2]
    return _positions(V), f


def _scrambled(builder, seed):
    v, f = builder()
    return v, ref.scramble(f, seed)[0]


FIXTURES = {
    "strip3": lambda: _scrambled(lambda: ref.strip(3), 1),
    "strip128": lambda: _scrambled(lambda: ref.strip(128), 2),
    "moebius3": lambda: _scrambled(lambda: ref.strip(3, True), 3),
    "moebius129": lambda: _scrambled(lambda: ref.strip(129, True), 4),
    "torus": lambda: _scrambled(lambda: ref.grid(9, 7), 5),
    "klein": lambda: _scrambled(lambda: ref.grid(8, 6, klein=True), 6),
    "sphere": lambda: _scrambled(ref.latlong_sphere, 7),
    "book": lambda: _indexed(lambda: ref_mesh_manifold.book(5)),
    "hub": lambda: _indexed(lambda: ref_mesh_manifold.hub(5)),
    "tetrahedra": lambda: _indexed(ref_mesh_manifold.two_tetrahedra),
    "soup63": lambda: (_positions(63), ref_mesh_manifold.soups()[63]),
    "soup257": lambda: (_positions(257), ref_mesh_manifold.soups()[257]),
    "soup1025": lambda: (_positions(1025), ref_mesh_manifold.soups()[1025]),
    "mixed": lambda: ref.mixed_mesh()[:2],
}


@functools.lru_cache(maxsize=None)
def _case(name):
    v, f = FIXTURES[name]()
    return v, f, {mode: ref.check_promises(len(v), f, None, mode, v) for mode in ref.MODES}  # both forms of the reference, the promises


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_union_find_and_walking_agree_and_the_promises_hold(name):
    v, f, by_mode = _case(name)
    F = len(f)
    for mode, (first, second) in by_mode.items():
        c = first["counts"]
        assert first["face_piece"].shape == (F,) and first["face_piece"].dtype == np.int32
        assert first["face_flip"].shape == (F,) and first["face_flip"].dtype == np.uint8 and set(first["face_flip"].tolist()) <= {0, 1}
        assert first["out_faces"].shape == (F, 3) and first["out_faces"].dtype == np.int32
        piece = first["face_piece"]
        part = piece >= 0
        assert (piece[part] <= np.nonzero(part)[0]).all() and (piece[piece[part]] == piece[part]).all()  # the smallest face, itself an anchor
        assert c[0] == part.sum() and c[1] == len(np.unique(piece[part])) and c[5] >= c[6] and c[3] >= c[2]
        assert np.array_equal(first["out_faces"][:, 0], np.asarray(f)[:, 0].astype(np.int32))            # slot 0 stays
        assert np.array_equal(np.sort(first["out_faces"], 1), np.sort(np.asarray(f), 1).astype(np.int32))
        if mode != "volume":
            assert c[9] == 0
        print(f"{name}, {mode}: {dict(zip(ref.COUNT_NAMES, c))}")
    pieces = [by_mode[m][0]["face_piece"] for m in ref.MODES]
    assert np.array_equal(pieces[0], pieces[1]) and np.array_equal(pieces[0], pieces[2])
    anchor = by_mode["anchor"][0]
    assert anchor["counts"][8] == 0 and not anchor["face_flip"][np.unique(anchor["face_piece"][anchor["face_piece"] >= 0])].any()


def test_face_piece_does_not_depend_on_the_winding():
    v, f, _, _ = ref.mixed_mesh()
    base = ref.orient(len(v), f, None, "anchor")
    for seed in (1, 2):
        g = ref.scramble(f, seed, permute=False)[0]
        got = ref.orient(len(v), g, None, "anchor")
        assert np.array_equal(got["face_piece"], base["face_piece"]) and got["counts"][:5] == base["counts"][:5]
        assert np.array_equal(got["nonorientable"], base["nonorientable"])


@pytest.mark.parametrize("mode,fraction", [("volume", 0.5), ("volume", 0.9), ("majority", 0.3)])
def test_scrambled_outward_sphere_comes_back(mode, fraction):
    v, f = ref.latlong_sphere()
    assert ref.signed_volume(v, f) > 0
    g, mask, order = ref.scramble(f, 11, fraction)
    assert 0 < mask.sum() < len(f) and (mode != "majority" or 2 * mask.sum() < len(f))
    out = ref.orient(len(v), g, None, mode, v)
    assert np.array_equal(out["out_faces"], f[order].astype(np.int32))              # equal to the unscrambled rows
    assert np.array_equal(out["face_flip"], mask.astype(np.uint8)) and out["counts"][7] == mask.sum()
    assert out["counts"][:4] == [len(f), 1, 0, 0] and out["counts"][5] > 0 and out["counts"][6] == 0
    if mode == "volume":
        assert out["S"][0] != 0 and 2 ** 40 < abs(out["S"][0]) < 2 ** 59
    same = ref.orient(len(v), f, None, mode, v)                                    # consistent and non-negative: bit for bit
    assert np.array_equal(same["out_faces"], f.astype(np.int32)) and same["counts"][5:9] == [0, 0, 0, 0]
    inward = ref.orient(len(v), f[:, [0, 2, 1]], None, "volume", v)
    assert np.array_equal(inward["out_faces"], f.astype(np.int32)) and inward["counts"][7:9] == [len(f), 1]


def test_small_sphere_far_from_the_origin_is_as_well_resolved_as_a_large_one():
    sums = []
    for radius, centre in ((0.6, (0, 0, 0)), (0.002, (50.0, 0, 0)), (300.0, (-1e4, 3e3, 7.0))):
        v, f = ref.latlong_sphere(radius=radius, centre=centre)
        inward = ref.orient(len(v), f[:, [0, 2, 1]], None, "volume", v)
        assert np.array_equal(inward["out_faces"], f.astype(np.int32)) and inward["counts"][8] == 1
        sums.append(abs(inward["S"][0]))
    print("|S_p|:", [f"2^{np.log2(s):.1f}" for s in sums])
    assert all(2 ** 40 < s < 2 ** 59 for s in sums)


@pytest.mark.parametrize("n", [3, 4, 37, 129])
def test_moebius_strip_is_one_nonorientable_piece_and_is_unchanged(n):
    v, f = ref.strip(n, twist=True)
    g = ref.scramble(f, n)[0]
    for faces in (f, g):
        for mode in ref.MODES:
            out = ref.orient(len(v), faces, None, mode, v)
            assert out["counts"][:5] == [2 * n, 1, 1, 2 * n, 2 * n] and out["counts"][7:9] == [0, 0]
            assert out["counts"][5] == out["counts"][6] > 0 and not out["face_flip"].any()
            assert np.array_equal(out["out_faces"], faces.astype(np.int32)) and (out["face_piece"] == 0).all()
    plain = ref.orient(len(v), ref.scramble(ref.strip(n)[1], n)[0], None, "majority")
    assert plain["counts"][:4] == [2 * n, 1, 0, 0] and plain["counts"][6] == 0
    assert ref.orient(len(v), f, None, "anchor")["counts"][5] == 1  # consistently wound but for the one seam that cannot be


def test_klein_bottle_is_closed_and_nonorientable_and_the_torus_is_not():
    v, f = ref.grid(8, 6, klein=True)
    out = ref.orient(len(v), f, None, "volume", v)
    assert out["counts"][:5] == [96, 1, 1, 96, 144] and out["counts"][5] == out["counts"][6] > 0 and np.array_equal(out["out_faces"], f.astype(np.int32))
    v, f = ref.grid(9, 7)
    out = ref.orient(len(v), f, None, "volume", v)
    assert out["counts"][:8] == [126, 1, 0, 0, 189, 0, 0, 0] or out["counts"][7] == 126  # consistent already: kept, or turned as one
    assert out["counts"][5:7] == [0, 0]


def test_books_link_nothing_and_nonfinite_vertices_are_counted():
    V, f = ref_mesh_manifold.book(7)
    out = ref.orient(V, f, None, "majority")
    assert out["counts"] == [7, 7, 0, 0, 0, 0, 0, 0, 0, 0] and out["face_piece"].tolist() == list(range(7))
    v, f = ref.latlong_sphere()
    w = v.copy()
    w[5], w[9, 1] = np.nan, np.inf
    touched = int(np.isin(f, [5, 9]).any(1).sum())
    out = ref.orient(len(w), f[:, [0, 2, 1]], None, "volume", w)
    assert out["counts"][9] == touched and out["counts"][8] == 1 and np.array_equal(out["out_faces"], f.astype(np.int32))
    w[0] = np.nan  # the anchor vertex: every difference is NaN, every term 0, S_p == 0 changes nothing
    out = ref.orient(len(w), f[:, [0, 2, 1]], None, "volume", w)
    assert out["counts"][9] == len(f) and out["counts"][7:9] == [0, 0] and out["S"] == {0: 0}
    flat = ref.orient(4, [[0, 1, 2], [0, 2, 3]], None, "volume", np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32))
    assert flat["S"] == {0: 0} and flat["counts"][5:10] == [0, 0, 0, 0, 0]
    empty = ref.orient(0, [[0, 1, 2], [-1, 5, 2 ** 31 - 1]], None, "volume", np.zeros((0, 3), np.float32))
    assert empty["counts"] == [0] * 10 and (empty["face_piece"] == -1).all() and not empty["face_flip"].any()


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(orient_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsw_last_error.restype = ctypes.c_char_p; "
            "l.tsw_workspace_bytes.restype = ctypes.c_size_t; print(l.tsw_workspace_bytes(100000, 200000) >= 92 * 200000, "
            "repr(l.tsw_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, orient_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(orient_path):
    out = subprocess.run(["nm", "-D", "--defined-only", orient_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES and len(NAMES) == 3
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", orient_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", orient_path], capture_output=True, text=True).stdout
    assert "libts_orient.so" in dynamic
    for other in ("libts2d.so", "libts_geom.so", "libts_bvh.so", "libts_ray.so", "libts_volume.so", "libts_color.so", "libts_simplify.so",
                  "libts_smooth.so", "libts_holes.so", "libts_manifold.so"):
        assert other not in dynamic


def test_header_defines_no_struct_and_states_the_contract():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsv|tsc|tsq|tss|tsh|tsf)_[a-z0-9_]+)\s*\(", text)  # a prefix of its own
    assert "struct" not in text
    full = open(HEADER).read()
    for word in ("TAKES PART", "EXACTLY TWICE", "EVEN", "ODD", "DOUBLED GRAPH", "2 f + 1", "min(r0, r1) >> 1", "NON-ORIENTABLE", "r0 & 1", "ANCHOR",
                 "MAJORITY", "VOLUME", "a tie keeps the anchor", "56 - bitlength(n_p) - 3 e_p", "llrint(ldexp(t, k_p))", "2^59", "frexp",
                 "-ffp-contract=off", "(a, c, b)", "bit for bit", "715827882", "Monotonic", "does not depend on the winding", "compare-exchange",
                 "ONE piece"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(ORIENT_SIGNATURES) and len(declared) == 3
    for name, arity in declared.items():
        assert len(ORIENT_SIGNATURES[name][1]) == arity, name
    assert declared["tsw_orient"] == 13
    abi = _abi_module()
    tables = [abi.SIGNATURES, abi.LAB_SIGNATURES, abi.GEOM_SIGNATURES, abi.BVH_SIGNATURES, abi.RAY_SIGNATURES, abi.VOLUME_SIGNATURES,
              abi.COLOR_SIGNATURES, abi.SIMPLIFY_SIGNATURES, abi.SMOOTH_SIGNATURES, abi.HOLES_SIGNATURES, abi.MANIFOLD_SIGNATURES,
              abi.ORIENT_SIGNATURES]
    for a in range(len(tables)):
        for b in range(a + 1, len(tables)):
            assert not set(tables[a]) & set(tables[b])  # no signature table overlaps another
    restype, argtypes = ORIENT_SIGNATURES["tsw_orient"]
    assert restype == ctypes.c_int and argtypes[11] == ctypes.c_size_t and argtypes[5] == ctypes.c_int32 and argtypes[:2] == [ctypes.c_int32] * 2
    assert all(a == ctypes.c_void_p for i, a in enumerate(argtypes) if i not in (0, 1, 5, 11))
    assert ORIENT_SIGNATURES["tsw_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32])


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_orient", ("build.py",))
    assert build.ORIENT_SOURCES == {"mesh_orient.hip": ["-ffp-contract=off"], "api_orient.hip": []} and build.ORIENT_SHARED == ["radix_sort"]
    assert build.orient_units() == ["mesh_orient", "api_orient"]
    cmd = build.orient_command("mesh_orient", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert "-ffp-contract=off" not in build.orient_command("api_orient", cc="hipcc")
    assert build.orient_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_orient", "api_orient", "radix_sort")]
    for others in (build.units(), build.geom_units(), build.bvh_units(), build.ray_units(), build.volume_units(), build.color_units(),
                   build.simplify_units(), build.smooth_units(), build.holes_units(), build.manifold_units()):
        assert not {"mesh_orient", "api_orient"} & set(others)  # its own library only
    assert build.ORIENT_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_orient.so")
    for header in ("ts_orient_launch.h", "ts_union_find.h", os.path.join("..", "..", "include", "ts_orient.h")):
        assert header in build.HEADERS
    with pytest.raises(ValueError):
        build.orient_command("mesh_manifold")


def test_built_objects_carry_the_flags_and_the_union_find_is_the_shared_one(orient_path):
    build = _load("ts2d_build_orient2", ("build.py",))
    for unit in ("mesh_orient", "api_orient"):
        stamp = open(os.path.join(build.OBJ_DIR, unit + ".o.cmd")).read()  # what the object on disk was compiled with
        assert stamp.endswith(" ".join(build.orient_command(unit, cc=stamp.splitlines()[1].split()[0])))
        assert ("-ffp-contract=off" in stamp) == (unit == "mesh_orient")
    link = open(build.ORIENT_LIB + ".cmd").read()
    assert "-soname,libts_orient.so" in link and "radix_sort.o" in link and "mesh_manifold" not in link and "mesh_weld" not in link
    text = open(os.path.join(build.CSRC, "mesh_orient.hip")).read()
    assert '#include "ts_union_find.h"' in text and "uf_union(" in text and "uf_find(" in text
    assert not re.search(r"\buf_(load|find|union)\s*\([^;{]*\)\s*\{", text.replace("\n", " "))  # used there, defined in the header alone
    assert "fma(" not in text and "atomicAdd((float" not in text and "atomicAdd((double" not in text  # integer atomics, no fused operation


def test_size_query_is_monotone_in_both_counts(lib):
    sizes = (0, 1, 2, 63, 682, 683, 1024, 1025, 4097, 100000, 416666, 416667, 833333, 833334, 2499999, 2500000, 2500001, 2600000, 5000000)
    for fixed in (0, 1000, 3000000):
        prev_v = prev_f = -1
        for n in sizes:
            by_v, by_f = lib.tsw_workspace_bytes(n, fixed), lib.tsw_workspace_bytes(fixed, n)
            assert by_v >= prev_v and by_f >= prev_f, (n, fixed)
            assert by_f >= 92 * n  # two keys, two values and the other end per half-edge, two parents and 24 bytes of sums per face
            prev_v, prev_f = by_v, by_f
    assert lib.tsw_workspace_bytes(-5, -5) == lib.tsw_workspace_bytes(0, 0)
    assert lib.tsw_workspace_bytes(10, 2 ** 31 - 1) == lib.tsw_workspace_bytes(10, MAX_FACES)


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    big = 1 << 40

    def refused(rc, word, code=INVALID):
        assert rc == code, rc
        text = lib.tsw_last_error()
        assert text and word.encode() in text, text

    def orient(V=10, F=20, vertices=P, faces=P, keep=None, mode=1, face_piece=P, face_flip=P, out_faces=P, counts=P, ws=P, ws_bytes=big):
        return lib.tsw_orient(V, F, vertices, faces, keep, mode, face_piece, face_flip, out_faces, counts, ws, ws_bytes, None)

    for bad in (-1, -(2 ** 31)):
        refused(orient(V=bad), ">= 0")
        refused(orient(F=bad), ">= 0")
    refused(orient(F=MAX_FACES + 1), "exceeds", CAPACITY)
    refused(orient(F=2 ** 31 - 1), "exceeds", CAPACITY)
    for bad in (3, -1, 2 ** 31 - 1, -(2 ** 31)):
        refused(orient(mode=bad), "mode")
    refused(orient(mode=2, vertices=None), "vertices is null")
    for name in ("faces", "face_piece", "face_flip", "out_faces", "counts"):
        refused(orient(**{name: None}), "null")
    refused(orient(ws=None), "workspace is null")
    need = lib.tsw_workspace_bytes(1000, 2000)
    refused(orient(V=1000, F=2000, ws_bytes=need - 1), "workspace too small")
    assert str(need).encode() in lib.tsw_last_error()
    refused(orient(V=1000, F=2000, ws_bytes=0), "workspace too small")
    # what the checks accept, for the record: keep may be null, vertices may be null in modes 0 and 1, and nothing but counts is needed with
    # F == 0 (those calls would reach the device, so they are made in tests/test_mesh_orient_gpu.py)


def test_missing_library_is_an_import_error_and_the_package_still_imports(tmp_path, orient_path):
    """Without libts_orient.so, diff_recon_hip.mesh_orient raises and names the build command; everything else still imports."""
    src = os.path.dirname(orient_path)
    pkg = tmp_path / "diff_recon_hip"
    pkg.mkdir()
    for name in os.listdir(src):
        if name.endswith(".py") or (name.endswith(".so") and name != "libts_orient.so"):
            shutil.copy(os.path.join(src, name), pkg / name)
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([str(tmp_path), os.path.join(ROOT, "triangle-splatting_amd")])}
    code = ("import diff_recon_hip, sys\n"
            "assert str(diff_recon_hip.__file__).startswith(sys.argv[1]), diff_recon_hip.__file__\n"
            "print('others', callable(diff_recon_hip.weld_mesh), callable(diff_recon_hip.split_nonmanifold), callable(diff_recon_hip.fill_holes))\n"
            "try:\n    diff_recon_hip.orient_faces\nexcept ImportError as e:\n    print('lazy', e)\n"
            "import diff_recon_hip.mesh_orient\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, env=env)
    assert "others True True True" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert "lazy" in r.stdout and "libts_orient.so" in r.stdout
    assert r.returncode != 0 and "ImportError" in r.stderr
    assert "libts_orient.so" in r.stderr and "no CPU fallback" in r.stderr and "triangle-splatting_amd/build.py" in r.stderr


def test_package_re_exports_the_feature_lazily_and_keeps_the_pinned_parameter_lists(orient_path):
    import diff_recon_hip
    from diff_recon_hip import mesh_holes, mesh_manifold, mesh_orient, mesh_smooth
    names = ("OrientedMesh", "orient_faces", "orient_fused")
    assert diff_recon_hip._ORIENT_NAMES == names
    for name in names:
        assert getattr(diff_recon_hip, name) is getattr(mesh_orient, name)
    assert diff_recon_hip.mesh_orient is mesh_orient
    r = subprocess.run([sys.executable, "-c", "import sys, diff_recon_hip; print('diff_recon_hip.mesh_orient' in sys.modules); "
                        "diff_recon_hip.orient_faces; print('diff_recon_hip.mesh_orient' in sys.modules)"], capture_output=True, text=True,
                       env={**os.environ, "PYTHONPATH": os.path.join(ROOT, "triangle-splatting_amd")})
    assert r.stdout.split() == ["False", "True"], (r.stdout, r.stderr[-2000:])  # loaded on first use
    params = lambda fn: list(inspect.signature(fn).parameters)
    assert params(mesh_orient.orient_faces) == ["vertices", "faces", "keep", "outward"]
    assert params(mesh_orient.orient_fused) == ["mesh", "outward"]
    for fn in (mesh_orient.orient_faces, mesh_orient.orient_fused):
        assert inspect.signature(fn).parameters["outward"].default == "majority"
    assert mesh_orient.OrientedMesh._fields == ("faces", "face_flip", "face_piece", "stats")
    assert mesh_orient.COUNT_NAMES == ref.COUNT_NAMES and len(ref.COUNT_NAMES) == 10 and mesh_orient.OUTWARD == ref.MODES
    # the neighbours keep their parameter lists
    assert diff_recon_hip._MANIFOLD_NAMES == ("VertexFans", "ManifoldMesh", "vertex_fans", "split_nonmanifold", "manifold_fused")
    assert params(mesh_manifold.vertex_fans) == ["num_vertices", "faces", "keep"]
    assert params(mesh_manifold.split_nonmanifold) == ["vertices", "faces", "vertex_attributes", "attribute_valid", "keep", "fans"]
    assert params(mesh_manifold.manifold_fused) == ["mesh"]
    assert params(mesh_holes.fill_holes) == ["vertices", "faces", "max_loop_edges", "vertex_attributes", "attribute_valid", "keep", "loops"]
    assert params(mesh_holes.fill_fused) == ["mesh", "max_loop_edges"]
    assert params(mesh_smooth.vertex_normals)[:2] == ["vertices", "faces"]
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_orient.orient_faces(torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="outward"):
        mesh_orient.orient_faces(torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32), outward="inward")
