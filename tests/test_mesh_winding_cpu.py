"""CPU tests of the generalised winding number (no GPU): the numpy reference against itself (the tree form with beta = inf is brute force
bit for bit on any tree, the cube's known values, the overflow bound of include/ts_winding.h), libts_winding.so is a library of its own
with exactly the C ABI of the header, its size queries are monotonic, and every argument check answers before any HIP call."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_inside as refi
import ref_mesh_winding as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_winding.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tsn_last_error", "tsn_leaf_faces_bytes", "tsn_moments", "tsn_moments_bytes", "tsn_sign_distance", "tsn_winding",
         "tsn_winding_workspace_bytes"]
TURN, HALF = 1 << 38, 1 << 37


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_winding", ("diff_triangle_rasterization_2D", "_abi.py"))


WINDING_SIGNATURES = _abi_module().WINDING_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def winding_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_winding.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_winding.so"
    return path


@pytest.fixture(scope="module")
def lib(winding_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_winding(ctypes.CDLL(winding_path))


def _header_prototypes():
    """name -> number of parameters of every tsn_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


# ---- the reference against itself ------------------------------------------------------------------------------------------------------
def test_cube_values_inside_outside_reversed_doubled_and_on_the_surface():
    v, f = refi.cube()
    p = np.array([[0, 0, 0], [0.3, -0.2, 0.9], [3, 0.1, 0.2], [1, 1, 1], [1, 0, 0.3], [0, 0, 1], [np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    wq = ref.winding_exact(p, v, f)
    assert (np.abs(wq[:2] - TURN) <= 12).all() and abs(wq[2]) <= 12        # +1 inside the outward cube, 0 outside: within F units
    assert abs(wq[3] - TURN // 8) <= 12                                    # a corner sees an octant
    assert abs(wq[4] - HALF) <= 12 and abs(wq[5] - HALF) <= 12             # on an edge of a face, in a face: half
    assert (wq[6:] == ref.BAD).all() and np.isnan(ref.to_turns(wq)[6:]).all() and ref.to_turns(wq)[0] == wq[0] / 2.0 ** 38
    assert (np.abs(ref.winding_exact(p[:3], *refi.cube(reverse=True)) + wq[:3]) <= 12).all()   # inside out: -1
    twice = ref.winding_exact(p[:3], *refi.join((v, f), (v, f)))
    assert np.array_equal(twice, 2 * wq[:3])                               # integer sums: the cube doubled is exactly twice the cube
    assert (ref.winding_exact(p[:6], v, np.zeros((0, 3), np.int32)) == 0).all()
    assert np.array_equal(ref.winding_exact(p[:3], v, f, keep=np.arange(12) < 0), np.zeros(3, np.int64))
    # a face in whose plane the query lies counts nothing, whichever way round
    tri_v, tri_f = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32)
    assert ref.winding_exact(np.array([[0.25, 0.25, 0], [2, 2, 0], [0, 0, 0], [0.5, 0, 0]], np.float32), tri_v, tri_f).tolist() == [0, 0, 0, 0]
    above = ref.winding_exact(np.array([[0.25, 0.25, 1e-3], [0.25, 0.25, -1e-3]], np.float32), tri_v, tri_f)
    assert above[0] < -HALF + (1 << 32) and above[1] == -above[0]         # just above the counter-clockwise face: its back, nearly -1/2


def test_the_open_cube_is_decided_by_a_half_on_the_24_cubed_grid():
    """The cube without its two z = -1 faces on the issue's grid: w >= 1/2 exactly on the 14^3 samples strictly inside, and every sample on the
    border of the grid is outside -- what a ray count cannot say, since every ray that leaves through the hole counts nothing."""
    v, f = refi.cube()
    keep = ~(v[f][:, :, 2] == -1).all(axis=1)
    assert keep.sum() == 10
    p = refi.grid_points((-1.6, -1.6, -1.6), 3.2 / 23, (24, 24, 24))
    wq = ref.winding_exact(p, v, f[keep])
    strictly_in = (np.abs(p) < 1).all(axis=1)
    assert strictly_in.sum() == 14 ** 3 and np.array_equal(wq >= HALF, strictly_in)
    margin = np.abs(ref.to_turns(wq) - 0.5).min()
    print(f"open cube on 24^3: the sample nearest to the threshold is {margin:.4f} turns away from it")
    assert margin > 1e-3  # no sample balances on the threshold: the far field may move w by less than that and change nothing


def test_tree_form_with_infinite_beta_is_brute_force_on_any_tree_and_finite_beta_is_near():
    rng = np.random.default_rng(5)
    for n, drop in ((2, False), (3, True)):
        v, f = ref.cube_grid(n, drop)
        f = np.concatenate([f, [[0, 1, 10 ** 6], [0, 0, 0]]]).astype(np.int32)  # a bad index (ineligible) and a zero-area face (eligible, counts 0)
        p = rng.uniform(-1.5, 1.5, (300, 3)).astype(np.float32)
        p[7] = np.nan
        exact = ref.winding_exact(p, v, f)
        for table in (ref.stand_in_leaf_faces(v, f), rng.permutation(ref.stand_in_leaf_faces(v, f))):  # -1 slots anywhere: still a tree
            assert sorted(table[table >= 0].tolist()) == list(range(len(f) - 2)) + [len(f) - 1]
            wq, terms = ref.winding_tree(p, v, f, table, np.inf)
            assert np.array_equal(wq, exact) and wq[7] == ref.BAD and terms[7].tolist() == [-1, -1]
            good = np.arange(300) != 7
            assert (terms[good, 0] == len(f) - 1).all() and (terms[good, 1] == 0).all()  # every eligible face, no node
        wide = p * np.float32(3)  # far enough from the small nodes of the ordered table for some to be accepted
        far, terms = ref.winding_tree(wide, v, f, ref.stand_in_leaf_faces(v, f), 2.0)
        assert (terms[good, 1] > 0).any() and (terms[good, 0] < len(f) - 1).any()
        near = np.abs(ref.to_turns(far[good]) - ref.to_turns(ref.winding_exact(wide, v, f)[good])).max()
        assert 0 < near < 0.1


def test_moments_of_one_leaf_and_of_its_parent():
    v, f = refi.cube()
    table = np.concatenate([np.arange(12), [-1] * 4]).astype(np.int32)  # two leaves: 8 + 4 faces, and the root
    m = ref.moments(v, f, table)
    assert m.shape == (3, 8)
    assert np.allclose(m[2, :3], 0, atol=1e-15) and m[2, 7] == 24.0 and np.allclose(m[2, 3:6], 0, atol=1e-15)  # closed: no dipole; area 24
    assert m[2, 6] == 3.0 and m[0, 7] + m[1, 7] == 24.0                  # the root's radius reaches the corners
    assert np.array_equal(m[2, :3], m[0, :3] + m[1, :3])
    empty = ref.moments(v, f, np.full(8, -1, np.int32))
    assert empty.shape == (1, 8) and empty[0, 6] == np.inf and (empty[0, [0, 1, 2, 3, 4, 5, 7]] == 0).all()
    assert ref.moments(v, f, np.zeros(0, np.int32)).shape == (0, 8)


def test_overflow_bound_of_the_header():
    """A face term is at most 2^37 units; an accepted node of m faces, each within sqrt(R2) of p, is below m / (2 pi beta^2) turns, with
    beta >= 1 below 2^36 m units: F <= 2^24 - 1 keeps the sum below 2^61."""
    assert ref.MAX_FACES == 2 ** 24 - 1 and ref.MAX_FACES * 2 ** 37 < 2 ** 61 < 2 ** 63
    assert 2.0 ** 38 / (2 * np.pi) < 2.0 ** 36
    # the largest face term: seen from just above its middle a face fills half the sky
    tri_v, tri_f = np.array([[-1e6, -1e6, 0], [1e6, -1e6, 0], [0, 2e6, 0]], np.float32), np.array([[0, 1, 2]], np.int32)
    big = ref.winding_exact(np.array([[0, 0, -1e-6]], np.float32), tri_v, tri_f)
    assert HALF - 4 <= big[0] <= HALF
    # an accepted node against the bound: random sheets, every accepted node's own term
    rng = np.random.default_rng(2)
    v, f = ref.cube_grid(3, True)
    t = ref.Tree(v, f, ref.stand_in_leaf_faces(v, f))
    q = rng.uniform(-4, 4, (2000, 3))
    for at in range(t.total):
        m = t.moments[at]
        level = max(l for l in range(len(t.count)) if t.offset[l] <= at)
        faces = min(8 ** (level + 1), len(f))
        r = m[3:6] - q
        d2 = ref.dot(r, r)
        ok = d2 > 1.0 * m[6]
        term = np.abs(ref.dot(m[0:3], r[ok]) / (d2[ok] * np.sqrt(d2[ok])) / (4 * np.pi))
        assert (term < faces / (2 * np.pi)).all()


def test_cube_grid_is_closed_and_outward_and_loses_98_faces_with_its_bottom():
    v, f = ref.cube_grid(7)
    assert len(f) == 588 and len(ref.cube_grid(7, True)[1]) == 490
    tri = v[f].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.einsum("ij,ij->i", n, tri.mean(axis=1)) > 0).all() and abs(0.5 * np.linalg.norm(n, axis=1).sum() - 24.0) < 1e-9
    assert abs(np.einsum("ij,ij->i", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum() / 6 - 8.0) < 1e-9  # the signed volume
    ov, of = ref.cube_grid(7, True)
    assert not (ov[of][:, :, 2] == -1).all(axis=1).any()


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(winding_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsn_last_error.restype = ctypes.c_char_p; "
            "l.tsn_winding_workspace_bytes.restype = ctypes.c_size_t; print(l.tsn_winding_workspace_bytes(1000) >= 32000, repr(l.tsn_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, winding_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(winding_path):
    out = subprocess.run(["nm", "-D", "--defined-only", winding_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", winding_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", winding_path], capture_output=True, text=True).stdout
    assert "libts_winding.so" in dynamic
    for other in ("libts2d.so", "libts_geom.so", "libts_bvh.so", "libts_ray.so", "libts_inside.so"):
        assert other not in dynamic


def test_header_text_stays_out_of_the_other_libraries_lists():
    """tests/test_cabi_cpu.py strips only block comments before it collects the names of libts2d.so's entry points from every header."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsi|tsw)_[a-z0-9_]+)\s*\(", text)
    full = open(HEADER).read()
    for word in ("2^-38 turns", "INT64_MIN", "-ffp-contract=off", "ts_bvh.h", "0x400921FB54442D18", "round half to even", "2^24 - 1", "is finite",
                 "beta2 = beta*beta", "Purity"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(WINDING_SIGNATURES)
    for name, arity in declared.items():
        assert len(WINDING_SIGNATURES[name][1]) == arity, name
    assert declared["tsn_winding"] == 13 and declared["tsn_moments"] == 8 and declared["tsn_sign_distance"] == 7
    abi = _abi_module()
    for table in (abi.SIGNATURES, abi.LAB_SIGNATURES, abi.GEOM_SIGNATURES, abi.BVH_SIGNATURES, abi.RAY_SIGNATURES, abi.ATLAS_SIGNATURES,
                  abi.INSIDE_SIGNATURES, abi.ORIENT_SIGNATURES):
        assert not set(WINDING_SIGNATURES) & set(table)
    assert WINDING_SIGNATURES["tsn_winding"][1][2] is ctypes.c_double and WINDING_SIGNATURES["tsn_sign_distance"][1][3] is ctypes.c_int64


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_winding", ("build.py",))
    assert list(build.WINDING_SOURCES) == ["mesh_winding.hip", "api_winding.hip"] and build.WINDING_SHARED == ["radix_sort"]
    assert "-ffp-contract=off" in build.WINDING_SOURCES["mesh_winding.hip"]
    assert build.winding_units() == ["mesh_winding", "api_winding"]
    cmd = build.winding_command("mesh_winding", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert build.winding_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_winding", "api_winding", "radix_sort")]
    for others in (build.units(), build.geom_units(), build.bvh_units(), build.ray_units(), build.inside_units()):
        assert not {"mesh_winding", "api_winding"} & set(others)  # its own library only
    assert build.WINDING_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_winding.so")
    for header in ("ts_winding_launch.h", "ts_bvh_layout.h", "ts_knn_front.h", os.path.join("..", "..", "include", "ts_winding.h")):
        assert header in build.HEADERS
    with pytest.raises(ValueError):
        build.winding_command("mesh_inside")


def test_built_objects_carry_the_flags_and_the_layout_is_one_text(winding_path):
    build = _load("ts2d_build_winding2", ("build.py",))
    assert "-ffp-contract=off" in open(os.path.join(build.OBJ_DIR, "mesh_winding.o.cmd")).read()  # what the object on disk was compiled with
    assert "-soname,libts_winding.so" in open(build.WINDING_LIB + ".cmd").read()
    text = open(os.path.join(build.CSRC, "mesh_winding.hip")).read()
    assert '#include "ts_bvh_layout.h"' in text and "struct Leaf" not in text and "knn_prepare<true>" in text


def test_size_queries_are_monotone_and_follow_the_layout(lib, winding_path):
    sizes = [0, 1, 2, 7, 8, 9, 63, 64, 65, 512, 513, 1023, 1024, 1025, 4097, 65_537, 640_000, 2_499_999, 2_500_000, 2_500_001, 2_600_000, 5_000_000,
             2 ** 24 - 1, 100_000_000, 2 ** 31 - 1025]
    prev = (-1, -1, -1)
    for n in sizes:
        got = (lib.tsn_winding_workspace_bytes(n), lib.tsn_moments_bytes(n), lib.tsn_leaf_faces_bytes(n))
        assert got[0] >= 32 * n and all(g >= p for g, p in zip(got, prev)), (n, got, prev)
        leaves = (n + 7) // 8
        nodes, c = 0, leaves
        while c > 0:
            nodes += c
            if c == 1:
                break
            c = (c + 7) // 8
        assert got[1] == 64 * nodes and got[2] == 32 * leaves, n
        prev = got
    from diff_triangle_rasterization_2D import _abi
    here = os.path.dirname(winding_path)
    bvh = _abi.bind_bvh(ctypes.CDLL(os.path.join(here, "libts_bvh.so")))
    inside = _abi.bind_inside(ctypes.CDLL(os.path.join(here, "libts_inside.so")))
    assert [lib.tsn_winding_workspace_bytes(n) for n in sizes] == [inside.tsi_crossings_workspace_bytes(n) for n in sizes]  # the same front half
    P, big = 0x1000, 1 << 40
    for F in (1, 8, 9, 64, 65, 513, 4097, 1_000_000):  # one byte short of the other library's size query is refused, the size itself is not
        need = bvh.tsb_bvh_bytes(F)
        rc = lib.tsn_winding(1, P, 2.0, F, P, need - 1, P, big, P, None, P, big, None)
        assert rc == INVALID and b"bvh too small" in lib.tsn_last_error() and str(need).encode() in lib.tsn_last_error()
        assert lib.tsn_winding(1, P, 2.0, F, P, need, P, big, P, None, P, 0, None) == INVALID
        assert b"workspace too small" in lib.tsn_last_error()
        assert lib.tsn_moments(F, P, need - 1, P, big, None, 0, None) == INVALID and b"bvh too small" in lib.tsn_last_error()


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    big = 1 << 40
    nan, inf = float("nan"), float("inf")

    def refused(rc, word, code=INVALID):
        assert rc == code, rc
        text = lib.tsn_last_error()
        assert text and word.encode() in text, text

    def wind(Q=1, points=P, beta=2.0, F=1, bvh=P, bvh_bytes=big, moments=P, moments_bytes=big, wq=P, terms=None, ws=P, ws_bytes=big):
        return lib.tsn_winding(Q, points, beta, F, bvh, bvh_bytes, moments, moments_bytes, wq, terms, ws, ws_bytes, None)

    refused(wind(Q=-1), "Q")
    refused(wind(F=-1), "F")
    refused(wind(Q=2 ** 31 - 1), "at most")
    refused(wind(F=2 ** 31 - 1), "at most")
    refused(wind(F=2 ** 24), "must not wrap", CAPACITY)
    refused(wind(F=2 ** 31 - 1025), "must not wrap", CAPACITY)
    refused(wind(F=2 ** 24 - 1, bvh_bytes=1000), "bvh too small")  # the largest F that is taken
    refused(wind(beta=nan), "NaN")
    refused(wind(beta=0.999), "at least 1")
    refused(wind(beta=0.0), "at least 1")
    refused(wind(beta=-inf), "at least 1")
    refused(wind(Q=0, beta=nan), "NaN")  # the values are checked whatever the counts
    refused(wind(Q=0, F=2 ** 24), "must not wrap", CAPACITY)
    refused(wind(points=None), "null")
    refused(wind(wq=None), "null")
    refused(wind(bvh=None), "null")
    refused(wind(moments=None), "null")
    refused(wind(ws=None), "null")
    refused(wind(F=1000, bvh_bytes=1000), "bvh too small")
    refused(wind(F=1000, moments_bytes=lib.tsn_moments_bytes(1000) - 1), "moments too small")
    refused(wind(Q=1000, ws_bytes=lib.tsn_winding_workspace_bytes(1000) - 1), "workspace too small")
    assert wind(Q=0, points=None, bvh=None, bvh_bytes=0, moments=None, moments_bytes=0, wq=None, ws=None, ws_bytes=0) == 0  # the no-op
    assert wind(Q=0, beta=inf) == 0 and wind(Q=0, beta=1.0) == 0

    def mom(F=1, bvh=P, bvh_bytes=big, moments=P, moments_bytes=big, leaf_faces=None, leaf_faces_bytes=0):
        return lib.tsn_moments(F, bvh, bvh_bytes, moments, moments_bytes, leaf_faces, leaf_faces_bytes, None)

    refused(mom(F=-1), "F")
    refused(mom(F=2 ** 24), "must not wrap", CAPACITY)
    refused(mom(bvh=None), "null")
    refused(mom(moments=None), "null")
    refused(mom(F=100, bvh_bytes=100), "bvh too small")
    refused(mom(F=100, moments_bytes=lib.tsn_moments_bytes(100) - 1), "moments too small")
    refused(mom(F=100, leaf_faces=P, leaf_faces_bytes=lib.tsn_leaf_faces_bytes(100) - 1), "leaf_faces too small")
    assert mom(F=0, bvh=None, bvh_bytes=0, moments=None, moments_bytes=0) == 0  # the no-op

    def sd(Q=1, dist2=P, wq=P, threshold=HALF, out=P, decided=P):
        return lib.tsn_sign_distance(Q, dist2, wq, threshold, out, decided, None)

    refused(sd(Q=-1), "Q")
    refused(sd(Q=2 ** 31 - 1), "at most")
    for name in ("dist2", "wq", "out", "decided"):
        refused(sd(**{name: None}), "null")
    assert sd(Q=0, dist2=None, wq=None, out=None, decided=None) == 0
    assert sd(Q=0, threshold=-(1 << 63)) == 0


def test_package_re_exports_the_feature_and_the_defaults_stay(winding_path):
    import diff_recon_hip
    from diff_recon_hip import mesh_inside, mesh_winding
    for name in mesh_winding.__all__:
        assert getattr(diff_recon_hip, name) is getattr(mesh_winding, name)
    assert sorted(mesh_winding.__all__) == sorted(diff_recon_hip._WINDING_NAMES)
    assert callable(diff_recon_hip.MeshBVH.winding_number)
    sig = inspect.signature(diff_recon_hip.generalized_winding_number).parameters
    assert list(sig) == ["points", "mesh", "beta", "return_terms"] and sig["beta"].default == 2.0 and sig["return_terms"].default is False
    sig = inspect.signature(diff_recon_hip.contains_points_winding).parameters
    assert list(sig) == ["points", "mesh", "beta", "threshold"] and sig["threshold"].default == 0.5
    for fn in (diff_recon_hip.contains_points, diff_recon_hip.signed_distance, diff_recon_hip.mesh_volume_iou):  # today's path is the default
        sig = inspect.signature(fn).parameters
        assert sig["method"].default == "rays" and sig["beta"].default == 2.0
    assert mesh_winding.threshold_units(0.5) == HALF and mesh_winding.threshold_units(1.0) == TURN and mesh_winding.threshold_units(-0.25) == -(1 << 36)
    assert mesh_winding.UNITS_PER_TURN == TURN and mesh_winding.BAD_QUERY == ref.BAD
    for bad in (float("nan"), 0.5, -1.0):
        with pytest.raises(ValueError):
            mesh_winding._beta(bad)
    assert mesh_winding._beta(float("inf")) == float("inf") and mesh_winding._beta(1) == 1.0
    with pytest.raises(ValueError):
        mesh_winding.threshold_units(float("inf"))
    with pytest.raises(ValueError):
        mesh_inside._method("scanline")
    with pytest.raises(ValueError):
        mesh_inside._method("winding", "odd")   # the winding number knows one rule
    assert mesh_inside._method("winding") is True and mesh_inside._method("rays", "odd") is False


def test_example_takes_the_remesh_method():
    example = os.path.join(ROOT, "examples", "train_synthetic.py")
    r = subprocess.run([sys.executable, example, "--remesh", "32", "--remesh-method", "winding"], capture_output=True, text=True)
    assert r.returncode == 2 and "--remesh remeshes the mesh of --extract-mesh" in r.stderr
    r = subprocess.run([sys.executable, example, "--remesh-method", "scanline"], capture_output=True, text=True)
    assert r.returncode == 2 and "invalid choice" in r.stderr
