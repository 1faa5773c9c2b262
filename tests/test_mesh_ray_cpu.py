"""CPU tests of the ray-casting feature (no GPU): the numpy reference keeps the promises of include/ts_ray.h (watertight, exact on known
answers, the pruned walk equal to brute force), libts_ray.so is a library of its own with exactly the C ABI of the header, and every argument
check answers before any HIP call."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_distance as refd
import ref_mesh_ray as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_ray.h")
INVALID = 1  # TS2D_ERR_INVALID
NAMES = ["tsr_cast", "tsr_cast_workspace_bytes", "tsr_last_error"]


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_ray", ("diff_triangle_rasterization_2D", "_abi.py"))


RAY_SIGNATURES = _abi_module().RAY_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def ray_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_ray.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_ray.so"
    return path


@pytest.fixture(scope="module")
def lib(ray_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_ray(ctypes.CDLL(ray_path))


def _header_prototypes():
    """name -> number of parameters of every tsr_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


def _cube():
    """The cube [-1, 1]^3: integer coordinates, twelve outward counter-clockwise faces."""
    v = np.array(list(itertools.product((-1, 1), repeat=3)), np.float32)  # index = 4 x + 2 y + z over {0, 1}
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


# ---- the reference holds its own promises ------------------------------------------------------------------------------------------------
def test_cube_all_26_rays_from_the_centre_hit_at_exactly_one():
    v, f = _cube()
    tri = v[f].astype(np.float64)
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.einsum("ij,ij->i", normal, tri.mean(axis=1)) > 0).all()  # the faces look outwards
    d = np.array([p for p in itertools.product((-1, 0, 1), repeat=3) if any(p)], np.float32)
    assert len(d) == 26
    face, t, bary, side = ref.cast(np.zeros_like(d), d, v, f)
    assert (face >= 0).all() and (t == 1.0).all() and (side == -1).all()  # from inside: every hit is on a back
    assert np.allclose(bary.sum(axis=1), 1.0, atol=2 ** -22) and (bary >= 0).all()
    hit_point = np.einsum("ij,ijk->ik", bary.astype(np.float64), tri[face])
    assert np.array_equal(hit_point, d.astype(np.float64))
    # corners and edge midpoints lie on several faces: the smallest index of those that contain the point wins
    for i in range(26):
        on = [k for k in range(12) if ref.cast(np.zeros((1, 3)), d[i:i + 1], v, f[k:k + 1])[0][0] == 0]
        assert face[i] == min(on) and len(on) >= (1 if np.abs(d[i]).sum() == 1 else 2)


def test_every_ray_from_inside_a_closed_mesh_hits():
    v, f = ref.closed_mesh(3, seed=1)
    assert len(f) == 512 and len(v) == 258
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts == 2).all()  # closed: every edge has two faces
    o, d = ref.rays_from_inside(v, f, 1500, seed=2)
    tri = v[f]
    every_vertex = v - o[:len(v)]
    every_edge = (0.5 * tri[:, 0] + 0.5 * tri[:, 1]).astype(np.float32) - o[:512]
    o = np.concatenate([o, o[:len(v)], o[:512]])
    d = np.concatenate([d, every_vertex, every_edge])
    face, t, bary, side = ref.cast(o, d, v, f)
    assert (face >= 0).all(), np.nonzero(face < 0)[0][:10]
    assert np.isfinite(t).all() and (t > 0).all() and (side == -1).all()
    face_c, t_c, _, _ = ref.cast(o, d, v, f, cull_back=True)  # all backs: nothing is left
    assert (face_c == -1).all() and np.isposinf(t_c).all()
    face_r, t_r, _, side_r = ref.cast(o, d, v, f[:, ::-1], cull_back=True)  # every face reversed: all fronts, the same hits (a and c change roles:
    assert (face_r >= 0).all() and (side_r == 1).all() and np.allclose(t_r, t, rtol=1e-12, atol=0)  # the sums associate the other way round)


def test_side_is_front_exactly_where_the_ray_runs_against_the_normal():
    rng = np.random.default_rng(3)
    seen = set()
    for axis in range(3):
        for sign in (-1.0, 1.0):
            for winding in (0, 1):
                a, b = (axis + 1) % 3, (axis + 2) % 3
                tri = np.zeros((3, 3), np.float32)
                tri[:, axis] = 2.0 * sign + rng.uniform(-0.2, 0.2, 3)
                tri[0, [a, b]], tri[1, [a, b]], tri[2, [a, b]] = (-1, -1), (1, -1), (0, 1.5)
                order = [0, 1, 2] if winding == 0 else [0, 2, 1]
                f = np.array([order], np.int32)
                d = np.zeros((1, 3), np.float32)
                d[0, axis] = sign
                d[0, [a, b]] = rng.uniform(-0.1, 0.1, 2)
                face, t, _, side = ref.cast(np.zeros((1, 3), np.float32), d, tri, f)
                p = tri[order].astype(np.float64)
                n_dot_d = float(np.cross(p[1] - p[0], p[2] - p[0]) @ d[0].astype(np.float64))
                assert face[0] == 0 and t[0] > 0 and n_dot_d != 0
                assert side[0] == (1 if n_dot_d < 0 else -1), (axis, sign, winding)
                culled = ref.cast(np.zeros((1, 3), np.float32), d, tri, f, cull_back=True)[0][0]
                assert culled == (0 if side[0] == 1 else -1)
                seen.add((axis, sign, side[0]))
    assert len(seen) == 12  # both sides on each of the six dominant axes


def test_cull_back_drops_exactly_the_back_hits_and_finds_the_next_front_face():
    v, f = refd.heavy_tailed_soup(300, seed=4)
    o, d = ref.mixed_rays(400, v, f, seed=5)
    face, t, _, side = ref.cast(o, d, v, f)
    face_c, t_c, _, side_c = ref.cast(o, d, v, f, cull_back=True)
    front = side == 1
    assert front.sum() > 20 and (side == -1).sum() > 20
    assert np.array_equal(face_c[front], face[front]) and np.array_equal(t_c[front], t[front])
    assert (side_c[face_c >= 0] == 1).all()
    behind = (side == -1) & (face_c >= 0)
    assert behind.sum() > 5 and (t_c[behind] >= t[behind]).all()  # the next front face behind a culled back
    # ray by ray against the faces that show this ray their front, alone and without culling
    tri = v[f].astype(np.float64)
    for i in np.nonzero(behind)[0][:20]:
        det = ref.evaluate(o[i:i + 1].astype(np.float64), d[i:i + 1].astype(np.float64), tri, 0.0, np.array([np.inf]), False)[5]
        alone = ref.cast(o[i:i + 1], d[i:i + 1], v, f, keep=(det[0] > 0).astype(np.uint8))
        assert alone[0][0] == face_c[i] and alone[1][0] == t_c[i] and alone[3][0] == 1


def test_pruned_walk_over_groups_equals_brute_force_bit_for_bit():
    v, f = refd.heavy_tailed_soup(96, seed=6)
    rng = np.random.default_rng(7)
    f = np.concatenate([f, f[rng.integers(0, 96, 64)]])[rng.permutation(160)]  # repeated faces: ties that the smallest index must win
    groups = [g for g in rng.permutation(160).reshape(20, 8)]
    o, d = ref.mixed_rays(150, v, f, seed=8)
    good = ~ref.bad_rays(o, d)
    o, d = o[good], d[good]
    want = ref.cast(o, d, v, f)
    assert (want[0] >= 0).sum() > 40
    total = 0
    for order in (None, [rng.permutation(20) for _ in range(len(o))]):
        got, entered = ref.pruned_cast(o, d, v, f, groups, order=order)
        total += entered
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)) and np.array_equal(got[3], want[3])
    print("groups entered:", total, "of", 2 * 20 * len(o))
    assert total < 2 * 20 * len(o)  # the walk did skip
    got, _ = ref.pruned_cast(o, d, v, f, groups, tmin=0.25, tmax=2.0, cull_back=True)
    want = ref.cast(o, d, v, f, tmin=0.25, tmax=2.0, cull_back=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))


# ---- known answers on two parallel unit squares -----------------------------------------------------------------------------------------------
def test_known_answers_two_parallel_squares():
    v, f = ref.two_squares(0.5)
    rng = np.random.default_rng(9)
    xy = (rng.integers(1, 255, (200, 2)) / 256).astype(np.float32)
    o = np.concatenate([xy, np.full((200, 1), -2.0, np.float32)], axis=1)
    d = np.tile(np.array([[0, 0, 1]], np.float32), (200, 1))
    face, t, bary, side = ref.cast(o, d, v, f)
    assert (t == 2.0).all() and np.isin(face, (0, 1)).all() and (side == -1).all()  # from below: the back of the z = 0 square, at its distance
    assert np.array_equal(np.einsum("ij,ijk->ik", bary.astype(np.float64), v[f[face]].astype(np.float64))[:, :2], xy.astype(np.float64))
    face, t, _, side = ref.cast(o, 2 * d, v, f)  # t counts in units of d
    assert (t == 1.0).all()
    face, t, _, _ = ref.cast(o, d, v, f, tmin=2.25)  # the near square is skipped
    assert (t == 2.5).all() and np.isin(face, (2, 3)).all()
    face, t, _, _ = ref.cast(o, d, v, f, tmin=2.0, tmax=2.0)  # both ends are closed
    assert (t == 2.0).all()
    face, t, _, _ = ref.cast(o, d, v, f, tmin=2.125, tmax=2.375)  # between the two: nothing
    assert (face == -1).all() and np.isposinf(t).all()
    face, t, _, _ = ref.cast(o, d, v, f, tmax=1.5)
    assert (face == -1).all()
    limit = np.where(np.arange(200) % 2 == 0, 1.999, 2.0).astype(np.float32)  # a per-ray limit below the plane distance: a miss
    face, t, _, _ = ref.cast(o, d, v, f, t_limit=limit)
    assert (face[::2] == -1).all() and np.isposinf(t[::2]).all() and (t[1::2] == 2.0).all()
    face, t, _, side = ref.cast(o + np.array([0, 0, 4], np.float32), -d, v, f)  # from above: the front of the z = 0.5 square
    assert (t == 1.5).all() and np.isin(face, (2, 3)).all() and (side == 1).all()
    # the shared diagonal and the corners: both faces count, the smaller index wins
    od = np.array([[0.5, 0.5, -1], [0, 0, -1], [1, 1, -1], [0.25, 0.25, 3]], np.float32)
    dd = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, -1]], np.float32)
    face, t, _, _ = ref.cast(od, dd, v, f)
    assert face.tolist() == [0, 0, 0, 2] and t.tolist() == [1.0, 1.0, 1.0, 2.5]
    # bad rays, and rays that miss
    ob = np.array([[0.5, 0.5, -1]] * 6 + [[np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    db = np.array([[0, 0, 0], [np.nan, 0, 1], [0, -np.inf, 1], [0, 0, 1], [1, 0, 0], [0, 0, -1], [0, 0, 1], [0, 0, 1]], np.float32)
    lim = np.array([1, 1, 1, np.nan, 9, 9, 9, 9], np.float32)
    face, t, bary, side = ref.cast(ob, db, v, f, t_limit=lim)
    assert (face == -1).all() and (side == 0).all() and np.isnan(bary).all()
    assert np.isnan(t[[0, 1, 2, 3, 6, 7]]).all() and np.isposinf(t[[4, 5]]).all()
    face, t, _, _ = ref.cast(ob, db, v, np.zeros((0, 3), np.int32))  # no face at all
    assert (face == -1).all() and np.isnan(t[[0, 1, 2, 6, 7]]).all() and np.isposinf(t[[3, 4, 5]]).all()
    assert ref.visibility(np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.0], [2, 2, 0.5]], np.float32), np.array([[0.5, 0.5, -3], [0.5, 0.5, 3]], np.float32),
                          v, f).tolist() == [1, 1, 2]


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(ray_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsr_last_error.restype = ctypes.c_char_p; "
            "l.tsr_cast_workspace_bytes.restype = ctypes.c_size_t; print(l.tsr_cast_workspace_bytes(1000) >= 32000, repr(l.tsr_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, ray_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(ray_path):
    out = subprocess.run(["nm", "-D", "--defined-only", ray_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", ray_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", ray_path], capture_output=True, text=True).stdout
    assert "libts_ray.so" in dynamic
    for other in ("libts2d.so", "libts_geom.so", "libts_bvh.so"):
        assert other not in dynamic


def test_header_text_stays_out_of_the_other_libraries_lists():
    """tests/test_cabi_cpu.py strips only block comments before it collects the names of libts2d.so's entry points from every header."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb)_[a-z0-9_]+)\s*\(", text)
    full = open(HEADER).read()
    for word in ("Woop", "2^-40", "monotone", "SMALLEST FACE INDEX", "-ffp-contract=off", "ts_bvh.h"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(RAY_SIGNATURES)
    for name, arity in declared.items():
        assert len(RAY_SIGNATURES[name][1]) == arity, name
    assert declared["tsr_cast"] == 18
    abi = _abi_module()
    for table in (abi.SIGNATURES, abi.LAB_SIGNATURES, abi.GEOM_SIGNATURES, abi.BVH_SIGNATURES):
        assert not set(RAY_SIGNATURES) & set(table)
    assert RAY_SIGNATURES["tsr_cast"][1][4:6] == [ctypes.c_double, ctypes.c_double]


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_ray", ("build.py",))
    assert list(build.RAY_SOURCES) == ["mesh_ray.hip", "api_ray.hip"] and build.RAY_SHARED == ["radix_sort"]
    assert "-ffp-contract=off" in build.RAY_SOURCES["mesh_ray.hip"]
    assert build.ray_units() == ["mesh_ray", "api_ray"]
    cmd = build.ray_command("mesh_ray", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert build.ray_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_ray", "api_ray", "radix_sort")]
    for others in (build.units(), build.geom_units(), build.bvh_units()):
        assert not {"mesh_ray", "api_ray"} & set(others)  # its own library only
    assert build.RAY_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_ray.so")
    for header in ("ts_ray_launch.h", "ts_bvh_layout.h", os.path.join("..", "..", "include", "ts_ray.h")):
        assert header in build.HEADERS
    with pytest.raises(ValueError):
        build.ray_command("mesh_bvh")


def test_built_objects_carry_the_flags(ray_path):
    build = _load("ts2d_build_ray2", ("build.py",))
    assert "-ffp-contract=off" in open(os.path.join(build.OBJ_DIR, "mesh_ray.o.cmd")).read()  # what the object on disk was compiled with
    assert "-soname,libts_ray.so" in open(build.RAY_LIB + ".cmd").read()
    # the layout is one text: both units that read the index include it, neither restates it
    csrc = os.path.join(build.CSRC)
    for unit in ("mesh_bvh.hip", "mesh_ray.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "ts_bvh_layout.h"' in text and "struct Leaf" not in text and "struct BvhView" not in text


def test_size_query_is_monotone_and_index_size_agrees_with_the_bvh_library(lib, ray_path):
    sizes = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 65_537, 640_000, 2_499_999, 2_500_000, 2_500_001, 2_600_000, 5_000_000, 100_000_000,
             2 ** 31 - 1025]
    prev = -1
    for n in sizes:
        got = lib.tsr_cast_workspace_bytes(n)
        assert got >= 32 * n and got >= prev, (n, got, prev)  # the sorted origins and two key / value pairs
        prev = got
    from diff_triangle_rasterization_2D import _abi
    bvh = _abi.bind_bvh(ctypes.CDLL(os.path.join(os.path.dirname(ray_path), "libts_bvh.so")))
    P, big = 0x1000, 1 << 40
    for F in (1, 8, 9, 64, 65, 513, 4097, 1_000_000):  # one byte short of the other library's size query is refused, the size itself is not
        need = bvh.tsb_bvh_bytes(F)
        rc = lib.tsr_cast(1, P, P, None, 0.0, 1.0, 0, F, P, need - 1, P, P, None, None, None, P, big, None)
        assert rc == INVALID and b"bvh too small" in lib.tsr_last_error() and str(need).encode() in lib.tsr_last_error()
        assert lib.tsr_cast(1, P, P, None, 0.0, 1.0, 0, F, P, need, P, P, None, None, None, P, 0, None) == INVALID
        assert b"workspace too small" in lib.tsr_last_error()


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    big = 1 << 40
    nan, inf = float("nan"), float("inf")

    def refused(rc, word):
        assert rc == INVALID, rc
        text = lib.tsr_last_error()
        assert text and word.encode() in text, text

    def cast(Q=1, origins=P, directions=P, t_limit=None, tmin=0.0, tmax=inf, cull_back=0, F=1, bvh=P, bvh_bytes=big, face=P, t=P, bary=P, side=P,
             ws=P, ws_bytes=big):
        return lib.tsr_cast(Q, origins, directions, t_limit, tmin, tmax, cull_back, F, bvh, bvh_bytes, face, t, bary, side, None, ws, ws_bytes, None)

    refused(cast(Q=-1), "Q")
    refused(cast(F=-1), "F")
    refused(cast(Q=2 ** 31 - 1), "at most")
    refused(cast(F=2 ** 31 - 1), "at most")
    refused(cast(origins=None), "null")
    refused(cast(directions=None), "null")
    refused(cast(face=None), "null")
    refused(cast(t=None), "null")
    refused(cast(bvh=None), "null")
    refused(cast(ws=None), "null")
    refused(cast(F=1000, bvh_bytes=1000), "bvh too small")
    refused(cast(Q=1000, ws_bytes=lib.tsr_cast_workspace_bytes(1000) - 1), "workspace too small")
    refused(cast(tmin=nan), "NaN")
    refused(cast(tmax=nan), "NaN")
    refused(cast(tmin=2.0, tmax=1.0), "exceeds")
    refused(cast(tmin=inf, tmax=-inf), "exceeds")
    refused(cast(cull_back=2), "cull_back")
    refused(cast(cull_back=-1), "cull_back")
    refused(cast(Q=0, tmin=nan), "NaN")  # the values are checked whatever the counts
    assert cast(Q=0, origins=None, directions=None, bvh=None, bvh_bytes=0, face=None, t=None, bary=None, side=None, ws=None, ws_bytes=0) == 0  # the no-op
    assert cast(Q=0, tmin=1.0, tmax=1.0, cull_back=1) == 0


def test_missing_library_is_an_import_error_and_closest_still_imports(tmp_path, ray_path):
    """Without libts_ray.so, diff_recon_hip.mesh_ray raises and names the build command; the package, MeshBVH.closest included, still imports."""
    src = os.path.dirname(ray_path)
    pkg = tmp_path / "diff_recon_hip"
    pkg.mkdir()
    for name in os.listdir(src):
        if name.endswith(".py") or name in ("libts_geom.so", "libts_bvh.so"):
            shutil.copy(os.path.join(src, name), pkg / name)
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([str(tmp_path), os.path.join(ROOT, "triangle-splatting_amd")])}
    code = ("import diff_recon_hip, sys\n"
            "assert str(diff_recon_hip.__file__).startswith(sys.argv[1]), diff_recon_hip.__file__\n"
            "print('closest', callable(diff_recon_hip.MeshBVH.closest), callable(diff_recon_hip.MeshBVH.ray_cast))\n"
            "try:\n    diff_recon_hip.ray_cast\nexcept ImportError as e:\n    print('lazy', e)\n"
            "import diff_recon_hip.mesh_ray\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, env=env)
    assert "closest True True" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert "lazy" in r.stdout and "libts_ray.so" in r.stdout
    assert r.returncode != 0 and "ImportError" in r.stderr
    assert "libts_ray.so" in r.stderr and "no CPU fallback" in r.stderr and "triangle-splatting_amd/build.py" in r.stderr


def test_package_re_exports_the_feature(ray_path):
    import diff_recon_hip
    from diff_recon_hip import mesh_ray
    for name in ("RayHits", "ray_cast", "camera_rays", "point_visibility"):
        assert getattr(diff_recon_hip, name) is getattr(mesh_ray, name)
    assert diff_recon_hip.RayHits._fields == ("face", "t", "bary", "side")
    import inspect
    assert list(inspect.signature(diff_recon_hip.ray_cast).parameters) == ["bvh", "origins", "directions", "tmin", "tmax", "t_limit", "cull_back",
                                                                            "leaf_visits"]
    assert inspect.signature(diff_recon_hip.mesh_surface_distance).parameters["visible_from"].default is None
    assert inspect.signature(diff_recon_hip.point_visibility).parameters["rel_eps"].default == 1e-5


def test_example_refuses_eval_visible_without_eval_surface():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), "--eval-visible"], capture_output=True, text=True)
    assert r.returncode == 2 and "--eval-visible restricts the scores of --eval-surface" in r.stderr
