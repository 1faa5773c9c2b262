"""CPU tests of the inside test and the signed distance of a mesh (no GPU): the numpy reference gives the known answers of the half-crossing
rule (through an edge, along a face diagonal, grazing an edge, through a corner, nested and reversed cubes), libts_inside.so is a library of
its own with exactly the C ABI of include/ts_inside.h, and every argument check answers before any HIP call."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_inside as ref
import ref_mesh_ray as refr
import ref_mesh_surface as refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_inside.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tsi_crossings", "tsi_crossings_workspace_bytes", "tsi_last_error", "tsi_signed_distance"]


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_inside", ("diff_triangle_rasterization_2D", "_abi.py"))


INSIDE_SIGNATURES = _abi_module().INSIDE_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def inside_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_inside.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_inside.so"
    return path


@pytest.fixture(scope="module")
def lib(inside_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_inside(ctypes.CDLL(inside_path))


def _header_prototypes():
    """name -> number of parameters of every tsi_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsi_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


def _one(o, d, v, f, **kw):
    h, w2, t = ref.crossings(np.array([o], np.float32), np.array(d, np.float32), v, f, **kw)
    return int(h[0]), int(w2[0]), int(t[0])


# ---- known answers of the reference on the cube [-1, 1]^3 -------------------------------------------------------------------------------
def test_cube_known_answers_centre_outside_edge_diagonal_graze_and_corner():
    v, f = ref.cube()
    tri = v[f].astype(np.float64)
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.einsum("ij,ij->i", normal, tri.mean(axis=1)) > 0).all()  # the faces look outwards
    for d in ref.DIRECTIONS:
        assert _one((0, 0, 0), d, v, f) == (1, -2, 0)        # from the centre: one back
        assert _one((3, 0.1, 0.2), d, v, f) == (0, 0, 0)     # outside, looking away or past
    assert _one((0, 0, 0.3), (1, 1, 0), v, f) == (2, -2, 0)  # through a cube edge: two half crossings on equal sides are one crossing
    assert _one((0, 0, 0), (1, 0, 0), v, f) == (2, -2, 0)    # along a face diagonal: the two faces of the square share the hit
    assert _one((3, -1, 0.3), (-1, 1, 0), v, f) == (2, 0, 0)  # grazing an edge: a front and a back, no crossing
    h, w2, t = _one((0, 0, 0), (1, 1, 1), v, f)              # through a corner: every face at it reports a touch
    assert (h, w2, t) == (6, 0, 6) and not ref.clean(np.array([h]), np.array([w2]), np.array([t]))[0]


def test_reversed_nested_and_cavity_cubes():
    v, f = ref.cube()
    for d in ref.DIRECTIONS:
        assert _one((0, 0, 0), d, *ref.cube(reverse=True)) == (1, 2, 0)
        both = ref.join((v, f), ref.cube(0.5))  # a half-size cube inside, same orientation: wound twice
        assert _one((0, 0, 0), d, *both) == (2, -4, 0)
        cavity = ref.join((v, f), ref.cube(0.5, reverse=True))
        assert _one((0, 0, 0), d, *cavity) == (2, 0, 0)
        assert _one((0.75, 0.1, 0.2), d, *cavity)[1:] == (-2, 0)  # between the two: one or three hits, the way through the cavity cancels
    w, decided, _ = ref.winding_number(np.array([[0, 0, 0], [0.75, 0.1, 0.2], [3, 0.1, 0.2]], np.float32), *both)
    assert w.tolist() == [2, 1, 0] and decided.all()
    p = np.array([[0, 0, 0], [0.75, 0.1, 0.2], [3, 0.1, 0.2]], np.float32)
    assert ref.contains_points(p, *both, rule="nonzero")[0].tolist() == [True, True, False]
    assert ref.contains_points(p, *both, rule="odd")[0].tolist() == [False, True, False]
    assert ref.contains_points(p, *ref.cube(reverse=True), rule="positive")[0].tolist() == [False, False, False]
    assert ref.contains_points(p, *ref.cube(reverse=True), rule="nonzero")[0].tolist() == [True, True, False]
    sdf, face, decided = ref.signed_distance(p, *cavity)
    assert decided.all() and sdf.tolist() == [0.5, -0.25, 2.0] and (face >= 0).all()  # the cavity is outside


def test_random_points_around_a_closed_mesh_are_clean_along_all_three_directions():
    v, f = refr.closed_mesh(2, 0)
    rng = np.random.default_rng(1)
    p = rng.uniform(-1.5, 1.5, (2000, 3)).astype(np.float32)
    seen = set()
    for d in ref.DIRECTIONS:
        h, w2, t = ref.crossings(p, d, v, f)
        assert ref.clean(h, w2, t).all()
        w = -(w2 // 2)
        assert np.isin(w, (0, 1)).all()
        seen.add(tuple(w.tolist()))
    assert len(seen) == 1  # the three directions agree
    w = np.array(next(iter(seen)))
    assert 200 < w.sum() < 1800
    # star-shaped around the origin: inside means nearer to the origin than the surface along the point's own ray
    face, t, _, _ = refr.cast(np.zeros_like(p), p, v, f)
    assert (face >= 0).all() and np.array_equal(w == 1, t > 1.0)
    # the shared form is the per-ray form
    for a, b in zip(ref.crossings(p[:100], ref.DIRECTIONS[1], v, f), ref.crossings(p[:100], np.tile(ref.DIRECTIONS[1], (100, 1)), v, f)):
        assert np.array_equal(a, b)


def test_the_17_cubed_grid_over_the_cube_leaves_its_corners_to_the_distance():
    v, f = ref.cube()
    p = ref.grid_points((-2.0, -2.0, -2.0), 0.25, (17, 17, 17))
    assert p.shape == (4913, 3) and p[0].tolist() == [-2, -2, -2] and p[1].tolist() == [-1.75, -2, -2] and p[-1].tolist() == [2, 2, 2]
    corner = (np.abs(p) == 1).all(axis=1)
    assert corner.sum() == 8
    for d in ref.DIRECTIONS:
        h, w2, t = ref.crossings(p, d, v, f)
        assert np.array_equal(~ref.clean(h, w2, t), corner)
    w, decided, tried = ref.winding_number(p, v, f)
    assert np.array_equal(~decided, corner) and tried.sum(axis=1).tolist() == [4913, 8, 8]
    sdf, _, decided = ref.signed_distance(p, v, f)
    assert decided.all()  # dist2 == 0 decides where no ray does
    on = (np.abs(p).max(axis=1) == 1)
    assert (sdf[on] == 0).all() and not np.signbit(sdf[on]).any()
    strictly_in = np.abs(p).max(axis=1) < 1
    assert (sdf[strictly_in] < 0).all() and (sdf[~strictly_in & ~on] > 0).all() and strictly_in.sum() == 343
    assert np.array_equal(sdf[strictly_in], (np.abs(p[strictly_in]).max(axis=1) - 1).astype(np.float32))


def test_signed_distance_cases_of_the_header():
    v, f = ref.cube()
    p = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 1, 1], [0.5, 0.25, 2]], np.float32)
    sdf, face, decided = ref.signed_distance(p, v, f)
    assert sdf[0] == -1 and decided[0] and np.isnan(sdf[1]) and not decided[1] and face[1] == -1
    assert sdf[2] == 0 and decided[2] and sdf[3] == 1 and decided[3]
    sdf, face, decided = ref.signed_distance(p, v, np.zeros((0, 3), np.int32))  # no face: no distance
    assert np.isnan(sdf).all() and not decided.any() and (face == -1).all()
    # an open mesh (one face of the cube removed): the rays through the hole's rim leave winding2 odd; a ray that leaves through the hole is
    # clean and says outside -- the caller's business, the counts are what they are
    h, w2, t = ref.crossings(np.zeros((1, 3), np.float32), np.array([1, 0, 0], np.float32), v, f[~((v[f][:, :, 0] == 1).all(axis=1))])
    assert (h[0], w2[0], t[0]) == (0, 0, 0)
    h, w2, t = ref.crossings(np.array([[0, 0, 0.3]], np.float32), np.array([1, 1, 0], np.float32), v, f[~((v[f][:, :, 0] == 1).all(axis=1))])
    assert (h[0], w2[0], t[0]) == (1, -1, 0) and not ref.clean(h, w2, t)[0]  # a boundary edge: odd


def test_ranges_limit_what_is_counted():
    v, f = ref.join(ref.cube(), ref.cube(0.5))
    o, d = (-3, 0.1, 0.2), (1, 0, 0)
    assert _one(o, d, v, f) == (4, 0, 0)
    assert _one(o, d, v, f, tmax=3.0) == (2, 4, 0)               # both fronts
    assert _one(o, d, v, f, tmin=3.0) == (2, -4, 0)              # both backs
    assert _one(o, d, v, f, tmin=2.0, tmax=2.0) == (1, 2, 0)     # both ends are closed
    assert _one(o, d, v, f, t_limit=np.array([2.25], np.float32)) == (1, 2, 0)
    assert _one(o, d, v, f, t_limit=np.array([np.nan], np.float32)) == (-1, 0, 0)
    assert _one(o, (0, 0, 0), v, f) == (-1, 0, 0) and _one((np.inf, 0, 0), d, v, f) == (-1, 0, 0)
    assert _one(o, d, v, np.zeros((0, 3), np.int32)) == (0, 0, 0)
    assert _one(o, d, v, f, keep=np.arange(24) < 12) == (2, 0, 0)


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(inside_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsi_last_error.restype = ctypes.c_char_p; "
            "l.tsi_crossings_workspace_bytes.restype = ctypes.c_size_t; print(l.tsi_crossings_workspace_bytes(1000) >= 32000, repr(l.tsi_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, inside_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(inside_path):
    out = subprocess.run(["nm", "-D", "--defined-only", inside_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", inside_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", inside_path], capture_output=True, text=True).stdout
    assert "libts_inside.so" in dynamic
    for other in ("libts2d.so", "libts_geom.so", "libts_bvh.so", "libts_ray.so"):
        assert other not in dynamic


def test_header_text_stays_out_of_the_other_libraries_lists():
    """tests/test_cabi_cpu.py strips only block comments before it collects the names of libts2d.so's entry points from every header."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr)_[a-z0-9_]+)\s*\(", text)
    full = open(HEADER).read()
    for word in ("HALF crossings", "monotone", "bit for bit", "-ffp-contract=off", "ts_ray.h", "ts_bvh.h", "0.7548777", "-0.4301597", "0.8793852",
                 "only_undecided"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(INSIDE_SIGNATURES)
    for name, arity in declared.items():
        assert len(INSIDE_SIGNATURES[name][1]) == arity, name
    assert declared["tsi_crossings"] == 17 and declared["tsi_signed_distance"] == 10
    abi = _abi_module()
    for table in (abi.SIGNATURES, abi.LAB_SIGNATURES, abi.GEOM_SIGNATURES, abi.BVH_SIGNATURES, abi.RAY_SIGNATURES, abi.ATLAS_SIGNATURES):
        assert not set(INSIDE_SIGNATURES) & set(table)
    assert INSIDE_SIGNATURES["tsi_crossings"][1][5:7] == [ctypes.c_double, ctypes.c_double]


def test_python_and_header_name_the_same_three_directions():
    text = open(os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "mesh_inside.py")).read()
    table = re.search(r"INSIDE_DIRECTIONS = \((.*?)\)\)", text, flags=re.S).group(1)
    got = np.array([float(x) for x in re.findall(r"-?\d+\.\d+", table)], np.float32).reshape(3, 3)
    assert np.array_equal(got, ref.DIRECTIONS)
    line = re.search(r"clean:\s+(\(.*\))\.", open(HEADER).read()).group(1)
    assert np.array_equal(np.array([float(x) for x in re.findall(r"-?\d+\.\d+", line)], np.float32).reshape(3, 3), ref.DIRECTIONS)
    n = np.linalg.norm(ref.DIRECTIONS.astype(np.float64), axis=1)
    assert (np.abs(n - 1.0) < 1e-3).all() and (np.abs(ref.DIRECTIONS) > 0.2).all()  # about unit, no axis nearly zero: t is about a distance


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_inside", ("build.py",))
    assert list(build.INSIDE_SOURCES) == ["mesh_inside.hip", "api_inside.hip"] and build.INSIDE_SHARED == ["radix_sort"]
    assert "-ffp-contract=off" in build.INSIDE_SOURCES["mesh_inside.hip"]
    assert build.inside_units() == ["mesh_inside", "api_inside"]
    cmd = build.inside_command("mesh_inside", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert build.inside_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_inside", "api_inside", "radix_sort")]
    for others in (build.units(), build.geom_units(), build.bvh_units(), build.ray_units()):
        assert not {"mesh_inside", "api_inside"} & set(others)  # its own library only
    assert build.INSIDE_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_inside.so")
    for header in ("ts_inside_launch.h", "ts_ray_tests.h", "ts_bvh_layout.h", os.path.join("..", "..", "include", "ts_inside.h")):
        assert header in build.HEADERS
    with pytest.raises(ValueError):
        build.inside_command("mesh_ray")


def test_built_objects_carry_the_flags_and_the_ray_tests_are_one_text(inside_path):
    build = _load("ts2d_build_inside2", ("build.py",))
    assert "-ffp-contract=off" in open(os.path.join(build.OBJ_DIR, "mesh_inside.o.cmd")).read()  # what the object on disk was compiled with
    assert "-soname,libts_inside.so" in open(build.INSIDE_LIB + ".cmd").read()
    for unit in ("mesh_ray.hip", "mesh_inside.hip"):  # both include the tests and the layout, neither restates them
        text = open(os.path.join(build.CSRC, unit)).read()
        assert '#include "ts_ray_tests.h"' in text and '#include "ts_bvh_layout.h"' in text
        assert "slab_axis(double" not in text and "struct Leaf" not in text and "0x1p-40" not in text
    assert "0x1p-40" in open(os.path.join(build.CSRC, "ts_ray_tests.h")).read()


def test_size_query_is_monotone_and_index_size_agrees_with_the_bvh_library(lib, inside_path):
    sizes = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 65_537, 640_000, 2_499_999, 2_500_000, 2_500_001, 2_600_000, 5_000_000, 100_000_000,
             2 ** 31 - 1025]
    prev = -1
    for n in sizes:
        got = lib.tsi_crossings_workspace_bytes(n)
        assert got >= 32 * n and got >= prev, (n, got, prev)  # the sorted origins and two key / value pairs
        prev = got
    from diff_triangle_rasterization_2D import _abi
    here = os.path.dirname(inside_path)
    bvh = _abi.bind_bvh(ctypes.CDLL(os.path.join(here, "libts_bvh.so")))
    ray = _abi.bind_ray(ctypes.CDLL(os.path.join(here, "libts_ray.so")))
    assert [lib.tsi_crossings_workspace_bytes(n) for n in sizes] == [ray.tsr_cast_workspace_bytes(n) for n in sizes]  # the same front half
    P, big = 0x1000, 1 << 40
    for F in (1, 8, 9, 64, 65, 513, 4097, 1_000_000):  # one byte short of the other library's size query is refused, the size itself is not
        need = bvh.tsb_bvh_bytes(F)
        rc = lib.tsi_crossings(1, P, P, 0, None, 0.0, 1.0, F, P, need - 1, P, P, P, None, P, big, None)
        assert rc == INVALID and b"bvh too small" in lib.tsi_last_error() and str(need).encode() in lib.tsi_last_error()
        assert lib.tsi_crossings(1, P, P, 0, None, 0.0, 1.0, F, P, need, P, P, P, None, P, 0, None) == INVALID
        assert b"workspace too small" in lib.tsi_last_error()


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    big = 1 << 40
    nan, inf = float("nan"), float("inf")

    def refused(rc, word, code=INVALID):
        assert rc == code, rc
        text = lib.tsi_last_error()
        assert text and word.encode() in text, text

    def cross(Q=1, origins=P, directions=P, shared=0, t_limit=None, tmin=0.0, tmax=inf, F=1, bvh=P, bvh_bytes=big, hits=P, winding2=P, touches=P,
              ws=P, ws_bytes=big):
        return lib.tsi_crossings(Q, origins, directions, shared, t_limit, tmin, tmax, F, bvh, bvh_bytes, hits, winding2, touches, None, ws, ws_bytes,
                                 None)

    refused(cross(Q=-1), "Q")
    refused(cross(F=-1), "F")
    refused(cross(Q=2 ** 31 - 1), "at most")
    refused(cross(F=2 ** 31 - 1), "at most")
    refused(cross(F=2 ** 30), "half crossings", CAPACITY)
    refused(cross(F=2 ** 31 - 1025), "half crossings", CAPACITY)
    refused(cross(F=2 ** 30 - 1, bvh_bytes=1000), "bvh too small")  # the largest F that is taken
    refused(cross(origins=None), "null")
    refused(cross(directions=None), "null")
    refused(cross(hits=None), "null")
    refused(cross(winding2=None), "null")
    refused(cross(touches=None), "null")
    refused(cross(bvh=None), "null")
    refused(cross(ws=None), "null")
    refused(cross(F=1000, bvh_bytes=1000), "bvh too small")
    refused(cross(Q=1000, ws_bytes=lib.tsi_crossings_workspace_bytes(1000) - 1), "workspace too small")
    refused(cross(tmin=nan), "NaN")
    refused(cross(tmax=nan), "NaN")
    refused(cross(tmin=2.0, tmax=1.0), "exceeds")
    refused(cross(tmin=inf, tmax=-inf), "exceeds")
    refused(cross(shared=2), "shared_direction")
    refused(cross(shared=-1), "shared_direction")
    refused(cross(Q=0, tmin=nan), "NaN")  # the values are checked whatever the counts
    refused(cross(Q=0, F=2 ** 30), "half crossings", CAPACITY)
    assert cross(Q=0, origins=None, directions=None, bvh=None, bvh_bytes=0, hits=None, winding2=None, touches=None, ws=None, ws_bytes=0) == 0  # the no-op
    assert cross(Q=0, tmin=1.0, tmax=1.0, shared=1) == 0

    def sd(Q=1, dist2=P, winding2=P, touches=P, hits=P, rule=0, only=0, out=P, decided=P):
        return lib.tsi_signed_distance(Q, dist2, winding2, touches, hits, rule, only, out, decided, None)

    refused(sd(Q=-1), "Q")
    refused(sd(Q=2 ** 31 - 1), "at most")
    refused(sd(rule=3), "rule")
    refused(sd(rule=-1), "rule")
    refused(sd(only=2), "only_undecided")
    refused(sd(Q=0, rule=7), "rule")
    for name in ("dist2", "winding2", "touches", "hits", "out", "decided"):
        refused(sd(**{name: None}), "null")
    assert sd(Q=0, dist2=None, winding2=None, touches=None, hits=None, out=None, decided=None) == 0
    assert sd(Q=0, rule=2, only=1) == 0


def test_missing_library_is_an_import_error_and_the_rest_still_imports(tmp_path, inside_path):
    """Without libts_inside.so, diff_recon_hip.mesh_inside raises and names the build command; the package, ray_cast included, still imports."""
    src = os.path.dirname(inside_path)
    pkg = tmp_path / "diff_recon_hip"
    pkg.mkdir()
    for name in os.listdir(src):
        if name.endswith(".py") or name in ("libts_geom.so", "libts_bvh.so", "libts_ray.so"):
            shutil.copy(os.path.join(src, name), pkg / name)
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([str(tmp_path), os.path.join(ROOT, "triangle-splatting_amd")])}
    code = ("import diff_recon_hip, sys\n"
            "assert str(diff_recon_hip.__file__).startswith(sys.argv[1]), diff_recon_hip.__file__\n"
            "print('others', callable(diff_recon_hip.MeshBVH.closest), callable(diff_recon_hip.MeshBVH.ray_crossings), callable(diff_recon_hip.ray_cast))\n"
            "try:\n    diff_recon_hip.signed_distance\nexcept ImportError as e:\n    print('lazy', e)\n"
            "import diff_recon_hip.mesh_inside\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, env=env)
    assert "others True True True" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert "lazy" in r.stdout and "libts_inside.so" in r.stdout
    assert r.returncode != 0 and "ImportError" in r.stderr
    assert "libts_inside.so" in r.stderr and "no CPU fallback" in r.stderr and "triangle-splatting_amd/build.py" in r.stderr


def test_package_re_exports_the_feature(inside_path):
    import inspect
    import diff_recon_hip
    from diff_recon_hip import mesh_inside
    for name in ("INSIDE_DIRECTIONS", "RayCrossings", "ray_crossings", "winding_number", "contains_points", "signed_distance", "mesh_to_sdf",
                 "remesh", "mesh_volume_iou"):
        assert getattr(diff_recon_hip, name) is getattr(mesh_inside, name)
    assert sorted(mesh_inside.__all__) == sorted(diff_recon_hip._INSIDE_NAMES)
    assert diff_recon_hip.RayCrossings._fields == ("hits", "winding2", "touches")
    assert list(inspect.signature(diff_recon_hip.ray_crossings).parameters) == ["bvh", "origins", "directions", "tmin", "tmax", "t_limit", "leaf_visits"]
    assert list(inspect.signature(diff_recon_hip.mesh_to_sdf).parameters) == ["mesh", "origin", "voxel_size", "dims", "trunc", "rule"]
    assert list(inspect.signature(diff_recon_hip.remesh).parameters) == ["mesh", "resolution", "offset", "pad_voxels"]
    assert list(inspect.signature(diff_recon_hip.mesh_volume_iou).parameters)[:3] == ["mesh_a", "mesh_b", "resolution"]
    for fn in (diff_recon_hip.contains_points, diff_recon_hip.signed_distance, diff_recon_hip.mesh_to_sdf):
        assert inspect.signature(fn).parameters["rule"].default == "nonzero"
    assert np.array_equal(np.array(diff_recon_hip.INSIDE_DIRECTIONS, np.float32), ref.DIRECTIONS)
    assert callable(diff_recon_hip.MeshBVH.ray_crossings)
    with pytest.raises(ValueError):
        mesh_inside._rule("even")


def test_example_refuses_remesh_without_extract_mesh():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), "--remesh", "32"], capture_output=True, text=True)
    assert r.returncode == 2 and "--remesh remeshes the mesh of --extract-mesh" in r.stderr
