"""CPU tests of mesh smoothing and normals (no GPU): the numpy reference keeps the promises of include/ts_smooth.h on the fixtures of
ref_mesh_simplify and reproduces the figures of DESIGN.md 16j, libts_smooth.so is a library of its own with exactly the C ABI of the header,
and every argument check answers before any HIP call."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_simplify as fixtures
import ref_mesh_smooth as ref
import ref_mesh_weld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_smooth.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tss_adjacency", "tss_face_normals", "tss_last_error", "tss_smooth", "tss_vertex_normals", "tss_workspace_bytes"]
SPHERE_ANALYTIC_CENTRE, SPHERE_RADIUS = np.array([13.63, 13.29, 13.57]), 9.3


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_smooth", ("diff_triangle_rasterization_2D", "_abi.py"))


SMOOTH_SIGNATURES = _abi_module().SMOOTH_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def smooth_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_smooth.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_smooth.so"
    return path


@pytest.fixture(scope="module")
def lib(smooth_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_smooth(ctypes.CDLL(smooth_path))


@functools.lru_cache(maxsize=None)
def _sphere():
    """The sphere fixture, its adjacency, the noisy copy, and the four smoothed meshes of the table: computed once, never changed."""
    v, f = fixtures.sphere_mesh()
    assert v.shape == (4834, 3) and f.shape == (9664, 3) and v.dtype == np.float32
    adj = ref.adjacency(len(v), f)
    vn = ref.noisy(v)
    meshes = {"clean": v, "taubin": ref.smooth(v, adj), "laplacian": ref.smooth(v, adj, mu=0.0),
              "noisy": vn, "noisy_taubin": ref.smooth(vn, adj), "noisy_laplacian": ref.smooth(vn, adj, mu=0.0)}
    return v, f, adj, meshes


def _header_prototypes():
    """name -> number of parameters of every tss_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tss_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


# ---- the reference reproduces the prototype's figures and holds the conditions ---------------------------------------------------------------
# operation -> (volume / the clean sphere's, radial std about the clean sphere's vertex mean, mean face normal . radial direction, inverted faces)
TABLE = {"clean": (1.0, 0.0109, 0.9991, 0), "taubin": (1.0017, 0.0103, None, None), "laplacian": (0.9703, 0.0352, None, None),
         "noisy": (1.0014, 0.1520, 0.5516, 1631), "noisy_taubin": (1.0030, 0.0598, 0.9892, 0), "noisy_laplacian": (0.9714, 0.0424, None, None)}


def _figures(name):
    v, f, _, meshes = _sphere()
    centre = ref.centroid(v)
    w = meshes[name]
    dot, inverted = ref.normal_dot_radial(w, f, centre)
    return fixtures.signed_volume(w, f) / fixtures.signed_volume(v, f), ref.radial_std(w, centre), dot, inverted


@pytest.mark.parametrize("name", sorted(TABLE))
def test_reference_reproduces_the_table_within_the_digits_shown(name):
    volume, std, dot, inverted = _figures(name)
    print(f"{name}: volume ratio {volume:.6f}, radial std {std:.6f}, normal . radial {dot:.6f}, {inverted} faces inverted")
    want = TABLE[name]
    assert abs(volume - want[0]) < 0.5e-4 and abs(std - want[1]) < 0.5e-4
    if want[2] is not None:
        assert abs(dot - want[2]) < 0.5e-4 and inverted == want[3]


def test_taubin_keeps_the_volume_and_removes_the_noise_where_the_laplacian_shrinks():
    fig = {name: _figures(name) for name in TABLE}
    for src, out, lap in (("clean", "taubin", "laplacian"), ("noisy", "noisy_taubin", "noisy_laplacian")):
        assert abs(fig[out][0] / fig[src][0] - 1.0) < 0.005      # Taubin, 10 iterations: within 0.5 % of the input's volume
        assert abs(fig[lap][0] / fig[src][0] - 1.0) > 0.025      # the Laplacian: off by more than 2.5 %
    assert fig["noisy_taubin"][1] < 0.5 * fig["noisy"][1]         # radial std below half the input's
    assert fig["noisy_taubin"][3] == 0 and fig["noisy_taubin"][2] > 0.98  # no inverted face; mean face normal . radial
    assert fig["noisy"][3] > 1000                                  # the input of that row really is folded over


def test_sphere_adjacency_is_all_interior_with_2e_entries():
    v, f, adj, _ = _sphere()
    V, F = len(v), len(f)
    assert (adj["vertex_class"] == ref.INTERIOR).all()
    assert adj["counts"] == [2 * (V + F - 2), 0, 2 * (V + F - 2), 0] and adj["counts"][0] == 28992  # Euler: E = V + F - 2
    degree = np.diff(adj["offsets"])
    assert degree.min() == 4 and degree.max() == 10 and adj["offsets"][V] == 28992
    assert (adj["neighbors"][28992:] == -1).all() and (adj["edge_faces"][28992:] == 0).all() and len(adj["neighbors"]) == 6 * F
    # symmetric by construction, rows ascending
    row = np.repeat(np.arange(V), degree)
    col = adj["neighbors"][:28992].astype(np.int64)
    assert set(zip(row.tolist(), col.tolist())) == set(zip(col.tolist(), row.tolist()))
    assert all((np.diff(col[adj["offsets"][i]:adj["offsets"][i + 1]]) > 0).all() for i in range(V))


def test_cube_and_plane_adjacency():
    v, f = fixtures.cube_mesh()
    adj = ref.adjacency(len(v), f)
    degree = np.bincount(np.diff(adj["offsets"]))
    assert degree[3] == 4 and degree[6] == len(v) - 4 and degree.sum() == len(v)  # degree 6, except four vertices of degree 3
    assert (adj["vertex_class"] == ref.INTERIOR).all()
    v, f, _, _ = fixtures.plane_grid()
    assert v.shape == (625, 3) and f.shape == (1152, 3)
    adj = ref.adjacency(len(v), f)
    cls = np.bincount(adj["vertex_class"], minlength=4)
    assert cls.tolist() == [0, 529, 96, 0]          # 96 boundary, 529 interior
    assert adj["counts"] == [3552, 192, 3360, 0]    # 192 entries used by one face, 3360 by two


@pytest.mark.parametrize("fixture", ["sphere", "cube", "plane", "soup"])
def test_counts_are_twice_the_edge_census(fixture):
    if fixture == "soup":  # boundary, manifold and non-manifold edges at once; no repeated index, so the census applies as it is
        rng = np.random.default_rng(11)
        V = 40
        f = np.array([rng.permutation(V)[:3] for _ in range(160)])
        f = np.concatenate([f, f[:20], f[20:30, ::-1]])
    else:
        v, f = {"sphere": fixtures.sphere_mesh, "cube": fixtures.cube_mesh, "plane": lambda: fixtures.plane_grid()[:2]}[fixture]()
        V = len(v)
    adj, topo = ref.adjacency(V, f), ref_mesh_weld.topology(V, f)
    assert adj["counts"] == [2 * topo[k] for k in ("edges", "boundary", "manifold", "nonmanifold")]
    if fixture == "soup":
        assert min(adj["counts"][1:]) > 0 and sorted(np.unique(adj["vertex_class"]).tolist()) != [ref.INTERIOR]
    keep = np.arange(len(f)) % 3 != 0
    adj, topo = ref.adjacency(V, f, keep), ref_mesh_weld.topology(V, f, keep)
    assert adj["counts"] == [2 * topo[k] for k in ("edges", "boundary", "manifold", "nonmanifold")]


def test_classes_of_a_small_hand_made_mesh():
    # a fan of three faces around edge (0, 1), a lone triangle, a face with a repeated index, one out of range, an unused vertex
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [5, 6, 7], [8, 8, 9], [0, 1, 11], [1, 2, -1]])
    adj = ref.adjacency(11, f)
    assert adj["vertex_class"].tolist() == [3, 3, 2, 2, 2, 2, 2, 2, 0, 0, 0]
    assert adj["offsets"].tolist() == [0, 4, 8, 10, 12, 14, 16, 18, 20, 20, 20, 20]
    assert adj["neighbors"][:8].tolist() == [1, 2, 3, 4, 0, 2, 3, 4] and adj["edge_faces"][:8].tolist() == [3, 1, 1, 1, 3, 1, 1, 1]
    assert adj["counts"] == [20, 18, 0, 2]
    # two closed fans that touch in one vertex: INTERIOR by the rule (the class looks at edges)
    tet = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    other = np.where(tet == 0, 0, tet + 3)
    assert (ref.adjacency(7, np.concatenate([tet, other]))["vertex_class"] == ref.INTERIOR).all()


def test_fixed_boundary_stays_and_curve_slides_within_the_boundary_neighbours_span():
    v, f, p0, nrm = fixtures.plane_grid()
    v = ref.noisy(v, 0.05, seed=3)
    adj = ref.adjacency(len(v), f)
    boundary = adj["vertex_class"] == ref.BOUNDARY
    fixed = ref.smooth(v, adj, mode=ref.FIXED)
    assert fixed[boundary].tobytes() == v[boundary].tobytes() and (fixed[~boundary] != v[~boundary]).any(1).all()
    # one lambda step (mu = 0 adds k d = 0): a boundary vertex moves by lambda (mean of its BOUNDARY neighbours - itself)
    curve = ref.smooth(v, adj, iterations=1, lam=0.5, mu=0.0, mode=ref.CURVE)
    q = v.astype(np.float64)
    worst = 0.0
    for i in np.nonzero(boundary)[0]:
        a, b = adj["offsets"][i], adj["offsets"][i + 1]
        nb = adj["neighbors"][a:b][adj["edge_faces"][a:b] == 1]
        assert len(nb) == 2 and boundary[nb].all()
        want = q[i] + 0.5 * (((0.0 + q[nb[0]]) + q[nb[1]]) / 2.0 - q[i])
        assert np.array_equal(curve[i], want.astype(np.float32))
        basis = (q[nb] - q[i]).T  # the displacement lies in the span of the two boundary edges at i
        d = curve[i].astype(np.float64) - q[i]
        residual = np.linalg.norm(d - basis @ np.linalg.lstsq(basis, d, rcond=None)[0])
        worst = max(worst, residual / ref.ulp32(np.abs(curve[i]).max()))
    print(f"CURVE: largest residual outside the boundary neighbours' span {worst:.3f} fp32 ulps of the output vertex's largest coordinate")
    assert worst <= 0.9  # the one rounding to fp32 at the end, half an ulp per axis: at most sqrt(3) / 2 = 0.87 ulp
    assert (curve[boundary] != v[boundary]).any()
    free = ref.smooth(v, adj, mode=ref.FREE)
    assert (free[boundary] != v[boundary]).any(1).all()


def test_max_move_holds_per_axis_and_special_vertices_stay():
    v, f, adj, meshes = _sphere()
    vn = meshes["noisy"]
    free = np.abs(meshes["noisy_taubin"].astype(np.float64) - vn).max()
    for bound in (0.0, 0.05, 0.3):
        out = ref.smooth(vn, adj, max_move=bound)
        over = np.abs(out.astype(np.float64) - vn.astype(np.float64)) - np.float64(np.float32(bound))
        print(f"max_move {bound}: largest displacement {over.max() + bound:.6f} (unbounded: {free:.4f}), {int((over >= 0).sum())} coordinates at the bound")
        assert (over <= ref.ulp32(out)).all()  # up to one fp32 ulp of the output: the one rounding at the end
        assert bound >= free or (over >= -ref.ulp32(out)).any()  # the bound binds
        if bound == 0.0:
            assert out.tobytes() == vn.tobytes()
    assert ref.smooth(vn, adj, iterations=0).tobytes() == vn.tobytes()
    w = vn.copy()
    w[5] = (np.nan, 1.0, 2.0)
    w[9, 2] = -np.inf
    pinned = np.zeros(len(w), np.uint8)
    pinned[[20, 21]] = 1
    out = ref.smooth(w, adj, pinned=pinned)
    for i in (5, 9, 20, 21):
        assert out[i].tobytes() == w[i].tobytes()
    assert np.isfinite(np.delete(out, [5, 9], axis=0)).all()  # a dead vertex never enters a sum


def test_area_vertex_normals_of_the_sphere_point_outward():
    v, f, _, _ = _sphere()
    for weighting in (ref.AREA, ref.UNIFORM):
        n, valid, s = ref.vertex_normals(v, f, weighting)
        assert valid.all() and np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 1e-6
        r = v.astype(np.float64) - SPHERE_ANALYTIC_CENTRE
        dots = (n * (r / np.linalg.norm(r, axis=1, keepdims=True))).sum(1)
        # A face of the level set lies in one voxel (diagonal sqrt(3)) with its corners on the sphere up to the interpolation error, so its
        # normal is within about sqrt(3) / R = 0.186 rad of the radial direction at any of its corners; a vertex normal is a positive
        # combination of such normals and stays in that cone: cos(0.186) = 0.9827.
        print(f"weighting {weighting}: smallest vertex normal . radial direction {dots.min():.5f}, mean {dots.mean():.5f}")
        assert dots.min() > 0.98
    fn, fvalid = ref.face_normals(v, f)
    assert fvalid.all() and np.abs(np.linalg.norm(fn.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    # degenerate and dead faces come out invalid; a face counts once for a vertex
    w = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0]], np.float32)
    g = np.array([[0, 1, 2], [0, 1, 3], [0, 0, 1], [0, 1, 4], [0, 1, 7], [2, 1, 0]])
    fn, fvalid = ref.face_normals(w, g)
    assert fvalid.tolist() == [1, 0, 0, 0, 0, 1] and fn[0].tolist() == [0, 0, 1] and fn[5].tolist() == [0, 0, -1] and not fn[1:5].any()
    n, valid, s = ref.vertex_normals(w, g, ref.AREA, keep=np.array([1, 1, 1, 1, 1, 0]))
    assert s[:3].tolist() == [[0, 0, 1]] * 3 and valid.tolist() == [1, 1, 1, 0, 0]


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(smooth_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tss_last_error.restype = ctypes.c_char_p; "
            "l.tss_workspace_bytes.restype = ctypes.c_size_t; print(l.tss_workspace_bytes(100000, 200000) >= 24 * 4 * 200000, "
            "repr(l.tss_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, smooth_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(smooth_path):
    out = subprocess.run(["nm", "-D", "--defined-only", smooth_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", smooth_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", smooth_path], capture_output=True, text=True).stdout
    assert "libts_smooth.so" in dynamic
    for other in ("libts2d.so", "libts_geom.so", "libts_bvh.so", "libts_ray.so", "libts_volume.so", "libts_color.so", "libts_simplify.so"):
        assert other not in dynamic


def test_header_defines_no_struct_and_states_the_contract():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsv|tsc|tsq)_[a-z0-9_]+)\s*\(", text)  # a prefix of its own
    assert "struct" not in text
    full = open(HEADER).read()
    for word in ("-ffp-contract=off", "ONE thread's work", "serial", "Jacobi", "rounded to fp32 once", "LIVE", "two closed fans touch",
                 "ascending face index", "nobody waits for anybody", "TSS_BOUNDARY_CURVE", "TSS_NORMAL_UNIFORM", "twice the matching", "357913941"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(SMOOTH_SIGNATURES) and len(declared) == 6
    for name, arity in declared.items():
        assert len(SMOOTH_SIGNATURES[name][1]) == arity, name
    assert declared["tss_adjacency"] == 12 and declared["tss_smooth"] == 17 and declared["tss_face_normals"] == 8 and declared["tss_vertex_normals"] == 12
    abi = _abi_module()
    tables = [abi.SIGNATURES, abi.LAB_SIGNATURES, abi.GEOM_SIGNATURES, abi.BVH_SIGNATURES, abi.RAY_SIGNATURES, abi.VOLUME_SIGNATURES,
              abi.COLOR_SIGNATURES, abi.SIMPLIFY_SIGNATURES, abi.SMOOTH_SIGNATURES]
    for a in range(len(tables)):
        for b in range(a + 1, len(tables)):
            assert not set(tables[a]) & set(tables[b])  # no signature table overlaps another
    sig = SMOOTH_SIGNATURES["tss_smooth"][1]
    assert sig[8:10] == [ctypes.c_float] * 2 and sig[12] == ctypes.c_float and sig[15] == ctypes.c_size_t
    assert SMOOTH_SIGNATURES["tss_workspace_bytes"][0] == ctypes.c_size_t


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_smooth", ("build.py",))
    assert build.SMOOTH_SOURCES == {"mesh_smooth.hip": ["-ffp-contract=off"], "api_smooth.hip": []}
    assert build.smooth_units() == ["mesh_smooth", "api_smooth"] and build.SMOOTH_SHARED == ["radix_sort"]
    cmd = build.smooth_command("mesh_smooth", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert build.smooth_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_smooth", "api_smooth", "radix_sort")]
    for others in (build.units(), build.geom_units(), build.bvh_units(), build.ray_units(), build.volume_units(), build.color_units(),
                   build.simplify_units()):
        assert not {"mesh_smooth", "api_smooth"} & set(others)  # its own library only
    assert build.SMOOTH_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_smooth.so")
    for header in ("ts_smooth_launch.h", os.path.join("..", "..", "include", "ts_smooth.h")):
        assert header in build.HEADERS
    with pytest.raises(ValueError):
        build.smooth_command("mesh_simplify")


def test_built_objects_carry_the_flags(smooth_path):
    build = _load("ts2d_build_smooth2", ("build.py",))
    assert "-ffp-contract=off" in open(os.path.join(build.OBJ_DIR, "mesh_smooth.o.cmd")).read()  # what the object on disk was compiled with
    assert "-soname,libts_smooth.so" in open(build.SMOOTH_LIB + ".cmd").read()


def test_size_query_is_monotone_in_both_counts(lib):
    sizes = (0, 1, 2, 63, 1024, 1025, 4097, 100000, 416666, 416667, 2499999, 2500000, 2500001, 2600000, 5000000)
    for fixed in (0, 1000, 3000000):
        prev_v = prev_f = -1
        for n in sizes:
            by_v, by_f = lib.tss_workspace_bytes(n, fixed), lib.tss_workspace_bytes(fixed, n)
            assert by_v >= prev_v and by_f >= prev_f, (n, fixed)
            assert by_v >= 2 * 24 * n + n and by_f >= 24 * 4 * n  # the two float64 states and the flags; the four columns over 6 F slots
            prev_v, prev_f = by_v, by_f
    assert lib.tss_workspace_bytes(-5, -5) == lib.tss_workspace_bytes(0, 0)
    assert lib.tss_workspace_bytes(10, 2 ** 31 - 1) == lib.tss_workspace_bytes(10, 357913941)


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    Q = 0x2000
    big = 1 << 40
    nan, inf = float("nan"), float("inf")

    def refused(rc, word, code=INVALID):
        assert rc == code, rc
        text = lib.tss_last_error()
        assert text and word.encode() in text, text

    def adjacency(V=10, F=20, faces=P, keep=None, offsets=P, neighbors=P, edge_faces=P, cls=P, counts=P, ws=P, ws_bytes=big):
        return lib.tss_adjacency(V, F, faces, keep, offsets, neighbors, edge_faces, cls, counts, ws, ws_bytes, None)

    def smooth(V=10, vertices=P, offsets=P, neighbors=P, edge_faces=P, entries=60, cls=P, pinned=None, lam=0.5, mu=-0.53, iterations=10, mode=0,
               max_move=inf, out=Q, ws=P, ws_bytes=big):
        return lib.tss_smooth(V, vertices, offsets, neighbors, edge_faces, entries, cls, pinned, lam, mu, iterations, mode, max_move, out, ws,
                              ws_bytes, None)

    def fnormals(V=10, F=20, vertices=P, faces=P, keep=None, normal=P, valid=P):
        return lib.tss_face_normals(V, F, vertices, faces, keep, normal, valid, None)

    def vnormals(V=10, F=20, vertices=P, faces=P, keep=None, weighting=0, normal=P, valid=P, sums=None, ws=P, ws_bytes=big):
        return lib.tss_vertex_normals(V, F, vertices, faces, keep, weighting, normal, valid, sums, ws, ws_bytes, None)

    for call in (adjacency, smooth, fnormals, vnormals):
        refused(call(V=-1), ">= 0")
        refused(call(V=-(2 ** 31)), ">= 0")
    for call in (adjacency, fnormals, vnormals):
        refused(call(F=-1), ">= 0")
        refused(call(F=357913942), "exceeds", CAPACITY)
    for bad in (nan, inf, -inf):
        refused(smooth(lam=bad), "lambda and mu must be finite")
        refused(smooth(mu=bad), "lambda and mu must be finite")
    for bad in (-1, -(2 ** 31)):
        refused(smooth(iterations=bad), "iterations")
    for bad in (nan, -1e-9, -1.0, -inf):
        refused(smooth(max_move=bad), "max_move")
    for bad in (-1, 3, 7):
        refused(smooth(mode=bad), "boundary_mode")
        refused(vnormals(weighting=bad if bad != 3 else 2), "weighting")
    refused(smooth(entries=-1), "num_entries")
    for name in ("vertices", "offsets", "cls", "out"):
        refused(smooth(**{name: None}), "null")
    refused(smooth(neighbors=None), "neighbors is null")
    refused(smooth(edge_faces=None, mode=1), "edge_faces is null in TSS_BOUNDARY_CURVE")
    refused(smooth(out=P), "alias")
    refused(adjacency(counts=None), "counts is null")
    for name in ("offsets", "cls", "faces", "neighbors", "edge_faces"):
        refused(adjacency(**{name: None}), "null")
    for name in ("faces", "normal", "valid", "vertices"):
        refused(fnormals(**{name: None}), "null")
    for name in ("vertices", "normal", "valid"):
        refused(vnormals(**{name: None}), "null")
    refused(vnormals(faces=None), "faces is null")
    for call in (adjacency, smooth, vnormals):
        refused(call(ws=None), "workspace is null")
    need = lib.tss_workspace_bytes(1000, 2000)
    refused(adjacency(V=1000, F=2000, ws_bytes=need - 1), "workspace too small")
    assert str(need).encode() in lib.tss_last_error()
    refused(vnormals(V=1000, F=2000, ws_bytes=need - 1), "workspace too small")
    refused(smooth(V=1000, ws_bytes=lib.tss_workspace_bytes(1000, 0) - 1), "workspace too small")
    # the no-ops answer without touching anything either
    assert smooth(V=0, vertices=None, offsets=None, neighbors=None, edge_faces=None, entries=0, cls=None, out=None, ws=None, ws_bytes=0) == 0
    assert fnormals(F=0, faces=None, normal=None, valid=None) == 0
    assert vnormals(V=0, F=0, vertices=None, faces=None, normal=None, valid=None, ws=None, ws_bytes=0) == 0
    # what the checks accept, for the record: edge_faces may be null outside CURVE, +inf and 0 are both max_move
    # (those calls would reach the device, so they are made in tests/test_mesh_smooth_gpu.py)


def test_missing_library_is_an_import_error_and_the_package_still_imports(tmp_path, smooth_path):
    """Without libts_smooth.so, diff_recon_hip.mesh_smooth raises and names the build command; everything else still imports."""
    src = os.path.dirname(smooth_path)
    pkg = tmp_path / "diff_recon_hip"
    pkg.mkdir()
    for name in os.listdir(src):
        if name.endswith(".py") or (name.endswith(".so") and name != "libts_smooth.so"):
            shutil.copy(os.path.join(src, name), pkg / name)
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([str(tmp_path), os.path.join(ROOT, "triangle-splatting_amd")])}
    code = ("import diff_recon_hip, sys\n"
            "assert str(diff_recon_hip.__file__).startswith(sys.argv[1]), diff_recon_hip.__file__\n"
            "print('others', callable(diff_recon_hip.weld_mesh), callable(diff_recon_hip.fuse_mesh), callable(diff_recon_hip.simplify_mesh))\n"
            "try:\n    diff_recon_hip.smooth_mesh\nexcept ImportError as e:\n    print('lazy', e)\n"
            "import diff_recon_hip.mesh_smooth\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, env=env)
    assert "others True True True" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert "lazy" in r.stdout and "libts_smooth.so" in r.stdout
    assert r.returncode != 0 and "ImportError" in r.stderr
    assert "libts_smooth.so" in r.stderr and "no CPU fallback" in r.stderr and "triangle-splatting_amd/build.py" in r.stderr


def test_package_re_exports_the_feature_and_keeps_the_pinned_parameter_lists(smooth_path):
    import inspect

    import diff_recon_hip
    from diff_recon_hip import color_volume, mesh_simplify, mesh_smooth, volume
    names = ("MeshAdjacency", "SmoothedMesh", "vertex_adjacency", "smooth_mesh", "face_normals", "vertex_normals", "smooth_fused",
             "mesh_normal_consistency", "save_glb_shaded_mesh")
    assert diff_recon_hip._SMOOTH_NAMES == names
    for name in names:
        assert getattr(diff_recon_hip, name) is getattr(mesh_smooth, name)
    assert diff_recon_hip.mesh_smooth is mesh_smooth
    params = lambda fn: list(inspect.signature(fn).parameters)
    assert params(mesh_smooth.vertex_adjacency) == ["num_vertices", "faces", "keep"]
    assert params(mesh_smooth.smooth_mesh) == ["vertices", "faces", "iterations", "lam", "mu", "boundary", "pinned", "max_move", "adjacency"]
    defaults = {k: p.default for k, p in inspect.signature(mesh_smooth.smooth_mesh).parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == {"iterations": 10, "lam": 0.5, "mu": -0.53, "boundary": "fixed", "pinned": None, "max_move": None, "adjacency": None}
    assert params(mesh_smooth.face_normals) == ["vertices", "faces", "keep"]
    assert params(mesh_smooth.vertex_normals)[:4] == ["vertices", "faces", "weighting", "keep"]
    assert params(mesh_smooth.smooth_fused) == ["mesh", "volume", "iterations", "max_move_voxels", "kw"]
    assert params(mesh_smooth.mesh_normal_consistency) == ["mesh_a", "mesh_b", "samples", "seed"]
    assert params(mesh_smooth.save_glb_shaded_mesh) == ["path", "vertices", "faces", "vertex_normal", "vertex_color"]
    assert mesh_smooth.MeshAdjacency._fields == ("offsets", "neighbors", "edge_faces", "vertex_class", "stats")
    assert mesh_smooth.SmoothedMesh._fields == ("vertices", "adjacency", "stats")
    # the neighbours keep their parameter lists
    assert params(color_volume.save_glb_mesh) == ["path", "vertices", "faces", "vertex_color"]
    assert params(mesh_simplify.simplify_fused) == ["mesh", "volume", "simplify_cell", "min_piece_faces"]
    assert params(volume.fuse_mesh)[:4] == ["views", "vertices", "faces", "resolution"]
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_smooth.face_normals(torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_smooth.vertex_adjacency(4, torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="boundary"):
        mesh_smooth.smooth_mesh(torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32), boundary="loose")
    with pytest.raises(ValueError, match="max_move"):
        mesh_smooth.smooth_mesh(torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32), max_move=-1.0)
    with pytest.raises(ValueError, match="weighting"):
        mesh_smooth.vertex_normals(torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32), weighting="angle")


def test_shaded_glb_round_trips_through_read_glb(tmp_path, smooth_path):
    import torch
    from diff_recon_hip import save_glb_shaded_mesh
    from diff_recon_hip.mesh_renderer import load_glb_mesh
    from diff_recon_hip.raw_triangle import _accessor, read_glb
    v, f = fixtures.cube_mesh(n=3)
    n, valid, _ = ref.vertex_normals(v, f)
    assert valid.all()
    colour = np.random.default_rng(1).integers(0, 256, (len(v), 3)).astype(np.float64) / 255.0
    for name, col in (("shaded.glb", colour), ("plain.glb", None)):
        path = tmp_path / name
        save_glb_shaded_mesh(path, torch.from_numpy(v), f, n, col)
        doc, binary = read_glb(path)
        prim = doc["meshes"][0]["primitives"][0]
        assert sorted(prim["attributes"]) == (["COLOR_0", "NORMAL", "POSITION"] if col is not None else ["NORMAL", "POSITION"])
        normal = doc["accessors"][prim["attributes"]["NORMAL"]]
        assert normal["componentType"] == 5126 and normal["type"] == "VEC3" and normal["count"] == len(v)
        assert _accessor(doc, binary, prim["attributes"]["NORMAL"]).tobytes() == n.tobytes()
        assert _accessor(doc, binary, prim["attributes"]["POSITION"]).tobytes() == v.tobytes()
        assert all(view["byteOffset"] % 4 == 0 for view in doc["bufferViews"]) and doc["buffers"][0]["byteLength"] == len(binary)
        gv, gf, gc = load_glb_mesh(path, "cpu")
        assert gv.numpy().tobytes() == v.tobytes() and np.array_equal(gf.numpy(), f)
        want = colour[f[:, 0]].astype(np.float32) if col is not None else np.ones((len(f), 3), np.float32)
        assert np.array_equal(gc.numpy(), want)
    with pytest.raises(ValueError, match="vertex_normal"):
        save_glb_shaded_mesh(tmp_path / "bad.glb", v, f, n[:-1])


def test_example_refuses_smooth_mesh_without_extract_mesh():
    example = os.path.join(ROOT, "examples", "train_synthetic.py")
    r = subprocess.run([sys.executable, example, "--eval-mesh", "--smooth-mesh", "5"], capture_output=True, text=True)
    assert r.returncode == 2 and "--smooth-mesh smooths the mesh of --extract-mesh" in r.stderr
    r = subprocess.run([sys.executable, example, "--eval-mesh", "--extract-mesh", "24", "--smooth-mesh", "-1"], capture_output=True, text=True)
    assert r.returncode == 2 and "--smooth-mesh needs a number of iterations >= 0" in r.stderr
