"""CPU tests of the edge split (no GPU): the numpy reference of include/ts_subdivide.h on constructions with small even-integer coordinates,
where midpoints, squared lengths and doubled areas are exact -- every face case, the diagonal rule, closedness, Euler characteristic and
area, boundary and non-manifold edges, the faces that do not take part, the rounds; libts_subdivide.so is a library of its own with exactly
the C ABI of the header, and every argument check answers before any HIP call; view_edge_limit against a hand computation."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_subdivide as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_subdivide.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tsd_edges", "tsd_last_error", "tsd_split", "tsd_workspace_bytes"]
MAX_FACES = 536870911


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_subdivide", ("diff_triangle_rasterization_2D", "_abi.py"))


SUBDIVIDE_SIGNATURES = _abi_module().SUBDIVIDE_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def subdivide_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_subdivide.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_subdivide.so"
    return path


@pytest.fixture(scope="module")
def lib(subdivide_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_subdivide(ctypes.CDLL(subdivide_path))


def _header_prototypes():
    """name -> number of parameters of every tsd_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


def _area2(v, f):
    """The summed doubled area: exact where every cross product has a single non-zero component or small integer entries."""
    return np.sqrt((ref.doubled_area_vectors(v, f) ** 2).sum(1)).sum()


def _edge_use(V, f, keep=None):
    t = ref.edges(V, f, keep)
    return {tuple(e): int(u) for e, u in zip(t["edge_vertices"][:t["E"]].tolist(), t["edge_use"][:t["E"]])}


# ---- the face cases -----------------------------------------------------------------------------------------------------------------------------
TRI = np.array([[0, 0, 0], [8, 0, 0], [0, 4, 0]], np.float32)  # edges of squared length 64, 80, 16


def test_zero_marked_edges_copy_the_face():
    v, f, _, _, e, parent, totals = ref.split_mesh(TRI, [[0, 1, 2]], mode=ref.MARK_LONGER, max_edge=9.0)
    assert f.tolist() == [[0, 1, 2]] and len(v) == 3 and len(e) == 0 and parent.tolist() == [0] and totals == [3, 0, 1, 0]
    s = ref.split(TRI, [[0, 1, 2]], mode=ref.MARK_LONGER, max_edge=9.0)  # the capacity and its fill values
    assert s["out_faces"].shape == (4, 3) and (s["out_faces"][1:] == -1).all() and (s["out_face_parent"][1:] == -1).all()
    assert s["new_vertices"].shape == (3, 3) and not s["new_vertices"].any() and (s["new_vertex_edge"] == -1).all()


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_one_marked_edge_gives_two_pieces_at_any_corner(rot):
    face = np.roll([0, 1, 2], -rot)  # the edge (1, 2), the longest, sits at corner k = (1 - rot) % 3
    v, f, _, _, e, parent, totals = ref.split_mesh(TRI, [face], mode=ref.MARK_LONGER, max_edge=8.5)
    assert totals == [3, 1, 2, 1] and e.tolist() == [[1, 2]] and v[3].tolist() == [4, 2, 0] and parent.tolist() == [0, 0]
    k = (1 - rot) % 3
    a, b, c = face[k], face[(k + 1) % 3], face[(k + 2) % 3]
    assert (a, b, c) == (1, 2, 0) and f.tolist() == [[a, 3, c], [3, b, c]]
    assert np.array_equal(ref.doubled_area_vectors(v, f).sum(0), ref.doubled_area_vectors(TRI, [face]).sum(0))  # orientation and area kept


def test_two_marked_edges_cut_the_quad_by_its_shorter_diagonal_both_ways():
    # edges (0,1) len2 64 and (1,2) len2 80 marked, (0,2) len2 16 not: the unmarked corner k is 2: a = 2, b = 0, c = 1
    v, f, _, _, e, parent, totals = ref.split_mesh(TRI, [[0, 1, 2]], mode=ref.MARK_LONGER, max_edge=5.0)
    assert totals == [3, 2, 3, 1] and e.tolist() == [[0, 1], [1, 2]] and v[3:].tolist() == [[4, 0, 0], [4, 2, 0]]
    a, b, c, m1, m2 = 2, 0, 1, 3, 4  # m1 on (b, c) = (0, 1), m2 on (c, a) = (1, 2)
    d1, d2 = ref.squared_length(v[a], v[m1]), ref.squared_length(v[b], v[m2])
    assert (d1, d2) == (32.0, 20.0)  # b-m2 is shorter
    assert f.tolist() == [[m1, c, m2], [a, b, m2], [b, m1, m2]] and parent.tolist() == [0, 0, 0]
    # the mirror image: a-m1 strictly shorter
    tri = np.array([[0, 0, 0], [4, 0, 0], [0, 8, 0]], np.float32)  # (0,1) 16, (1,2) 80, (0,2) 64: unmarked corner 0: a = 0, b = 1, c = 2
    v, f, _, _, e, _, totals = ref.split_mesh(tri, [[0, 1, 2]], mode=ref.MARK_LONGER, max_edge=5.0)
    assert e.tolist() == [[0, 2], [1, 2]] and v[3:].tolist() == [[0, 4, 0], [2, 4, 0]]
    a, b, c, m1, m2 = 0, 1, 2, 4, 3  # m1 on (1, 2), m2 on (2, 0)
    assert (ref.squared_length(v[a], v[m1]), ref.squared_length(v[b], v[m2])) == (20.0, 32.0)
    assert f.tolist() == [[m1, c, m2], [a, b, m1], [a, m1, m2]]
    assert np.array_equal(ref.doubled_area_vectors(v, f).sum(0), ref.doubled_area_vectors(tri, [[0, 1, 2]]).sum(0))


def test_the_diagonal_tie_goes_to_the_smaller_index():
    tri = np.array([[-4, 0, 0], [4, 0, 0], [0, 8, 0]], np.float32)  # isosceles: both diagonals have squared length 36 + 16 = 52
    for face, want_first in (([0, 1, 2], True), ([1, 0, 2], False)):
        limit = np.array([100, 100, 1], np.float32)  # min(limit) marks the two edges at vertex 2, not (0, 1)
        v, f, _, _, e, _, totals = ref.split_mesh(tri, [face], mode=ref.MARK_VERTEX_LIMIT, vertex_limit=limit)
        assert totals == [3, 2, 3, 1] and e.tolist() == [[0, 2], [1, 2]]
        a, b, c = face
        mid = {0: 3, 1: 4}
        m1, m2 = mid[b], mid[a]  # m1 on (b, c), m2 on (c, a)
        assert ref.squared_length(v[a], v[m1]) == ref.squared_length(v[b], v[m2]) == 52.0
        assert (a < b) == want_first
        assert f.tolist() == ([[m1, c, m2], [a, b, m1], [a, m1, m2]] if want_first else [[m1, c, m2], [a, b, m2], [b, m1, m2]])


def test_three_marked_edges_give_four_pieces_in_order():
    v, f, _, _, e, parent, totals = ref.split_mesh(TRI, [[0, 1, 2]])
    assert totals == [3, 3, 4, 1] and e.tolist() == [[0, 1], [0, 2], [1, 2]] and v[3:].tolist() == [[4, 0, 0], [0, 2, 0], [4, 2, 0]]
    m0, m1, m2 = 3, 5, 4  # on half-edges (0,1), (1,2), (2,0)
    assert f.tolist() == [[0, m0, m2], [m0, 1, m1], [m2, m1, 2], [m0, m1, m2]] and parent.tolist() == [0] * 4
    assert (ref.doubled_area_vectors(v, f) == [0, 0, 8]).all()  # four congruent pieces, the parent's orientation


# ---- whole meshes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,kw", [(ref.MARK_ALL, {}), (ref.MARK_LONGER, {"max_edge": 4.5}), (ref.MARK_LONGER, {"max_edge": 5.7})])
def test_a_closed_cube_grid_stays_closed_and_keeps_its_euler_characteristic_and_area(mode, kw):
    v, f = ref.cube_grid(2, 4)
    assert len(f) == 48 and ref.euler(len(v), f) == 2 and set(_edge_use(len(v), f).values()) == {2}
    v2, f2, _, _, e, parent, totals = ref.split_mesh(v, f, mode=mode, **kw)
    assert totals[1] == {0: 72, 4.5: 24, 5.7: 0}[kw.get("max_edge", 0)]  # all edges; the face diagonals (32 > 20.25); none (32 < 32.49)
    assert set(_edge_use(len(v2), f2).values()) == {2} and ref.euler(len(v2), f2) == 2
    assert _area2(v2, f2) == _area2(v, f) == 2 * 6 * 64.0
    assert np.array_equal(ref.doubled_area_vectors(v2, f2).sum(0), [0, 0, 0])
    # every piece has its parent's normal direction, and the parents' areas are the sums of their pieces'
    n2, n = ref.doubled_area_vectors(v2, f2), ref.doubled_area_vectors(v, f)
    assert np.array_equal(np.sign(n2), np.sign(n[parent]))
    assert np.array_equal(np.add.reduceat(n2, np.nonzero(np.r_[True, parent[1:] != parent[:-1]])[0]), n)
    assert (np.diff(parent) >= 0).all() and len(f2) == totals[2] == len(f) + {0: 3 * 48, 4.5: 48, 5.7: 0}[kw.get("max_edge", 0)]
    # no output vertex lies inside an output edge: every new vertex is an end of edges only, and each halved edge is gone
    gone = {tuple(x) for x in e.tolist()}
    assert not gone & set(_edge_use(len(v2), f2))


def test_a_boundary_edge_becomes_two_boundary_edges():
    v = np.array([[0, 0, 0], [8, 0, 0], [8, 8, 0], [0, 8, 0]], np.float32)
    f = [[0, 1, 2], [0, 2, 3]]
    before = _edge_use(4, f)
    assert sorted(before.values()) == [1, 1, 1, 1, 2]
    v2, f2, _, _, e, _, totals = ref.split_mesh(v, f)
    after = _edge_use(len(v2), f2)
    assert totals == [5, 5, 8, 2] and sorted(after.values()) == [1] * 8 + [2] * 8
    for (lo, hi), m in zip(e.tolist(), range(4, 9)):
        assert after[(lo, m)] == after[(hi, m)] == before[(lo, hi)]  # both halves keep the use count


def test_a_nonmanifold_edge_keeps_its_use_count_on_both_halves():
    v = np.array([[0, 0, 0], [16, 0, 0], [0, 8, 0], [0, -8, 0], [0, 0, 8]], np.float32)
    f = [[0, 1, 2], [1, 0, 3], [0, 1, 4]]  # a book of three pages on the spine (0, 1)
    t = ref.edges(5, f, vertices=v)
    assert t["counts"] == [7, 6, 0, 1] and t["edge_use"][0] == 3 and t["edge_length2"][0] == 256.0
    v2, f2, _, _, e, _, totals = ref.split_mesh(v, f, mode=ref.MARK_LONGER, max_edge=16.0)  # the pages' hypotenuses (320 > 256): not the spine
    assert totals[1] == 3 and [0, 1] not in e.tolist()
    v2, f2, _, _, e, _, totals = ref.split_mesh(v, f, mode=ref.MARK_VERTEX_LIMIT, vertex_limit=np.array([15, 100, 100, 100, 100], np.float32))  # 16 > 15
    assert e.tolist() == [[0, 1]] and totals == [7, 1, 6, 3]
    after = _edge_use(len(v2), f2)
    assert after[(0, 5)] == after[(1, 5)] == 3 and sorted(after.values()).count(3) == 2


def test_masked_degenerate_and_out_of_range_faces_are_copied_and_keep_their_long_edge():
    v = np.array([[0, 0, 0], [8, 0, 0], [8, 8, 0], [0, 8, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 2, 2], [0, 2, 4], [-1, 0, 2], [2, 0, 1]])
    keep = np.array([1, 0, 1, 1, 1, 0], np.uint8)
    assert ref.participation(4, f, keep).tolist() == [True, False, False, False, False, False]
    s = ref.split(v, f, keep)
    assert s["totals"] == [3, 3, 4 + 5, 1] and s["table"]["half_edge_edge"].tolist() == [0, 2, 1] + [-1] * 15
    assert np.array_equal(s["out_faces"][4:9], f[1:]) and s["out_face_parent"][:9].tolist() == [0, 0, 0, 0, 1, 2, 3, 4, 5]
    # the masked neighbour (0, 2, 3) keeps the edge (0, 2) whose midpoint now exists: the T-junction the header states
    assert s["new_vertex_edge"][:3].tolist() == [[0, 1], [0, 2], [1, 2]]


def test_non_finite_vertices_are_never_marked_and_their_length_is_the_stated_nan():
    v = np.array([[0, 0, 0], [8, 0, 0], [8, 8, 0], [0, 8, 0], [4, 4, np.inf], [np.nan, 0, 0]], np.float32)
    f = [[0, 1, 2], [0, 2, 3], [0, 2, 4], [1, 5, 2]]
    t = ref.edges(6, f, vertices=v)
    bad = [i for i, e in enumerate(t["edge_vertices"][:t["E"]].tolist()) if 4 in e or 5 in e]
    assert len(bad) == 4 and (t["edge_length2"][bad].view(np.uint64) == 0x7FF8000000000000).all() and not t["finite"][bad].any()
    for mode, kw in ((ref.MARK_ALL, {}), (ref.MARK_LONGER, {"max_edge": 0.0}), (ref.MARK_VERTEX_LIMIT, {"vertex_limit": np.zeros(6, np.float32)})):
        s = ref.split(v, f, mode=mode, **kw)
        assert s["totals"][1] == 5 and np.isfinite(s["new_vertices"]).all()
        assert s["out_faces"][s["out_face_parent"] == 2].tolist() == [[0, 6 + 1, 4], [6 + 1, 2, 4]]  # only (0, 2) of the face at infinity
    nan_limit = np.array([0, np.nan, 0, 0, 0, 0], np.float32)  # a NaN limit: the edges at vertex 1 are not marked
    e = ref.split(v, f, mode=ref.MARK_VERTEX_LIMIT, vertex_limit=nan_limit)
    assert e["totals"][1] == 3 and not (e["new_vertex_edge"][:3] == 1).any()
    z = np.array([[0, 0, 0], [0, 0, 0], [8, 0, 0]], np.float32)  # a zero-length edge: never longer than anything
    assert ref.split(z, [[0, 1, 2]], mode=ref.MARK_LONGER, max_edge=0.0)["new_vertex_edge"][:3].tolist() == [[0, 2], [1, 2], [-1, -1]]
    assert ref.split(z, [[0, 1, 2]])["totals"][1] == 3  # but every finite edge is marked by TSD_MARK_ALL


def test_attributes_follow_the_validity_of_the_ends():
    v = np.array([[0, 0, 0], [8, 0, 0], [0, 8, 0]], np.float32)
    a = np.array([[2, 10], [4, 20], [8, 40]], np.float32)
    s = ref.split(v, [[0, 1, 2]], attributes=a, attr_valid=[1, 0, 0])
    assert s["new_vertex_edge"][:3].tolist() == [[0, 1], [0, 2], [1, 2]]
    assert s["new_attributes"][:3].tolist() == [[2, 10], [2, 10], [0, 0]] and s["new_attr_valid"][:3].tolist() == [1, 1, 0]
    s = ref.split(v, [[0, 1, 2]], attributes=a)
    assert s["new_attributes"][:3].tolist() == [[3, 15], [5, 25], [6, 30]] and s["new_attr_valid"][:3].tolist() == [1, 1, 1]
    assert ref.split(v, [[0, 1, 2]])["new_attributes"] is None


def test_rounds_end_with_no_edge_above_the_limit_and_face_parent_composes():
    v, f = ref.cube_grid(1, 16)  # edges of 16 and diagonals of 16 sqrt 2
    colour = np.arange(len(f), dtype=np.float32)
    out = ref.split_rounds(v, f, 16, max_edge=5.0)
    assert out["converged"] and out["rounds"] == 3  # 22.6 -> 11.3 -> 5.7 -> 2.8
    t = ref.edges(len(out["vertices"]), out["faces"], vertices=out["vertices"])
    assert t["edge_length2"][:t["E"]].max() <= 25.0 and set(t["edge_use"][:t["E"]].tolist()) == {2}
    assert ref.euler(len(out["vertices"]), out["faces"]) == 2 and _area2(out["vertices"], out["faces"]) == 2 * 6 * 256.0
    # every piece lies in its ORIGINAL parent's plane and winds its way
    n, n0 = ref.doubled_area_vectors(out["vertices"], out["faces"]), ref.doubled_area_vectors(v, f)
    parent = out["face_parent"]
    assert np.array_equal(np.sign(n), np.sign(n0[parent])) and np.array_equal(np.bincount(parent, weights=np.abs(n).sum(1)), np.abs(n0).sum(1))
    assert np.array_equal(colour[parent][:3], [0, 0, 0]) and (np.diff(parent) >= 0).all()
    assert out["vertex_edge"][:len(v)].tolist() == [[-1, -1]] * len(v) and (out["vertex_edge"][len(v):] >= 0).all()
    assert (out["vertex_edge"][len(v):].max(1) < np.arange(len(v), len(out["vertices"]))).all()  # a new vertex halves an edge of older vertices
    short = ref.split_rounds(v, f, 2, max_edge=5.0)
    assert not short["converged"] and short["rounds"] == 2
    levels = ref.split_rounds(v, f, 2)
    assert len(levels["faces"]) == 16 * len(f) and levels["rounds"] == 2 and not levels["converged"]
    # a per-vertex limit is interpolated: the far half of the cube stays coarse
    limit = np.where(v[:, 0] == 0, 5.0, 100.0).astype(np.float32)
    part = ref.split_rounds(v, f, 16, vertex_limit=limit)
    assert part["converged"] and len(f) < len(part["faces"]) < len(out["faces"]) and len(part["limit"]) == len(part["vertices"])
    t = ref.edges(len(part["vertices"]), part["faces"], vertices=part["vertices"])
    ends = t["edge_vertices"][:t["E"]]
    assert (t["edge_length2"][:t["E"]] <= np.minimum(part["limit"][ends[:, 0]], part["limit"][ends[:, 1]]).astype(np.float64) ** 2).all()
    assert set(t["edge_use"][:t["E"]].tolist()) == {2}


def test_view_edge_limit_matches_a_hand_computation(subdivide_path):
    import torch
    from diff_recon_hip import mesh_subdivide
    v = torch.tensor([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [0.0, 0.0, 10.0]])
    centers = torch.tensor([[0.0, 0.0, 5.0], [3.0, 4.0, 12.0]])
    got = mesh_subdivide.view_edge_limit(v, centers, 100.0, 2.0)
    assert got.dtype == torch.float32 and got.tolist() == pytest.approx([2 * 5 / 100, 2 * np.sqrt(50) / 100, 2 * 5 / 100], rel=1e-6)
    got = mesh_subdivide.view_edge_limit(v, centers, torch.tensor([100.0, 300.0]), 2.0)  # per-view focal lengths: the second view is "nearer"
    assert got.tolist() == pytest.approx([2 * 13 / 300, 2 * 12 / 300, 2 * np.sqrt(29) / 300], rel=1e-6)
    assert np.allclose(got.numpy(), ref.view_edge_limit(v.numpy(), centers.numpy(), [100.0, 300.0], 2.0), rtol=1e-6)
    with pytest.raises(ValueError):
        mesh_subdivide.view_edge_limit(v, centers, 100.0, 0.0)


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(subdivide_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsd_last_error.restype = ctypes.c_char_p; "
            "l.tsd_workspace_bytes.restype = ctypes.c_size_t; print(l.tsd_workspace_bytes(100000, 200000) >= 20 * 3 * 200000, "
            "repr(l.tsd_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, subdivide_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(subdivide_path):
    out = subprocess.run(["nm", "-D", "--defined-only", subdivide_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES and len(NAMES) == 4
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", subdivide_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", subdivide_path], capture_output=True, text=True).stdout
    assert "libts_subdivide.so" in dynamic
    for other in ("libts2d.so", "libts_smooth.so", "libts_holes.so", "libts_manifold.so", "libts_orient.so", "libts_overlap.so"):
        assert other not in dynamic


def test_header_defines_no_struct_and_states_the_contract():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsv|tsc|tsq|tss|tsh|tsf|tsw|tsa|tsi|tsn|tsx)_[a-z0-9_]+)\s*\(", text)  # a prefix of its own
    assert "struct" not in text
    assert re.findall(r"#define (TSD_MARK_\w+) (\d)", text) == [("TSD_MARK_ALL", "0"), ("TSD_MARK_LONGER", "1"), ("TSD_MARK_VERTEX_LIMIT", "2")]
    full = open(HEADER).read()
    for word in ("TAKES PART", "ascending (lo, hi)", "(dx dx + dy dy) + dz dz", "0x7FF8000000000000", "FINITE", "zero-length edge is never marked",
                 "rank of the edge among the marked edges", "(float)((p_lo + p_hi) 0.5)", "exactly one end", "bit for bit", "shorter diagonal",
                 "a < b as indices", "(m0, m1, m2)", "parent's orientation", "conforming", "KEEPS its long edge", "T-junction", "to their capacity",
                 "{edges, marked, out_faces, faces_split}", "half of tss_adjacency's", "before any HIP call", "536870911", "2147483647", "Monotonic",
                 "nobody waits for anybody", "Purity"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(SUBDIVIDE_SIGNATURES) and len(declared) == 4
    for name, arity in declared.items():
        assert len(SUBDIVIDE_SIGNATURES[name][1]) == arity, name
    assert declared["tsd_edges"] == 13 and declared["tsd_split"] == 21
    abi = _abi_module()
    tables = [getattr(abi, n) for n in dir(abi) if n.endswith("SIGNATURES")]
    assert len(tables) >= 17 and abi.SUBDIVIDE_SIGNATURES in tables
    for a in range(len(tables)):
        for b in range(a + 1, len(tables)):
            assert not set(tables[a]) & set(tables[b])  # no signature table overlaps another
    assert SUBDIVIDE_SIGNATURES["tsd_edges"][1][11] == ctypes.c_size_t and SUBDIVIDE_SIGNATURES["tsd_split"][1][19] == ctypes.c_size_t
    assert SUBDIVIDE_SIGNATURES["tsd_split"][1][6] == ctypes.c_float and SUBDIVIDE_SIGNATURES["tsd_workspace_bytes"][0] == ctypes.c_size_t
    # the prefix is this library's alone
    for path in (os.path.join(ROOT, "include"), os.path.join(ROOT, "triangle-splatting_amd", "csrc")):
        for name in os.listdir(path):
            if "subdivide" not in name:
                assert not re.search(r"\btsd_", open(os.path.join(path, name)).read()), name


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_subdivide", ("build.py",))
    assert build.SUBDIVIDE_SOURCES == {"mesh_subdivide.hip": ["-ffp-contract=off"], "api_subdivide.hip": []} and build.SUBDIVIDE_SHARED == ["radix_sort"]
    assert build.subdivide_units() == ["mesh_subdivide", "api_subdivide"]
    cmd = build.subdivide_command("mesh_subdivide", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert "-ffp-contract=off" not in build.subdivide_command("api_subdivide")
    assert build.subdivide_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_subdivide", "api_subdivide", "radix_sort")]
    for others in (build.units(), build.smooth_units(), build.holes_units(), build.manifold_units(), build.orient_units(), build.overlap_units()):
        assert not {"mesh_subdivide", "api_subdivide"} & set(others)  # its own library only
    assert build.SUBDIVIDE_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_subdivide.so")
    for header in ("ts_subdivide_launch.h", "ts_mesh_edges.h", "ts_mesh_scan.h", os.path.join("..", "..", "include", "ts_subdivide.h")):
        assert header in build.HEADERS
    with pytest.raises(ValueError):
        build.subdivide_command("mesh_holes")


def test_built_objects_carry_the_flags_and_the_unit_uses_the_shared_front(subdivide_path):
    build = _load("ts2d_build_subdivide2", ("build.py",))
    for unit in ("mesh_subdivide", "api_subdivide"):
        stamp = open(os.path.join(build.OBJ_DIR, unit + ".o.cmd")).read()  # what the object on disk was compiled with
        assert stamp.endswith(" ".join(build.subdivide_command(unit, cc=stamp.splitlines()[1].split()[0])))
        assert ("-ffp-contract=off" in stamp) == (unit == "mesh_subdivide")
    link = open(build.SUBDIVIDE_LIB + ".cmd").read()
    assert "-soname,libts_subdivide.so" in link and "radix_sort.o" in link and "mesh_manifold" not in link
    text = open(os.path.join(build.CSRC, "mesh_subdivide.hip")).read()
    assert '#include "ts_mesh_edges.h"' in text and '#include "ts_mesh_scan.h"' in text
    for used in ("half_edge_records(", "sort_half_edges(", "edge_run_head(", "scan_columns<1>(", "block_scan256(", "face_takes_part("):
        assert used in text, used
    assert "atomicAdd(" not in text and "float atomic" not in text  # the counters go through count_into / count4_into: integer adds


def test_size_query_is_monotone_in_both_counts(lib):
    sizes = (0, 1, 2, 63, 682, 683, 1024, 1025, 4097, 100000, 416666, 416667, 833333, 833334, 2499999, 2500000, 2500001, 2600000, 5000000)
    for fixed in (0, 1000, 3000000):
        prev_v = prev_f = -1
        for n in sizes:
            by_v, by_f = lib.tsd_workspace_bytes(n, fixed), lib.tsd_workspace_bytes(fixed, n)
            assert by_v >= prev_v and by_f >= prev_f, (n, fixed)
            assert by_f >= 4 * 13 * 3 * n  # five words of the sort and eight of the table per half-edge
            prev_v, prev_f = by_v, by_f
    assert lib.tsd_workspace_bytes(-5, -5) == lib.tsd_workspace_bytes(0, 0)
    assert lib.tsd_workspace_bytes(10, 2 ** 31 - 1) == lib.tsd_workspace_bytes(10, MAX_FACES)


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    big = 1 << 40

    def refused(rc, word, code=INVALID):
        assert rc == code, rc
        text = lib.tsd_last_error()
        assert text and word.encode() in text, text

    def edges(V=10, F=20, vertices=P, faces=P, keep=None, ev=P, use=P, length2=P, hee=P, counts=P, ws=P, ws_bytes=big):
        return lib.tsd_edges(V, F, vertices, faces, keep, ev, use, length2, hee, counts, ws, ws_bytes, None)

    def split(V=10, F=20, vertices=P, faces=P, keep=None, mode=0, max_edge=1.0, limit=None, attrs=None, valid=None, channels=0, nv=P, na=None,
              nvalid=None, nedge=P, out_faces=P, parent=P, totals=P, ws=P, ws_bytes=big):
        return lib.tsd_split(V, F, vertices, faces, keep, mode, max_edge, limit, attrs, valid, channels, nv, na, nvalid, nedge, out_faces, parent,
                             totals, ws, ws_bytes, None)

    for call in (edges, split):
        refused(call(V=-1), ">= 0")
        refused(call(V=-(2 ** 31)), ">= 0")
        refused(call(F=-1), ">= 0")
        refused(call(F=-(2 ** 31)), ">= 0")
        refused(call(F=MAX_FACES + 1), "exceeds", CAPACITY)  # 4 F
        refused(call(F=2 ** 31 - 1), "exceeds", CAPACITY)
        refused(call(V=2 ** 31 - 1, F=1), "V + 3 F", CAPACITY)
        refused(call(V=2 ** 31 - 1 - 3 * 1000 + 1, F=1000), "V + 3 F", CAPACITY)
        refused(call(ws=None), "workspace is null")
        refused(call(faces=None), "null")
        refused(call(vertices=None), "vertices is null")
    for name in ("counts", "ev", "use", "hee"):
        refused(edges(**{name: None}), "null")
    for name in ("totals", "nv", "nedge", "out_faces", "parent"):
        refused(split(**{name: None}), "null")
    for mode in (-1, 3, 2 ** 31 - 1):
        refused(split(mode=mode), "mode")
    for bad in (-1.0, float("nan"), -float("inf")):
        refused(split(mode=1, max_edge=bad), "max_edge")
    refused(split(mode=2), "vertex_limit is null")
    refused(split(channels=-1), "channels")
    refused(split(channels=3, attrs=P, na=None, nvalid=P), "new_attributes")
    refused(split(channels=3, attrs=P, na=P, nvalid=None), "new_attributes")
    refused(split(channels=3, attrs=None, na=P, nvalid=P), "attributes is null")
    need = lib.tsd_workspace_bytes(1000, 2000)
    refused(edges(V=1000, F=2000, ws_bytes=need - 1), "workspace too small")
    assert str(need).encode() in lib.tsd_last_error()
    refused(split(V=1000, F=2000, ws_bytes=need - 1), "workspace too small")
    # what the checks accept, for the record: keep, attr_valid and edge_length2 (then vertices too) may be null, max_edge is not looked at
    # outside TSD_MARK_LONGER, and nothing but counts / totals is needed with F == 0 (those calls would reach the device, so they are made
    # in tests/test_mesh_subdivide_gpu.py)


def test_package_re_exports_the_feature(subdivide_path):
    import inspect

    import torch

    import diff_recon_hip
    from diff_recon_hip import mesh_subdivide
    names = ("MARK_ALL", "MARK_LONGER", "MARK_VERTEX_LIMIT", "MeshEdges", "SplitMesh", "mesh_edges", "split_edges", "split_long_edges", "subdivide_mesh",
             "view_edge_limit", "split_fused")
    assert diff_recon_hip._SUBDIVIDE_NAMES == names
    for name in names:
        assert getattr(diff_recon_hip, name) is getattr(mesh_subdivide, name)
    assert diff_recon_hip.mesh_subdivide is mesh_subdivide
    params = lambda fn: list(inspect.signature(fn).parameters)
    assert params(mesh_subdivide.mesh_edges) == ["num_vertices", "faces", "keep", "vertices"]
    common = ["vertex_attributes", "attribute_valid", "keep", "face_attributes"]
    assert params(mesh_subdivide.split_edges) == ["vertices", "faces", "max_edge", "vertex_limit"] + common
    assert params(mesh_subdivide.split_long_edges) == ["vertices", "faces", "max_edge", "vertex_limit"] + common + ["max_rounds"]
    assert inspect.signature(mesh_subdivide.split_long_edges).parameters["max_rounds"].default == 16
    assert params(mesh_subdivide.subdivide_mesh) == ["vertices", "faces", "levels"] + common
    assert params(mesh_subdivide.view_edge_limit) == ["vertices", "camera_centers", "focal_pixels", "max_pixels"]
    assert params(mesh_subdivide.split_fused) == ["mesh", "max_edge"]
    assert mesh_subdivide.MeshEdges._fields == ("edge_vertices", "edge_use", "length", "half_edge_edge", "stats")
    assert mesh_subdivide.SplitMesh._fields == ("vertices", "faces", "vertex_attributes", "attribute_valid", "new_vertex", "vertex_edge", "face_parent",
                                                "face_attributes", "stats")
    assert mesh_subdivide.COUNT_NAMES == ref.COUNT_NAMES and mesh_subdivide.TOTAL_NAMES == ref.TOTAL_NAMES
    assert (mesh_subdivide.MARK_ALL, mesh_subdivide.MARK_LONGER, mesh_subdivide.MARK_VERTEX_LIMIT) == (ref.MARK_ALL, ref.MARK_LONGER, ref.MARK_VERTEX_LIMIT)
    f = torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_subdivide.mesh_edges(4, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_subdivide.split_edges(torch.zeros((4, 3)), f)
    with pytest.raises(ValueError, match="not both"):
        mesh_subdivide.split_edges(torch.zeros((4, 3)), f, max_edge=1.0, vertex_limit=torch.zeros(4))
    with pytest.raises(ValueError, match="max_edge or vertex_limit"):
        mesh_subdivide.split_long_edges(torch.zeros((4, 3)), f)
    with pytest.raises(ValueError, match="num_vertices"):
        mesh_subdivide.mesh_edges(-1, f)


def test_example_refuses_split_edges_without_weld_mesh():
    example = os.path.join(ROOT, "examples", "train_synthetic.py")
    r = subprocess.run([sys.executable, example, "--eval-mesh", "--split-edges", "0.1"], capture_output=True, text=True)
    assert r.returncode == 2 and "--split-edges splits the welded mesh of --weld-mesh" in r.stderr
