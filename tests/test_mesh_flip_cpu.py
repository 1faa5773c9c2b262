"""CPU tests of the edge flip (no GPU): the numpy reference of include/ts_flip.h on hand constructions with small even-integer coordinates,
where every product of the criterion is exact -- both diagonals of a quad, the cocircular square, the cap, the guards, the duplicate rule,
the edges that are not eligible, the faces that do not take part; convergence to the unique Delaunay triangulation of ~100 integer points,
checked by the exact in-circle determinant; libts_flip.so is a library of its own with exactly the C ABI of the header, and every argument
check answers before any HIP call."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_flip as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_flip.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tse_flip", "tse_last_error", "tse_workspace_bytes"]
MAX_FACES = 536870911
COS_180, COS_30 = ref.min_cos_of(180.0), ref.min_cos_of(30.0)


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_flip", ("diff_triangle_rasterization_2D", "_abi.py"))


FLIP_SIGNATURES = _abi_module().FLIP_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def flip_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_flip.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_flip.so"
    return path


@pytest.fixture(scope="module")
def lib(flip_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_flip(ctypes.CDLL(flip_path))


def _header_prototypes():
    """name -> number of parameters of every tse_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tse_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


def _states(o):
    """{(lo, hi): state} of the round's edge table."""
    E = o["E"]
    return {tuple(e): int(s) for e, s in zip(o["edge_vertices"][:E].tolist(), o["edge_state"][:E])}


def _fills(o):
    """The capacity beyond E holds the fill values, and everything has its shape."""
    E, F = o["E"], len(o["out_faces"])
    assert o["edge_vertices"].shape == (3 * F, 2) and o["edge_state"].shape == (3 * F,) and o["edge_opposite"].shape == (3 * F, 2)
    assert (o["edge_vertices"][E:] == -1).all() and (o["edge_state"][E:] == ref.NO_EDGE).all() and (o["edge_opposite"][E:] == -1).all()
    assert o["totals"][0] == E


# ---- one quad ---------------------------------------------------------------------------------------------------------------------------------
#   A = (-8, 0), B = (8, 0), C = (0, 2), D = (0, -2): the diagonal A-B is long, the angles at C and D are obtuse
QUAD = np.array([[-8, 0, 0], [8, 0, 0], [0, 2, 0], [0, -2, 0]], np.float32)
LONG = [[0, 1, 2], [1, 0, 3]]   # cut by A-B
SHORT = [[2, 3, 1], [3, 2, 0]]  # cut by C-D


def test_long_diagonal_of_a_quad_flips_and_keeps_the_orientation():
    o = ref.flip_round(QUAD, LONG, min_cos=COS_30)
    _fills(o)
    assert o["totals"] == [5, 1, 1, 1] and o["face_flipped"].tolist() == [1, 1]
    assert o["out_faces"].tolist() == [[0, 3, 2], [3, 1, 2]]  # (a, d, c), (d, b, c)
    s = _states(o)
    assert s[(0, 1)] == ref.FLIPPED and o["edge_opposite"][0].tolist() == [2, 3]
    for e in ((0, 2), (0, 3), (1, 2), (1, 3)):  # boundary edges: use 1
        assert s[e] == ref.NOT_ELIGIBLE
    assert (o["edge_opposite"][1:5] == -1).all()
    for f in o["out_faces"]:  # counter-clockwise as before: doubled area > 0, and the two sum to the quad's 64
        p, q, r = QUAD[f]
        assert (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0]) == 32
    # the criterion by hand: at C u = (-8, -2), v = (8, -2), A = -60, P = 32^2; the same at D
    assert ref.wants_flip(QUAD[[0]].astype(float), QUAD[[1]].astype(float), QUAD[[2]].astype(float), QUAD[[3]].astype(float))[0]


def test_short_diagonal_of_the_quad_stays_and_a_second_round_changes_nothing():
    o = ref.flip_round(QUAD, SHORT, min_cos=COS_30)
    assert o["totals"] == [5, 0, 0, 0] and _states(o)[(2, 3)] == ref.DELAUNAY and o["out_faces"].tolist() == SHORT
    assert o["edge_opposite"][4].tolist() == [1, 0]  # edge (2, 3): 2 -> 3 runs in face 0, opposite vertex 1
    once = ref.flip_round(QUAD, LONG)["out_faces"]
    again = ref.flip_round(QUAD, once)
    assert again["totals"] == [5, 0, 0, 0] and again["out_faces"].tolist() == once.tolist()
    f, per_round, converged, union = ref.delaunay_flips(QUAD, LONG)
    assert converged and per_round == [[5, 1, 1, 1]] and union.tolist() == [True, True] and f.tolist() == once.tolist()


def test_the_rotation_of_the_faces_does_not_matter():
    for r0 in range(3):
        for r1 in range(3):
            faces = [np.roll(LONG[0], r0).tolist(), np.roll(LONG[1], r1).tolist()]
            assert ref.flip_round(QUAD, faces)["out_faces"].tolist() == [[0, 3, 2], [3, 1, 2]]
    swapped = ref.flip_round(QUAD, [LONG[1], LONG[0]])  # f0 is the face where the half-edge runs lo -> hi: slot 1 now
    assert swapped["out_faces"].tolist() == [[3, 1, 2], [0, 3, 2]]


def test_a_cocircular_square_is_not_flipped():
    v = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]], np.float32)
    for faces, diagonal in (([[0, 1, 2], [0, 2, 3]], (0, 2)), ([[0, 1, 3], [1, 2, 3]], (1, 3))):
        o = ref.flip_round(v, faces)
        assert o["totals"] == [5, 0, 0, 0] and _states(o)[diagonal] == ref.DELAUNAY and o["out_faces"].tolist() == faces


def test_a_cap_with_its_apex_on_the_edge_is_flipped_away():
    v = np.array([[0, 0, 0], [8, 0, 0], [4, 0, 0], [4, -4, 0]], np.float32)  # c = (4, 0) lies on a-b: face 0 has no area
    o = ref.flip_round(v, [[0, 1, 2], [1, 0, 3]], min_cos=COS_30)
    assert o["totals"] == [5, 1, 1, 1] and o["out_faces"].tolist() == [[0, 3, 2], [3, 1, 2]]
    for f in o["out_faces"]:  # both new faces have area 8
        p, q, r = v[f]
        assert (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0]) == 16
    assert ref.flip_round(v, o["out_faces"])["totals"] == [5, 0, 0, 0]


# ---- the guards ---------------------------------------------------------------------------------------------------------------------------
def test_flattened_tetrahedron_the_new_edge_exists():
    faces = [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]  # closed: all six pairs of the four vertices are edges
    o = ref.flip_round(QUAD, faces, min_cos=COS_180)
    assert o["E"] == 6 and o["totals"][1] >= 1 and o["totals"][2:] == [0, 0]
    s = _states(o)
    assert s[(0, 1)] == ref.GUARDED and o["edge_opposite"][0].tolist() == [2, 3]  # guard (i) alone: (2, 3) is in the table
    assert o["out_faces"].tolist() == faces and not o["face_flipped"].any()
    a, b, c, d = (QUAD[[i]].astype(float) for i in range(4))
    assert not ref.wants_flip(c, d, a, b)[0] and ref.flat_and_unfolded(a, b, c, d, COS_180)[0]


def test_two_quads_over_one_vertex_pair_only_the_smaller_edge_flips():
    #   the quad of QUAD in the plane z = 0 and a second one in the plane x = 0 over the same C, D
    v = np.concatenate([QUAD, np.array([[0, 0, -8], [0, 0, 8]], np.float32)])
    faces = [[0, 1, 2], [1, 0, 3], [4, 5, 2], [5, 4, 3]]
    o = ref.flip_round(v, faces, min_cos=COS_30)
    s = _states(o)
    assert o["totals"] == [10, 2, 2, 1]
    assert s[(0, 1)] == ref.FLIPPED and s[(4, 5)] == ref.DUPLICATE  # both won: their faces are disjoint
    assert o["out_faces"].tolist() == [[0, 3, 2], [3, 1, 2], [4, 5, 2], [5, 4, 3]] and o["face_flipped"].tolist() == [1, 1, 0, 0]
    nxt = ref.flip_round(v, o["out_faces"], min_cos=COS_30, seed=1)  # the next round: (2, 3) exists now
    assert _states(nxt)[(4, 5)] == ref.GUARDED and nxt["totals"] == [10, 1, 0, 0]
    # with the quads listed the other way round the smaller EDGE still flips, not the first face
    o2 = ref.flip_round(v, faces[2:] + faces[:2], min_cos=COS_30)
    assert _states(o2)[(0, 1)] == ref.FLIPPED and _states(o2)[(4, 5)] == ref.DUPLICATE


def test_a_crease_is_left_alone_and_a_cube_has_nothing_to_flip():
    roof = np.array([[-8, 0, 0], [8, 0, 0], [0, 2, 0], [0, 0, -2]], np.float32)  # the faces meet at 90 degrees along A-B
    for deg, state in ((30.0, ref.GUARDED), (89.0, ref.GUARDED), (90.0, ref.FLIPPED), (180.0, ref.FLIPPED)):
        if deg == 90.0:
            continue  # cos(90 degrees) rounds to 6e-17, not 0: D = 0 fails D D >= M L by a hair, which is what the header says
        o = ref.flip_round(roof, LONG, min_cos=ref.min_cos_of(deg))
        assert _states(o)[(0, 1)] == state, deg
        assert o["totals"][1] == 1 and o["totals"][3] == (state == ref.FLIPPED)
    assert _states(ref.flip_round(roof, LONG, min_cos=np.float32(0.0)))[(0, 1)] == ref.FLIPPED  # D = 0 >= 0 and 0 >= 0
    c = np.array([[x, y, z] for z in (0, 2) for y in (0, 2) for x in (0, 2)], np.float32)
    cube = [[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]]
    o = ref.flip_round(c, cube, min_cos=COS_180)
    assert o["totals"] == [18, 0, 0, 0] and set(_states(o).values()) == {ref.DELAUNAY}  # right angles everywhere: no edge wants to flip


def test_fold_guard_on_a_non_convex_quad():
    v = np.array([[-8, 0, 0], [8, 0, 0], [0, 2, 0], [12, 4, 0]], np.float32)  # D lies on C's side of A-B: the faces overlap
    a, b, c, d = (v[[i]].astype(float) for i in range(4))
    assert ref.wants_flip(a, b, c, d)[0] and not ref.wants_flip(c, d, a, b)[0]
    # S = n0 + n1 = (0, 0, 32 - 64); m0 = (D - A) x (C - A) = (0, 0, 40 - 32): against S
    assert not ref.flat_and_unfolded(a, b, c, d, COS_180)[0]
    o = ref.flip_round(v, LONG, min_cos=COS_180)
    assert _states(o)[(0, 1)] == ref.GUARDED and o["totals"] == [5, 1, 0, 0] and o["out_faces"].tolist() == LONG


# ---- edges that are not eligible, faces that do not take part -------------------------------------------------------------------------------
def test_same_direction_pair_and_an_edge_of_use_three():
    v = np.concatenate([QUAD, np.array([[0, 0, 4]], np.float32)])
    o = ref.flip_round(v, [[0, 1, 2], [0, 1, 3]], min_cos=COS_180)  # 0 -> 1 in both faces
    assert _states(o)[(0, 1)] == ref.NOT_ELIGIBLE and o["totals"] == [5, 0, 0, 0] and (o["edge_opposite"] == -1).all()
    o = ref.flip_round(v, [[0, 1, 2], [1, 0, 3], [0, 1, 4]], min_cos=COS_180)
    assert _states(o)[(0, 1)] == ref.NOT_ELIGIBLE and o["totals"] == [7, 0, 0, 0]
    o = ref.flip_round(v, [[0, 1, 2], [1, 0, 2]], min_cos=COS_180)  # c == d: the same three vertices twice
    assert set(_states(o).values()) == {ref.NOT_ELIGIBLE} and o["totals"] == [3, 0, 0, 0]


def test_masked_out_of_range_and_non_finite():
    o = ref.flip_round(QUAD, LONG, keep=[1, 0])
    assert o["totals"] == [3, 0, 0, 0] and o["out_faces"].tolist() == LONG and set(_states(o)) == {(0, 1), (0, 2), (1, 2)}
    _fills(o)
    faces = LONG + [[0, 1, 9], [2, 2, 3], [-1, 0, 1]]  # out of range, repeated, negative: copied bit for bit, no edges of theirs
    o = ref.flip_round(QUAD, faces)
    assert o["totals"] == [5, 1, 1, 1] and o["out_faces"].tolist() == [[0, 3, 2], [3, 1, 2]] + faces[2:] and o["face_flipped"].tolist() == [1, 1, 0, 0, 0]
    for bad in (np.nan, np.inf, -np.inf):
        for vertex in range(4):
            v = QUAD.copy()
            v[vertex, 1] = bad
            o = ref.flip_round(v, LONG)
            assert _states(o)[(0, 1)] == ref.NOT_ELIGIBLE and o["totals"] == [5, 0, 0, 0] and (o["edge_opposite"] == -1).all()
    empty = ref.flip_round(np.zeros((0, 3), np.float32), LONG)  # V == 0: nothing takes part
    assert empty["totals"] == [0, 0, 0, 0] and empty["out_faces"].tolist() == LONG and (empty["edge_state"] == ref.NO_EDGE).all()
    assert ref.flip_round(QUAD, np.zeros((0, 3), np.int32))["totals"] == [0, 0, 0, 0]


def test_selection_is_an_independent_set_and_the_seed_only_picks_another_one():
    v, f = ref.stretched_grid(7, 7)
    first = ref.flip_round(v, f, seed=0)
    assert first["totals"][2] > first["totals"][3] > 0  # neighbouring candidates: somebody has to wait
    chosen = set()
    for seed in range(4):
        o = ref.flip_round(v, f, seed=seed)
        assert o["totals"][:3] == first["totals"][:3]
        assert ((o["edge_state"] >= ref.LOST) == (first["edge_state"] >= ref.LOST)).all()  # the same candidates
        assert o["face_flipped"].sum() == 2 * o["totals"][3]  # winners share no face
        chosen.add(o["edge_state"].tobytes())
    assert len(chosen) > 1
    # the mixer of the header, by hand for one input: uint32 arithmetic
    h = (3 * 0x9E3779B1 + 5) & 0xFFFFFFFF
    h ^= h >> 16; h = (h * 0x85EBCA6B) & 0xFFFFFFFF; h ^= h >> 13; h = (h + 7) & 0xFFFFFFFF; h = (h * 0xC2B2AE35) & 0xFFFFFFFF; h ^= h >> 16
    assert int(ref.priority([5], [7], 3)[0]) == h


# ---- convergence against an independent fact ---------------------------------------------------------------------------------------------
def _incircle(pa, pb, pc, pd):
    """> 0 iff pd lies strictly inside the circle through the counter-clockwise pa, pb, pc: the 3 x 3 determinant in Python integers."""
    m = [[int(p[0]) - int(pd[0]), int(p[1]) - int(pd[1])] for p in (pa, pb, pc)]
    m = [[r[0], r[1], r[0] * r[0] + r[1] * r[1]] for r in m]
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def _doubled_areas(v, f):
    p = v.astype(np.int64)
    return [int((p[t[1]][0] - p[t[0]][0]) * (p[t[2]][1] - p[t[0]][1]) - (p[t[1]][1] - p[t[0]][1]) * (p[t[2]][0] - p[t[0]][0])) for t in f]


def _use_counts(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return sorted(np.unique(e, axis=0, return_counts=True)[1].tolist())


def test_flips_converge_to_the_delaunay_triangulation_of_integer_points():
    """99 points of a sheared 11 x 9 grid, spacing 3 x 7, jittered by 1, |coordinate| <= 28: every difference is below 2^6, A below 2^13, P
    below 2^26 and A A Q below 2^52, so each term of the criterion is exact in float64 and the reference decides the exact predicate."""
    v, f = ref.sheared_grid(10, 8, 3, 7, 1, seed=22)
    assert len(v) == 99 and len(f) == 160 and np.abs(v).max() <= 32 and (v == np.round(v)).all()
    before = _doubled_areas(v, f)
    assert min(before) > 0  # a valid triangulation of the parallelogram: every face counter-clockwise, and they tile it
    assert sum(before) == 2 * (10 * 3) * (8 * 7)
    start = ref.flip_round(v, f)
    assert start["totals"][1] > 60  # deliberately poor: the long diagonal everywhere
    g, per_round, converged, union = ref.delaunay_flips(v, f)
    assert converged and 2 <= len(per_round) <= 8 and union.sum() > 100
    end = ref.flip_round(v, g)
    assert end["totals"][1:] == [0, 0, 0]  # nothing left, guarded or not
    interior = np.nonzero(end["edge_state"] == ref.DELAUNAY)[0]
    assert len(interior) == end["E"] - 2 * (10 + 8)  # every edge off the outline has two faces and is eligible
    for e in interior:
        (lo, hi), (c, d) = end["edge_vertices"][e], end["edge_opposite"][e]
        assert _incircle(v[lo], v[hi], v[c], v[d]) < 0  # strictly outside: no cocircular quad, so the Delaunay triangulation is unique
    after = _doubled_areas(v, g)
    assert min(after) > 0 and sum(after) == sum(before)
    assert _use_counts(g) == _use_counts(f) and len(g) == len(f)
    V, E, F = len(v), end["E"], len(g)
    assert V - E + F == 1 and E == start["E"]  # a disc, before and after


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(flip_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tse_last_error.restype = ctypes.c_char_p; "
            "l.tse_workspace_bytes.restype = ctypes.c_size_t; print(l.tse_workspace_bytes(100000, 200000) >= 4 * 12 * 3 * 200000, "
            "repr(l.tse_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, flip_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(flip_path):
    out = subprocess.run(["nm", "-D", "--defined-only", flip_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES and len(NAMES) == 3
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", flip_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", flip_path], capture_output=True, text=True).stdout
    assert "libts_flip.so" in dynamic
    for other in ("libts2d.so", "libts_subdivide.so", "libts_manifold.so", "libts_orient.so", "libts_holes.so"):
        assert other not in dynamic


def test_header_defines_no_struct_and_states_the_contract():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsv|tsc|tsq|tss|tsh|tsf|tsw|tsa|tsi|tsn|tsx|tsd)_[a-z0-9_]+)\s*\(", text)  # a prefix of its own
    assert "struct" not in text
    assert re.findall(r"#define (TSE_\w+) (\d)", text) == [("TSE_NO_EDGE", "0"), ("TSE_NOT_ELIGIBLE", "1"), ("TSE_DELAUNAY", "2"), ("TSE_GUARDED", "3"),
                                                           ("TSE_LOST", "4"), ("TSE_DUPLICATE", "5"), ("TSE_FLIPPED", "6")]
    assert [ref.NO_EDGE, ref.NOT_ELIGIBLE, ref.DELAUNAY, ref.GUARDED, ref.LOST, ref.DUPLICATE, ref.FLIPPED] == list(range(7))
    full = open(HEADER).read()
    for word in ("TAKES PART", "ascending (lo, hi)", "ELIGIBLE", "opposite directions", "c != d", "twelve coordinates", "NON-DELAUNAY",
                 "(A A) Q > (B B) P", "(B B) P > (A A) Q", "P > 0 or Q > 0", "comparison with NaN is false", "cocircular", "is a cap", "CANDIDATE",
                 "binary search", "flip back", "D D >= M L", "D D <= M L", "dot(m0, S) > 0 && dot(m1, S) > 0", "0x9E3779B1", "0x85EBCA6B",
                 "0xC2B2AE35", "WINS", "smaller edge id", "DUPLICATES", "(a, d, c)", "(d, b, c)", "bit for bit", "to their capacity",
                 "{edges, nondelaunay, candidates, flipped}", "classifies only", "before any HIP call", "536870911", "2147483647", "Monotonic",
                 "nobody waits for anybody", "Purity", "-ffp-contract=off"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(FLIP_SIGNATURES) and len(declared) == 3
    for name, arity in declared.items():
        assert len(FLIP_SIGNATURES[name][1]) == arity, name
    assert declared["tse_flip"] == 16
    abi = _abi_module()
    tables = [getattr(abi, n) for n in dir(abi) if n.endswith("SIGNATURES")]
    assert len(tables) >= 18 and abi.FLIP_SIGNATURES in tables
    for a in range(len(tables)):
        for b in range(a + 1, len(tables)):
            assert not set(tables[a]) & set(tables[b])  # no signature table overlaps another
    args = FLIP_SIGNATURES["tse_flip"][1]
    assert args[5] == ctypes.c_float and args[6] == ctypes.c_uint32 and args[14] == ctypes.c_size_t
    assert FLIP_SIGNATURES["tse_workspace_bytes"][0] == ctypes.c_size_t
    # the prefix is this library's alone
    for path in (os.path.join(ROOT, "include"), os.path.join(ROOT, "triangle-splatting_amd", "csrc")):
        for name in os.listdir(path):
            if "flip" not in name:
                assert not re.search(r"\btse_", open(os.path.join(path, name)).read()), name


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_flip", ("build.py",))
    assert build.FLIP_SOURCES == {"mesh_flip.hip": ["-ffp-contract=off"], "api_flip.hip": []} and build.FLIP_SHARED == ["radix_sort"]
    assert build.flip_units() == ["mesh_flip", "api_flip"]
    cmd = build.flip_command("mesh_flip", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert "-ffp-contract=off" not in build.flip_command("api_flip")
    assert build.flip_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_flip", "api_flip", "radix_sort")]
    for others in (build.units(), build.smooth_units(), build.holes_units(), build.manifold_units(), build.orient_units(), build.subdivide_units()):
        assert not {"mesh_flip", "api_flip"} & set(others)  # its own library only
    assert build.FLIP_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_flip.so")
    for header in ("ts_flip_launch.h", "ts_mesh_edges.h", "ts_mesh_scan.h", "ts_mesh_common.h", os.path.join("..", "..", "include", "ts_flip.h")):
        assert header in build.HEADERS
    with pytest.raises(ValueError):
        build.flip_command("mesh_subdivide")


def test_built_objects_carry_the_flags_and_the_unit_uses_the_shared_front(flip_path):
    build = _load("ts2d_build_flip2", ("build.py",))
    for unit in ("mesh_flip", "api_flip"):
        stamp = open(os.path.join(build.OBJ_DIR, unit + ".o.cmd")).read()  # what the object on disk was compiled with
        assert stamp.endswith(" ".join(build.flip_command(unit, cc=stamp.splitlines()[1].split()[0])))
        assert ("-ffp-contract=off" in stamp) == (unit == "mesh_flip")
    link = open(build.FLIP_LIB + ".cmd").read()
    assert "-soname,libts_flip.so" in link and "radix_sort.o" in link and "mesh_subdivide" not in link
    text = open(os.path.join(build.CSRC, "mesh_flip.hip")).read()
    assert '#include "ts_mesh_edges.h"' in text and '#include "ts_mesh_scan.h"' in text
    for used in ("half_edge_records(", "sort_half_edges(", "edge_run_head(", "scan_columns<1>(", "face_takes_part(", "count4_into(", "Carver w("):
        assert used in text, used
    code = re.sub(r"//[^\n]*", "", text)
    assert "atomic" not in code  # the counters go through count_into / count4_into: integer adds, nothing else
    assert "sqrt" not in code and " / " not in code.replace("F / 2", "").replace("(r - l) / 2", "")  # no square root, no division in the criterion


def test_size_query_is_monotone_in_both_counts(lib):
    sizes = (0, 1, 2, 3, 63, 682, 683, 1024, 1025, 4097, 100000, 416666, 416667, 833333, 833334, 2499999, 2500000, 2500001, 2600000, 5000000,
             5000001, 5000002)
    for fixed in (0, 1000, 3000000):
        prev_v = prev_f = -1
        for n in sizes:
            by_v, by_f = lib.tse_workspace_bytes(n, fixed), lib.tse_workspace_bytes(fixed, n)
            assert by_v >= prev_v and by_f >= prev_f, (n, fixed)
            assert by_f >= 4 * 12 * 3 * n  # five words of the sort and seven of the round per half-edge
            prev_v, prev_f = by_v, by_f
    assert lib.tse_workspace_bytes(-5, -5) == lib.tse_workspace_bytes(0, 0)
    assert lib.tse_workspace_bytes(10, 2 ** 31 - 1) == lib.tse_workspace_bytes(10, MAX_FACES)


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    big = 1 << 40

    def refused(rc, word, code=INVALID):
        assert rc == code, rc
        text = lib.tse_last_error()
        assert text and word.encode() in text, text

    def flip(V=10, F=20, vertices=P, faces=P, keep=None, min_cos=0.5, seed=0, out_faces=P, flipped=P, ev=P, state=P, opposite=P, totals=P,
             ws=P, ws_bytes=big):
        return lib.tse_flip(V, F, vertices, faces, keep, min_cos, seed, out_faces, flipped, ev, state, opposite, totals, ws, ws_bytes, None)

    refused(flip(V=-1), ">= 0")
    refused(flip(V=-(2 ** 31)), ">= 0")
    refused(flip(F=-1), ">= 0")
    refused(flip(F=-(2 ** 31)), ">= 0")
    refused(flip(F=MAX_FACES + 1), "exceeds", CAPACITY)
    refused(flip(F=2 ** 31 - 1), "exceeds", CAPACITY)
    refused(flip(V=2 ** 31 - 1, F=1), "V + 3 F", CAPACITY)
    refused(flip(V=2 ** 31 - 1 - 3 * 1000 + 1, F=1000), "V + 3 F", CAPACITY)
    for bad in (1.5, -1.0000001, float("nan"), float("inf"), -float("inf")):
        refused(flip(min_cos=bad), "min_cos")
    refused(flip(totals=None), "totals")
    refused(flip(out_faces=None), "both")
    refused(flip(flipped=None), "both")
    refused(flip(faces=None), "faces")
    refused(flip(ev=None), "edge_vertices")
    refused(flip(state=None), "edge_vertices")
    refused(flip(opposite=None), "edge_vertices")
    refused(flip(vertices=None), "vertices")
    refused(flip(ws=None), "workspace")
    refused(flip(ws_bytes=lib.tse_workspace_bytes(10, 20) - 1), "too small")
    refused(flip(F=0, totals=None), "totals")  # an empty call still needs its totals
    refused(flip(F=0, out_faces=None), "both")


def test_python_module_checks_its_arguments_and_measures_quality():
    import torch
    import diff_recon_hip
    from diff_recon_hip import mesh_flip
    assert set(diff_recon_hip._FLIP_NAMES) <= set(mesh_flip.__all__) and diff_recon_hip.flip_edges is mesh_flip.flip_edges
    assert mesh_flip.EDGE_STATES == {"no_edge": ref.NO_EDGE, "not_eligible": ref.NOT_ELIGIBLE, "delaunay": ref.DELAUNAY, "guarded": ref.GUARDED,
                                     "lost": ref.LOST, "duplicate": ref.DUPLICATE, "flipped": ref.FLIPPED}
    for deg in (0.0, 30.0, 89.0, 90.0, 120.0, 180.0):  # the cosine in float64, rounded to fp32 once: what the reference takes
        assert mesh_flip.min_cos_of(deg) == float(ref.min_cos_of(deg))
    for deg in (-1.0, 180.5, float("nan")):
        with pytest.raises(ValueError):
            mesh_flip.min_cos_of(deg)
    v = torch.tensor([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 3.0 ** 0.5, 0.0], [4.0, 0.0, 0.0]])
    f = torch.tensor([[0, 1, 2], [0, 1, 3], [0, 1, 1], [0, 1, 7]], dtype=torch.int32)
    q = mesh_flip.triangle_quality(v, f)
    assert q.dtype == torch.float64 and abs(float(q[0]) - 1.0) < 1e-7 and float(q[1]) == 0.0 and bool(q[2:].isnan().all())
    q = mesh_flip.triangle_quality(v, f, keep=torch.tensor([False, True, True, True]))
    assert bool(q[0].isnan()) and float(q[1]) == 0.0
    with pytest.raises(RuntimeError):  # the kernels have no CPU fallback
        mesh_flip.flip_edges(v, f)
    with pytest.raises(ValueError):
        mesh_flip.delaunay_flips(v, f, max_rounds=0)
