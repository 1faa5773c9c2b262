"""CPU tests of the edge collapse (no GPU): the numpy reference of include/ts_collapse.h on hand constructions whose results are known by
hand -- held ends, the tetrahedron, the octahedron, fans, the ring bound, the link, length and normal guards, a crease, a zero-length edge,
pins, the direction rule, non-finite coordinates and limits, the ends of the binary search; the independence of a round's winners against a
brute-force test on Python sets; the counts and the topology per round and to convergence on closed manifold meshes;
libts_collapse.so is a library of its own with exactly the C ABI of the header, and every argument check answers before any HIP call."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_collapse as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_collapse.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tsp_collapse", "tsp_last_error", "tsp_workspace_bytes"]
MAX_FACES = 536870911
COS_30 = ref.min_cos_of(30.0)
HAND = ref.hand_constructions()


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_collapse", ("diff_triangle_rasterization_2D", "_abi.py"))


COLLAPSE_SIGNATURES = _abi_module().COLLAPSE_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def collapse_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_collapse.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_collapse.so"
    return path


@pytest.fixture(scope="module")
def lib(collapse_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_collapse(ctypes.CDLL(collapse_path))


def _header_prototypes():
    """name -> number of parameters of every tsp_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


def _round(name, **more):
    v, f, rule = HAND[name]
    return ref.collapse_round(v, f, **dict(rule, **more))


def _edges(o):
    """{(lo, hi): (state, removed, guard)} of the round's edge table."""
    E = o["E"]
    return {tuple(e): (int(s), int(r), int(g)) for e, s, r, g in
            zip(o["edge_vertices"][:E].tolist(), o["edge_state"][:E], o["edge_removed"][:E], o["edge_guard"][:E])}


def _fills(o):
    """The capacity beyond E holds the fill values, and everything has its shape."""
    E, F = o["E"], len(o["out_faces"])
    assert o["edge_vertices"].shape == (3 * F, 2) and o["edge_state"].shape == (3 * F,) and o["edge_removed"].shape == (3 * F,)
    assert o["edge_guard"].shape == (3 * F,) and o["out_keep"].shape == (F,)
    assert (o["edge_vertices"][E:] == -1).all() and (o["edge_state"][E:] == ref.NO_EDGE).all() and (o["edge_removed"][E:] == -1).all()
    assert (o["edge_guard"][E:] == 0).all() and o["totals"][0] == E
    quiet = o["edge_state"][:E] <= ref.LONG_ENOUGH  # only a short edge carries a mask, only a candidate a removed vertex
    assert (o["edge_guard"][:E][quiet] == 0).all() and ((o["edge_removed"][:E] >= 0) == (o["edge_state"][:E] >= ref.LOST)).all()


def _topology(V, faces, keep=None):
    """Counts of the kept faces on Python's own terms: referenced vertices, edges by use, pieces, Euler characteristic, duplicate faces."""
    f = np.asarray(faces).reshape(-1, 3)
    if keep is not None:
        f = f[np.asarray(keep) != 0]
    use = {}
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in f.tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            use[(min(p, q), max(p, q))] = use.get((min(p, q), max(p, q)), 0) + 1
            parent[find(p)] = find(q)
    named = sorted(set(f.reshape(-1).tolist()))
    triples = [tuple(sorted(t)) for t in f.tolist()]
    return {"vertices": len(named), "edges": len(use), "faces": len(f), "boundary": sum(u == 1 for u in use.values()),
            "nonmanifold": sum(u >= 3 for u in use.values()), "pieces": len({find(x) for x in named}),
            "euler": len(named) - len(use) + len(f), "duplicates": len(triples) - len(set(triples)), "use": use}


# ---- held ends ----------------------------------------------------------------------------------------------------------------------------
def test_one_face_and_the_two_face_quad_have_nothing_to_collapse():
    for name, E in (("one face", 3), ("two-face quad", 5)):
        o = _round(name)
        _fills(o)
        assert o["totals"] == [E, 0, 0, 0] and not o["vertex_free"].any()  # every vertex lies on the boundary: both ends of every edge are held
        assert set(s for s, _, _ in _edges(o).values()) == {ref.NOT_ELIGIBLE}
        assert o["out_faces"].tolist() == np.asarray(HAND[name][1]).tolist() and o["out_keep"].all()
        assert o["vertex_target"].tolist() == list(range(4))


# ---- the guards ---------------------------------------------------------------------------------------------------------------------------
def test_closed_tetrahedron_is_guarded_by_the_face_on_c_and_d():
    o = _round("tetrahedron")
    _fills(o)
    assert o["vertex_free"].all() and o["totals"] == [6, 6, 0, 0]
    for state, removed, guard in _edges(o).values():  # the one surviving face of r is (r, c, d): two faces on one triple otherwise
        assert state == ref.GUARDED and removed == -1 and guard & ref.GUARD_LINK and not guard & ref.GUARD_HELD
    assert o["out_keep"].all() and o["out_faces"].tolist() == ref.TETRAHEDRON[1].tolist()


def test_octahedron_collapses_once_into_the_double_pyramid():
    v, f = ref.OCTAHEDRON
    o = _round("octahedron")
    _fills(o)
    assert o["totals"] == [12, 12, 12, 1]  # every vertex lies in the closed ring of every edge: one winner
    t = _topology(6, o["out_faces"], o["out_keep"])
    assert (t["vertices"], t["edges"], t["faces"], t["euler"]) == (5, 9, 6, 2) and t["boundary"] == t["nonmanifold"] == t["duplicates"] == 0
    # the normal guard by hand: r = (0, 0, 2) -> k = (2, 0, 0) turns the face on c = (0, 2, 0) and the antipode of k
    # from n0 = (-4, 4, 4) to n1 = (0, 0, 8): D = 32 > 0, cos^2 = 1024 / (48 * 64) = 1/3, so it passes at 60 degrees and fails at 30
    assert _round("octahedron", min_cos=ref.min_cos_of(60.0))["totals"][2] == 12 and _round("octahedron", min_cos=COS_30)["totals"][1:] == [12, 0, 0]
    # the next round on the double pyramid (apex 4 over the base 0, 2, 1, 3, cut by the edge (2, 3) of length 4: long enough).  The two
    # edges from the apex to the ends of that diagonal are guarded by the link: 2 and 3 have valence four, and the other end of the
    # diagonal is adjacent to both.  Six edges can go, one does, and what is left is a tetrahedron, where nothing can (the test above).
    nxt = ref.collapse_round(v, o["out_faces"], keep=o["out_keep"], min_edge=3.0, min_cos=0.0, seed=1)
    assert nxt["totals"] == [9, 8, 6, 1] and _edges(nxt)[(2, 3)][0] == ref.LONG_ENOUGH
    assert _edges(nxt)[(2, 4)] == _edges(nxt)[(3, 4)] == (ref.GUARDED, -1, ref.GUARD_LINK)
    after = _topology(6, nxt["out_faces"], nxt["out_keep"])
    assert (after["vertices"], after["edges"], after["faces"], after["euler"]) == (4, 6, 4, 2)
    assert after["boundary"] == after["nonmanifold"] == after["duplicates"] == 0
    g, k, target, per_round, converged = ref.collapse_short_edges(v, f, min_edge=3.0, min_cos=0.0)
    assert converged and per_round == [[12, 12, 12, 1], [9, 8, 6, 1]] and np.array_equal(g, nxt["out_faces"]) and np.array_equal(k, nxt["out_keep"])
    last = ref.collapse_round(v, g, keep=k, min_edge=3.0, min_cos=0.0, seed=2)
    assert last["totals"] == [6, 5, 0, 0]  # five short edges, the sixth is the diagonal of length 4; all guarded


def test_hexagon_fan_centre_collapses_onto_the_rim():
    o = _round("hexagon fan")
    _fills(o)
    assert o["vertex_free"].tolist() == [True] + [False] * 6 and o["totals"] == [12, 1, 1, 1]
    assert _edges(o)[(0, 1)] == (ref.COLLAPSED, 0, ref.GUARD_HELD)  # hi = 1 lies on the boundary: held, so lo = 0 goes
    assert o["vertex_target"].tolist() == [1, 1, 2, 3, 4, 5, 6]
    assert o["out_keep"].tolist() == [0, 1, 1, 1, 1, 0] and o["out_faces"].tolist() == [[0, 1, 2], [1, 2, 3], [1, 3, 4], [1, 4, 5], [1, 5, 6], [0, 6, 1]]
    t = _topology(7, o["out_faces"], o["out_keep"])
    assert (t["vertices"], t["faces"], t["euler"], t["boundary"]) == (6, 4, 1, 6)  # 6 -> 4 faces, still a disc with the same outline


def test_ring_bound_holds_a_centre_of_65_and_frees_one_of_64():
    o = _round("fan of 65")
    assert o["totals"] == [130, 0, 0, 0] and not o["vertex_free"].any()  # the centre's ring has 65 corners: held, like the rim
    assert _edges(o)[(0, 1)][0] == ref.NOT_ELIGIBLE and o["out_keep"].all()
    o = _round("fan of 64")
    assert o["totals"] == [128, 1, 1, 1] and o["vertex_free"].tolist() == [True] + [False] * 64
    assert _edges(o)[(0, 1)] == (ref.COLLAPSED, 0, ref.GUARD_HELD) and o["out_keep"].sum() == 62
    assert ref.MAX_RING == 64


def test_link_guard_on_a_waist_of_three_edges_that_bounds_no_face():
    o = _round("waisted tube")
    _fills(o)
    assert o["vertex_free"].all() and o["totals"] == [45, 3, 0, 0]
    for e in ((6, 7), (6, 8), (7, 8)):  # the third vertex of the waist is adjacent to both ends and opposite to neither face
        assert _edges(o)[e] == (ref.GUARDED, -1, ref.GUARD_LINK)
    assert o["out_keep"].all()


def test_fold_guard_on_a_concave_ring():
    v, f, rule = HAND["concave ring"]
    o = _round("concave ring")
    state, removed, guard = _edges(o)[(0, 1)]  # the centre onto rim point 1 would turn the face (0, 2, 3) over: rim point 2 lies below 1-3
    assert state == ref.GUARDED and removed == -1 and guard == ref.GUARD_HELD | ref.GUARD_NORMAL
    p = v.astype(np.float64)
    area = lambda a, b, c: (p[b][0] - p[a][0]) * (p[c][1] - p[a][1]) - (p[b][1] - p[a][1]) * (p[c][0] - p[a][0])
    assert area(0, 2, 3) > 0 and area(1, 2, 3) < 0
    assert _edges(o)[(0, 2)][:2] == (ref.COLLAPSED, 0)  # onto rim point 2 itself the ring is star-shaped
    for a, b, c in o["out_faces"][o["out_keep"] != 0].tolist():
        assert area(a, b, c) > 0


def test_a_vertex_on_a_crease_slides_along_it_but_not_off_it():
    o = _round("cube edge")
    _fills(o)
    edges = _edges(o)
    assert o["vertex_free"].all() and o["totals"] == [21, 21, 2, 1]
    assert edges[(0, 8)] == (ref.COLLAPSED, 8, 0) and edges[(1, 8)] == (ref.LOST, 8, 0)  # along the crease, either way; the shorter first
    for e in ((3, 8), (4, 8), (5, 8)):  # off the crease, into a face of the cube: the faces of the other side turn by 90 degrees
        assert edges[e] == (ref.GUARDED, -1, ref.GUARD_NORMAL)
    for e, (state, removed, guard) in edges.items():
        if 8 not in e:  # a corner of the cube cannot move at all
            assert (state, removed, guard) == (ref.GUARDED, -1, ref.GUARD_NORMAL), e
    t = _topology(9, o["out_faces"], o["out_keep"])
    assert (t["vertices"], t["edges"], t["faces"], t["euler"]) == (8, 18, 12, 2)  # the cube again


def test_zero_length_edge_is_short_and_collapses():
    o = _round("zero length")
    assert o["totals"] == [18, 1, 1, 1] and _edges(o)[(0, 1)] == (ref.COLLAPSED, 1, 0)  # the two degenerate faces go, no normal turns
    assert _round("zero length", min_edge=0.0)["totals"] == [18, 0, 0, 0]  # 0 < 0 is false


def test_max_edge_guard_at_equality():
    o = _round("max_edge at equality")  # 1 -> 0 creates three edges of squared length 6.25 = 2.5^2: <= passes
    assert o["totals"] == [12, 1, 1, 1] and _edges(o)[(0, 1)] == (ref.COLLAPSED, 1, 0)
    v = ref.square_fan()[0].astype(np.float64)
    assert ref.length2(v, np.array([0, 0, 0]), np.array([2, 4, 5])).tolist() == [6.25, 6.25, 6.25]
    o = _round("max_edge just below")  # one ulp of fp32 less: 1 -> 0 is too long, and 0 -> 1 would create (1, 3) of length 4
    assert o["totals"] == [12, 1, 0, 0] and _edges(o)[(0, 1)] == (ref.GUARDED, -1, ref.GUARD_LONG) and o["out_keep"].all()
    assert _round("max_edge at equality", max_edge=np.inf)["totals"] == [12, 1, 1, 1]


def test_pinned_vertices_and_the_direction_rule():
    assert _edges(_round("closed hexagon fan"))[(0, 1)] == (ref.COLLAPSED, 1, 0)            # hi first
    assert _edges(_round("pinned rim"))[(0, 1)] == (ref.COLLAPSED, 0, ref.GUARD_HELD)      # hi is held: lo
    assert _edges(_round("pinned centre"))[(0, 1)] == (ref.COLLAPSED, 1, 0)                # lo is held: hi was first anyway
    both = _round("pinned both")
    assert _edges(both)[(0, 1)][0] == ref.NOT_ELIGIBLE and both["totals"] == [18, 0, 0, 0]  # no free end: not even short
    o = _round("nan in the ring")  # hi -> lo reads the non-finite apex: guarded (length and normal), so lo -> hi, whose ring is finite
    assert _edges(o)[(0, 1)] == (ref.COLLAPSED, 0, ref.GUARD_LONG | ref.GUARD_NORMAL) and not o["vertex_free"][7]
    v, f, rule = HAND["closed hexagon fan"]
    o = ref.collapse_round(v, f, pinned=[0, 1, 0, 0, 0, 0, 0, 0], **rule)
    assert o["vertex_target"].tolist() == [1, 1, 2, 3, 4, 5, 6, 7] and o["out_keep"].sum() == 10


def test_non_finite_coordinates_and_limits():
    v, f, rule = HAND["closed hexagon fan"]
    for bad in (np.nan, np.inf, -np.inf):
        for vertex in (0, 1, 2, 6):  # lo, hi, c, d of the edge (0, 1)
            w = v.copy()
            w[vertex, 1] = bad
            o = ref.collapse_round(w, f, **rule)
            assert _edges(o)[(0, 1)] == (ref.NOT_ELIGIBLE, -1, 0) and o["totals"][3] == 0 and not o["vertex_free"][vertex]
    assert _round("nan")["totals"] == [18, 0, 0, 0] and _round("inf")["totals"] == [18, 0, 0, 0]
    assert _round("vertex limit")["totals"] == [18, 1, 1, 1] and _round("vertex limit with a NaN")["totals"] == [18, 0, 0, 0]
    limit = np.full(8, 1.0, np.float32)
    limit[0] = 0.4  # the smaller limit of the two ends counts: 0.5 is not below it
    assert ref.collapse_round(v, f, vertex_limit=limit, min_cos=COS_30)["totals"] == [18, 0, 0, 0]
    limit[0] = np.inf
    assert ref.collapse_round(v, f, vertex_limit=limit, min_cos=COS_30)["totals"] == [18, 1, 1, 1]
    assert ref.collapse_round(v, f, min_edge=np.inf, min_cos=COS_30)["totals"][1] == 18  # every eligible edge is short
    for name in ("masked", "out of range"):
        o = _round(name)
        _fills(o)
        assert o["totals"][3] == 1
    o = _round("masked")  # the masked face leaves a hole: its three vertices are boundary vertices, held
    assert o["vertex_free"].tolist() == [True, False, True, True, True, True, False, False] and o["out_keep"][11] == 0
    o = _round("out of range")
    assert o["out_faces"][12:].tolist() == [[0, 1, 9], [2, 2, 3], [-1, 0, 1]] and o["out_keep"][12:].all()  # copied bit for bit
    empty = ref.collapse_round(np.zeros((0, 3), np.float32), f, min_edge=1.0)  # V == 0: nothing takes part
    assert empty["totals"] == [0, 0, 0, 0] and empty["out_faces"].tolist() == f.tolist() and (empty["edge_state"] == ref.NO_EDGE).all()
    assert ref.collapse_round(v, np.zeros((0, 3), np.int32), min_edge=1.0)["vertex_target"].tolist() == list(range(8))


def test_binary_search_in_front_of_the_first_and_behind_the_last_entry():
    """The link guard asks for (min(x, k), max(x, k)).  The closed hexagon fan relabelled so that the one pair asked for -- the apex x, in
    the ring of rim point r but not adjacent to the centre k -- sorts in front of the first entry of the table, (0, 1) before (0, 2), and
    behind its last, (6, 7) after (5, 7); each also with masked faces behind, whose sentinel keys end the sorted columns."""
    v, f, rule = HAND["closed hexagon fan"]  # centre 0, rim 1 .. 6, apex 7; the short edge is (0, 1)
    for relabel, pinned, edge, asked in ((np.array([0, 2, 3, 4, 5, 6, 7, 1]), None, (0, 2), (0, 1)),
                                         (np.array([7, 5, 0, 1, 2, 3, 4, 6]), [0, 0, 0, 0, 0, 0, 0, 1], (5, 7), (6, 7))):  # the centre pinned: r is the rim point
        w, g = np.empty_like(v), relabel[f].astype(np.int32)
        w[relabel] = v
        for extra, keep in ((np.zeros((0, 3), np.int32), None), (np.array([[0, 1, 2], [5, 6, 7]], np.int32), [1] * 12 + [0, 0])):
            o = ref.collapse_round(w, np.concatenate([g, extra]), keep=keep, pinned=pinned, **rule)
            _fills(o)
            table = [tuple(e) for e in o["edge_vertices"][:o["E"]].tolist()]
            r, k = (2, 0) if pinned is None else (5, 7)
            assert o["totals"] == [18, 1, 1, 1] and _edges(o)[edge][:2] == (ref.COLLAPSED, r)
            near_r = {x for e in table if r in e for x in e} - {r, k}
            assert asked in {(min(x, k), max(x, k)) for x in near_r} and asked not in table
            assert asked < table[0] if pinned is None else asked > table[-1]


# ---- independence -------------------------------------------------------------------------------------------------------------------------
def _meshes():
    yield "grid 9 x 9", ref.jittered_grid(9, 9, 0.3, seed=2, z=0.1), dict(min_edge=0.8, max_edge=2.2, min_cos=COS_30)
    yield "grid 17 x 17", ref.jittered_grid(17, 17, 0.3, seed=3, z=0.1), dict(min_edge=0.9, max_edge=2.5, min_cos=COS_30)
    yield "regular grid", ref.jittered_grid(12, 12, 0.0), dict(min_edge=1.2, max_edge=2.5, min_cos=COS_30)
    yield "sphere", ref.jittered_sphere(12, 16, 0.02, seed=4), dict(min_edge=0.3, max_edge=0.9, min_cos=ref.min_cos_of(45.0))


@pytest.mark.parametrize("name", [name for name, _, _ in _meshes()])
def test_winners_are_independent_and_the_round_equals_them_one_by_one(name):
    (v, f), rule = next((mesh, rule) for n, mesh, rule in _meshes() if n == name)
    g, keep = f, None
    total = 0
    for seed in range(3):
        o = ref.collapse_round(v, g, keep=keep, seed=seed, **rule)
        E = o["E"]
        kept = g if keep is None else g[keep != 0]
        near = {}
        for a, b, c in kept.tolist():
            for p, q in ((a, b), (b, c), (c, a)):
                near.setdefault(p, set()).add(q)
                near.setdefault(q, set()).add(p)
        winners = [(int(r), int(lo + hi - r)) for (lo, hi), s, r in zip(o["edge_vertices"][:E].tolist(), o["edge_state"][:E], o["edge_removed"][:E]) if s == ref.COLLAPSED]
        assert len(winners) == o["totals"][3]
        triples = {tuple(sorted(t)) for t in kept.tolist()}
        zones = []
        for r, k in winners:
            common = near[r] & near[k]
            assert len(common) == 2 and all(tuple(sorted((r, k, x))) in triples for x in common)  # the link condition: only c and d
            assert o["vertex_free"][r]
            zones.append(({r, k}, {r, k} | near[r] | near[k]))
        for i, (ends, _) in enumerate(zones):  # no winner has an end inside the closed rings of another winner's ends
            for j, (_, zone) in enumerate(zones):
                assert i == j or not ends & zone
        for order in (winners, winners[::-1]):  # one at a time, in two orders
            h, hk = g, keep
            for r, k in order:
                h, hk = ref.apply_one(h, hk, r, k)
            hk = np.ones(len(g), np.uint8) if hk is None else hk
            assert np.array_equal(h[hk != 0], o["out_faces"][o["out_keep"] != 0]) and np.array_equal(hk, o["out_keep"])
        total += len(winners)
        g, keep = o["out_faces"], o["out_keep"]
    assert total > (4 if name != "sphere" else 10)
    if name == "regular grid":  # ties everywhere: the seed picks the set
        assert len({ref.collapse_round(v, f, seed=s, **rule)["edge_state"].tobytes() for s in range(4)}) > 1
        h = (3 * 0x9E3779B1 + 5) & 0xFFFFFFFF
        h ^= h >> 16; h = (h * 0x85EBCA6B) & 0xFFFFFFFF; h ^= h >> 13; h = (h + 7) & 0xFFFFFFFF; h = (h * 0xC2B2AE35) & 0xFFFFFFFF; h ^= h >> 16
        assert int(ref.priority([5], [7], 3)[0]) == h


# ---- invariants on closed manifold meshes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "closed fan", "cube edge"])
def test_counts_and_topology_per_round_and_to_convergence(name):
    (v, f), rule = {"sphere": (ref.jittered_sphere(12, 16, 0.02, seed=4), dict(min_edge=0.3, max_edge=0.9, min_cos=ref.min_cos_of(45.0))),
                    "closed fan": (ref.closed_fan(24, (1.0, 0.3, 0.0)), dict(min_edge=1.5, max_edge=3.5, min_cos=COS_30)),
                    "cube edge": (ref.cube_with_edge_vertex(), dict(min_edge=1.0, min_cos=COS_30))}[name]
    V = len(v)
    start = _topology(V, f)
    assert start["boundary"] == start["nonmanifold"] == start["duplicates"] == 0 and start["euler"] == 2 and start["pieces"] == 1
    g, keep, before, rounds = f, None, start, 0
    for seed in range(64):
        o = ref.collapse_round(v, g, keep=keep, seed=seed, **rule)
        n = o["totals"][3]
        if n == 0:
            break
        rounds += 1
        after = _topology(V, o["out_faces"], o["out_keep"])
        assert (after["vertices"], after["edges"], after["faces"]) == (before["vertices"] - n, before["edges"] - 3 * n, before["faces"] - 2 * n)
        for key in ("pieces", "boundary", "nonmanifold", "euler", "duplicates"):  # closed, one piece, a sphere, no edge of use 3, no face twice
            assert after[key] == start[key], (key, seed)
        limit2 = np.float64(np.float32(rule.get("max_edge", np.inf))) ** 2
        for e in set(after["use"]) - set(before["use"]):  # no edge above max_edge is created
            assert ref.length2(v.astype(np.float64), np.array([e[0]]), np.array([e[1]]))[0] <= limit2, e
        g, keep, before = o["out_faces"], o["out_keep"], after
    else:
        raise AssertionError("the reference did not converge in 64 rounds")
    assert rounds >= (1 if name == "cube edge" else 2) and o["totals"][2] == 0  # converged: no candidate is left ...
    E = o["E"]
    lengths2 = ref.length2(v.astype(np.float64), o["edge_vertices"][:E, 0], o["edge_vertices"][:E, 1])
    still = lengths2 < np.float64(np.float32(rule["min_edge"])) ** 2
    free = o["vertex_free"]
    for e in np.nonzero(still)[0]:  # ... and every edge still short is GUARDED or has two held ends
        lo, hi = o["edge_vertices"][e]
        assert o["edge_state"][e] == ref.GUARDED or (o["edge_state"][e] == ref.NOT_ELIGIBLE and not free[lo] and not free[hi]), e
    whole = ref.collapse_short_edges(v, f, **rule)
    assert whole[4] and len(whole[3]) == rounds and np.array_equal(whole[0], g) and np.array_equal(whole[1], keep)
    assert (whole[2] == np.arange(V)).sum() == before["vertices"]  # the vertices that map to themselves are the ones still named


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(collapse_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsp_last_error.restype = ctypes.c_char_p; "
            "l.tsp_workspace_bytes.restype = ctypes.c_size_t; print(l.tsp_workspace_bytes(100000, 200000) >= 4 * 14 * 3 * 200000, "
            "repr(l.tsp_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, collapse_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(collapse_path):
    out = subprocess.run(["nm", "-D", "--defined-only", collapse_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES and len(NAMES) == 3
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", collapse_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", collapse_path], capture_output=True, text=True).stdout
    assert "libts_collapse.so" in dynamic
    for other in ("libts2d.so", "libts_subdivide.so", "libts_flip.so", "libts_manifold.so", "libts_orient.so"):
        assert other not in dynamic


def test_header_defines_no_struct_and_states_the_contract():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsv|tsc|tsq|tss|tsh|tsf|tsw|tsa|tsi|tsn|tsx|tsd|tse)_[a-z0-9_]+)\s*\(", text)  # a prefix of its own
    assert "struct" not in text
    assert re.findall(r"#define (TSP_\w+) (\d+)", text) == [
        ("TSP_NO_EDGE", "0"), ("TSP_NOT_ELIGIBLE", "1"), ("TSP_LONG_ENOUGH", "2"), ("TSP_GUARDED", "3"), ("TSP_LOST", "4"), ("TSP_COLLAPSED", "5"),
        ("TSP_MARK_SHORTER", "1"), ("TSP_MARK_VERTEX_LIMIT", "2"), ("TSP_GUARD_LINK", "1"), ("TSP_GUARD_LONG", "2"), ("TSP_GUARD_NORMAL", "4"),
        ("TSP_GUARD_HELD", "8"), ("TSP_MAX_RING", "64")]
    assert [ref.NO_EDGE, ref.NOT_ELIGIBLE, ref.LONG_ENOUGH, ref.GUARDED, ref.LOST, ref.COLLAPSED] == list(range(6))
    assert (ref.MARK_SHORTER, ref.MARK_VERTEX_LIMIT, ref.GUARD_LINK, ref.GUARD_LONG, ref.GUARD_NORMAL, ref.GUARD_HELD, ref.MAX_RING) == (1, 2, 1, 2, 4, 8, 64)
    subdivide = open(os.path.join(ROOT, "include", "ts_subdivide.h")).read()
    assert "#define TSD_MARK_LONGER 1" in subdivide and "#define TSD_MARK_VERTEX_LIMIT 2" in subdivide  # the modes mirror the split's marks
    full = open(HEADER).read()
    for word in ("TAKES PART", "ascending (lo, hi)", "CLEAN", "opposite directions", "FREE", "HELD", "TSP_MAX_RING = 64", "ELIGIBLE", "c != d",
                 "twelve coordinates", "at least one", "l2 < L L", "limit[hi] < limit[lo]", "zero-length edge is short", "r = hi, k = lo",
                 "r = lo, k = hi", "without\n * early exit", "binary search", "SURVIVING", "{x, y} = {c, d}", "(double)max_edge (double)max_edge",
                 "+inf", "Q1 > 0 && (Q0 == 0 || (D > 0 && D D >= (M Q0) Q1))", "comparison with NaN is false", "CANDIDATE", "TSP_GUARDED",
                 "0x9E3779B1", "0x85EBCA6B", "0xC2B2AE35", "l2 ascending, priority descending, edge id ascending", "best2[a] == best2[b] == e",
                 "distance two", "in any order", "at most one index changes", "bit for bit", "to their capacity",
                 "{edges, short, candidates, collapsed}", "classifies only", "before any HIP call", "536870911", "2147483647", "Monotonic",
                 "nobody waits for anybody", "walked, never stored", "Purity", "-ffp-contract=off"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(COLLAPSE_SIGNATURES) and len(declared) == 3
    for name, arity in declared.items():
        assert len(COLLAPSE_SIGNATURES[name][1]) == arity, name
    assert declared["tsp_collapse"] == 23
    abi = _abi_module()
    tables = [getattr(abi, n) for n in dir(abi) if n.endswith("SIGNATURES")]
    assert len(tables) >= 19 and abi.COLLAPSE_SIGNATURES in tables
    for a in range(len(tables)):
        for b in range(a + 1, len(tables)):
            assert not set(tables[a]) & set(tables[b])  # no signature table overlaps another
    args = COLLAPSE_SIGNATURES["tsp_collapse"][1]
    assert args[6] == ctypes.c_int32 and args[7] == args[9] == args[10] == ctypes.c_float and args[11] == ctypes.c_uint32 and args[21] == ctypes.c_size_t
    assert COLLAPSE_SIGNATURES["tsp_workspace_bytes"][0] == ctypes.c_size_t
    # the prefix is this library's alone
    for path in (os.path.join(ROOT, "include"), os.path.join(ROOT, "triangle-splatting_amd", "csrc")):
        for name in os.listdir(path):
            if "collapse" not in name:
                assert not re.search(r"\btsp_", open(os.path.join(path, name)).read(), flags=re.I), name


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_collapse", ("build.py",))
    assert build.COLLAPSE_SOURCES == {"mesh_collapse.hip": ["-ffp-contract=off"], "api_collapse.hip": []} and build.COLLAPSE_SHARED == ["radix_sort"]
    assert build.collapse_units() == ["mesh_collapse", "api_collapse"]
    cmd = build.collapse_command("mesh_collapse", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert "-ffp-contract=off" not in build.collapse_command("api_collapse")
    assert build.collapse_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_collapse", "api_collapse", "radix_sort")]
    for others in (build.units(), build.smooth_units(), build.holes_units(), build.manifold_units(), build.orient_units(), build.subdivide_units(),
                   build.flip_units()):
        assert not {"mesh_collapse", "api_collapse"} & set(others)  # its own library only
    assert build.COLLAPSE_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_collapse.so")
    for header in ("ts_collapse_launch.h", "ts_mesh_edge_ids.h", "ts_mesh_edges.h", "ts_mesh_scan.h", "ts_mesh_common.h",
                   os.path.join("..", "..", "include", "ts_collapse.h")):
        assert header in build.HEADERS and os.path.exists(os.path.join(build.CSRC, header)), header
    with pytest.raises(ValueError):
        build.collapse_command("mesh_flip")


def test_built_objects_carry_the_flags_and_the_unit_keeps_its_rules(collapse_path):
    build = _load("ts2d_build_collapse2", ("build.py",))
    for unit in ("mesh_collapse", "api_collapse"):
        stamp = open(os.path.join(build.OBJ_DIR, unit + ".o.cmd")).read()  # what the object on disk was compiled with
        assert stamp.endswith(" ".join(build.collapse_command(unit, cc=stamp.splitlines()[1].split()[0])))
        assert ("-ffp-contract=off" in stamp) == (unit == "mesh_collapse")
    link = open(build.COLLAPSE_LIB + ".cmd").read()
    assert "-soname,libts_collapse.so" in link and "radix_sort.o" in link and "mesh_subdivide" not in link and "mesh_flip" not in link
    text = open(os.path.join(build.CSRC, "mesh_collapse.hip")).read()
    assert '#include "ts_mesh_edge_ids.h"' in text
    shared = open(os.path.join(build.CSRC, "ts_mesh_edge_ids.h")).read()
    assert '#include "ts_mesh_edges.h"' in shared and '#include "ts_mesh_scan.h"' in shared
    for used in ("edge_run_head(", "scan_columns<1>(", "edge_heads_kernel", "edge_ids_kernel", "edge_scatter_kernel"):
        assert used in shared, used
    for used in ("half_edge_records(", "sort_half_edges(", "number_edges(", "face_takes_part(", "count4_into(", "count_into(", "Carver w("):
        assert used in text, used
    code = re.sub(r"//[^\n]*", "", text)
    for copied in ("heads_kernel", "runs_kernel", "scatter_kernel"):  # no third copy of the three small kernels of the front
        assert not re.search(r"__global__[^;{]*\b%s\b" % copied, code), copied
    assert "atomic" not in code  # the counters go through count_into / count4_into: integer adds, nothing else
    assert not re.search(r"\bmesh_fill\(|\bmesh_copy\(|\bhipMem(?:set|cpy)\w*", code)  # every element is written by the kernel that owns it
    assert not re.search(r"hipMalloc|hipFree|Synchronize", code)  # no call allocates or synchronises with the host
    assert "sqrt" not in code and " / " not in code.replace("(r - l) / 2", "")  # no square root, no division in the decisions
    assert not re.search(r"\[(?:MAX_RING|64)\]", code)  # rings are walked, never stored
    resources = open(os.path.join(ROOT, "profiles", "mesh_collapse_resources.txt")).read()
    rows = re.findall(r"^mesh_collapse\s+(\S+)\s+(\d+)/(\d+)/\s*(\d+)/(\d+)", resources, flags=re.M)
    assert {"classify_kernel", "vertex_class_kernel", "best_kernel", "best2_kernel", "winners_kernel", "apply_kernel"} <= {r[0] for r in rows}
    assert all(r[2] == "0" for r in rows)  # no kernel uses scratch


def test_size_query_is_monotone_in_both_counts(lib):
    sizes = (0, 1, 2, 3, 63, 682, 683, 1024, 1025, 4097, 100000, 416666, 416667, 833333, 833334, 2499999, 2500000, 2500001, 2600000, 5000000,
             5000001, 5000002)
    for fixed in (0, 1000, 3000000):
        prev_v = prev_f = -1
        for n in sizes:
            by_v, by_f = lib.tsp_workspace_bytes(n, fixed), lib.tsp_workspace_bytes(fixed, n)
            assert by_v >= prev_v and by_f >= prev_f, (n, fixed)
            assert by_f >= 4 * 14 * 3 * n and by_v >= 17 * n  # words per half-edge; four words and a byte per vertex
            prev_v, prev_f = by_v, by_f
    assert lib.tsp_workspace_bytes(-5, -5) == lib.tsp_workspace_bytes(0, 0)
    assert lib.tsp_workspace_bytes(10, 2 ** 31 - 1) == lib.tsp_workspace_bytes(10, MAX_FACES)


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    big = 1 << 40

    def refused(rc, word, code=INVALID):
        assert rc == code, rc
        text = lib.tsp_last_error()
        assert text and word.encode() in text, text

    def collapse(V=10, F=20, vertices=P, faces=P, keep=None, pinned=None, mode=1, min_edge=0.5, limit=None, max_edge=float("inf"), min_cos=0.5,
                 seed=0, out_faces=P, out_keep=P, target=P, ev=P, state=P, removed=P, guard=P, totals=P, ws=P, ws_bytes=big):
        return lib.tsp_collapse(V, F, vertices, faces, keep, pinned, mode, min_edge, limit, max_edge, min_cos, seed, out_faces, out_keep, target,
                                ev, state, removed, guard, totals, ws, ws_bytes, None)

    refused(collapse(V=-1), ">= 0")
    refused(collapse(V=-(2 ** 31)), ">= 0")
    refused(collapse(F=-1), ">= 0")
    refused(collapse(F=-(2 ** 31)), ">= 0")
    refused(collapse(F=MAX_FACES + 1), "exceeds", CAPACITY)
    refused(collapse(F=2 ** 31 - 1), "exceeds", CAPACITY)
    refused(collapse(V=2 ** 31 - 1, F=1), "V + 3 F", CAPACITY)
    refused(collapse(V=2 ** 31 - 1 - 3 * 1000 + 1, F=1000), "V + 3 F", CAPACITY)
    for bad in (1.5, -0.0000001, -1.0, float("nan"), float("inf"), -float("inf")):
        refused(collapse(min_cos=bad), "min_cos")
    for bad in (-1.0, float("nan"), -float("inf")):
        refused(collapse(min_edge=bad), "min_edge")
        assert collapse(mode=2, min_edge=bad, limit=P, F=0, ws=None, ws_bytes=0) != INVALID or b"min_edge" not in lib.tsp_last_error()  # not read in that mode
    for bad in (0.0, -1.0, float("nan"), -float("inf")):
        refused(collapse(max_edge=bad), "max_edge")
    for bad in (0, 3, -1, 2 ** 31 - 1):
        refused(collapse(mode=bad), "mode")
    refused(collapse(mode=2), "vertex_limit")
    refused(collapse(totals=None), "totals")
    refused(collapse(out_faces=None), "all")
    refused(collapse(out_keep=None), "all")
    refused(collapse(target=None), "all")
    refused(collapse(out_faces=None, out_keep=None), "all")
    refused(collapse(faces=None), "faces")
    refused(collapse(ev=None), "edge_vertices")
    refused(collapse(state=None), "edge_vertices")
    refused(collapse(removed=None), "edge_vertices")
    refused(collapse(guard=None), "edge_vertices")
    refused(collapse(vertices=None), "vertices")
    refused(collapse(ws=None), "workspace")
    refused(collapse(ws_bytes=lib.tsp_workspace_bytes(10, 20) - 1), "too small")
    refused(collapse(F=0, totals=None), "totals")  # an empty call still needs its totals
    refused(collapse(F=0, out_faces=None), "all")


def test_python_module_checks_its_arguments():
    import torch
    import diff_recon_hip
    from diff_recon_hip import mesh_collapse
    assert set(diff_recon_hip._COLLAPSE_NAMES) <= set(mesh_collapse.__all__) and diff_recon_hip.collapse_edges is mesh_collapse.collapse_edges
    assert "mesh_collapse.py" in diff_recon_hip.__doc__ and "libts_collapse.so" in diff_recon_hip.__doc__
    assert mesh_collapse.COLLAPSE_STATES == {"no_edge": ref.NO_EDGE, "not_eligible": ref.NOT_ELIGIBLE, "long_enough": ref.LONG_ENOUGH,
                                             "guarded": ref.GUARDED, "lost": ref.LOST, "collapsed": ref.COLLAPSED}
    assert mesh_collapse.COLLAPSE_GUARDS == {"link": ref.GUARD_LINK, "long": ref.GUARD_LONG, "normal": ref.GUARD_NORMAL, "held": ref.GUARD_HELD}
    for deg in (0.0, 30.0, 45.0, 60.0, 89.0, 90.0):  # the cosine in float64, rounded to fp32 once and clamped: what the reference takes
        assert mesh_collapse.min_cos_of(deg) == float(ref.min_cos_of(deg)) and 0.0 <= mesh_collapse.min_cos_of(deg) <= 1.0
    for deg in (-1.0, 90.5, 180.0, float("nan")):
        with pytest.raises(ValueError):
            mesh_collapse.min_cos_of(deg)
    v = torch.tensor([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 3.0 ** 0.5, 0.0], [4.0, 0.0, 0.0]])
    f = torch.tensor([[0, 1, 2], [0, 1, 3]], dtype=torch.int32)
    with pytest.raises(RuntimeError):  # the kernels have no CPU fallback
        mesh_collapse.collapse_edges(v, f, min_edge=1.0)
    for bad in (dict(), dict(min_edge=1.0, vertex_limit=torch.ones(4)), dict(min_edge=-1.0), dict(min_edge=float("nan")),
                dict(min_edge=1.0, max_edge=0.0), dict(min_edge=1.0, max_edge=float("nan")), dict(min_edge=1.0, max_normal_deg=120.0)):
        with pytest.raises(ValueError):
            mesh_collapse.collapse_edges(v, f, **bad)
    with pytest.raises(RuntimeError):
        mesh_collapse.collapse_edges(v, f, vertex_limit=torch.ones(3))
    with pytest.raises(RuntimeError):
        mesh_collapse.collapse_edges(v, f, min_edge=1.0, pinned=torch.ones(4))  # float: neither bool nor uint8
    with pytest.raises(ValueError):
        mesh_collapse.collapse_short_edges(v, f, min_edge=1.0, max_rounds=0)
    with pytest.raises(ValueError):
        mesh_collapse.isotropic_remesh(v, f, 0.0)
    with pytest.raises(ValueError):
        mesh_collapse.isotropic_remesh(v, f, 1.0, iterations=0)
