"""CPU tests of the quadric-error decimation (no GPU): the numpy reference of include/ts_decimate.h on integer meshes, where every float64
operation is exact and equalities are exact -- costs, ranks, the budget, the direction rule, the carried quadrics, a cube at max_cost = 0 --
on the guard constructions inherited from the edge collapse, and against a brute-force independence test on Python sets;
libts_decimate.so is a library of its own with exactly the C ABI of the header, and every argument check answers before any HIP call."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_collapse as rc
import ref_mesh_decimate as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_decimate.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tsz_decimate", "tsz_last_error", "tsz_vertex_quadrics", "tsz_workspace_bytes"]
MAX_FACES = 536870911
COS_30 = rc.min_cos_of(30.0)
ALL = 1 << 30  # a budget above every candidate count here


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    return _load("ts2d_abi_decimate", ("diff_triangle_rasterization_2D", "_abi.py"))


DECIMATE_SIGNATURES = _abi_module().DECIMATE_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def decimate_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_decimate.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_decimate.so"
    return path


@pytest.fixture(scope="module")
def lib(decimate_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_decimate(ctypes.CDLL(decimate_path))


def _header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsz_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


def _round(v, f, budget=ALL, quadrics=None, **rule):
    q = ref.vertex_quadrics(v, f, rule.get("keep")) if quadrics is None else quadrics
    return ref.decimate_round(v, f, q, budget, **rule)


def _edges(o):
    """{(lo, hi): (state, removed, guard, cost)} of the round's edge table."""
    E = o["E"]
    return {tuple(e): (int(s), int(r), int(g), float(c)) for e, s, r, g, c in
            zip(o["edge_vertices"][:E].tolist(), o["edge_state"][:E], o["edge_removed"][:E], o["edge_guard"][:E], o["edge_cost"][:E])}


def _fills(o):
    """The capacity beyond E holds the fill values, everything has its shape, and the columns agree with the states."""
    E, F = o["E"], len(o["out_faces"])
    N = 3 * F
    assert o["edge_vertices"].shape == (N, 2) and o["edge_state"].shape == o["edge_removed"].shape == o["edge_guard"].shape == o["edge_cost"].shape == (N,)
    assert o["out_keep"].shape == (F,) and o["out_quadrics"].shape == (len(o["vertex_target"]), 10)
    assert (o["edge_vertices"][E:] == -1).all() and (o["edge_state"][E:] == ref.NO_EDGE).all() and (o["edge_removed"][E:] == -1).all()
    assert (o["edge_guard"][E:] == 0).all() and np.isposinf(o["edge_cost"][E:]).all() and o["totals"][0] == E
    s = o["edge_state"][:E]
    cand = (s == ref.LOST) | (s == ref.COLLAPSED) | (s == ref.DEFERRED)
    assert ((o["edge_removed"][:E] >= 0) == cand).all() and np.isfinite(o["edge_cost"][:E][cand]).all()
    assert (np.signbit(o["edge_cost"][:E]) == 0).all()  # never -0, never negative
    assert np.isposinf(o["edge_cost"][:E][(s == ref.NOT_ELIGIBLE) | (s == ref.GUARDED)]).all() and (o["edge_guard"][:E][s == ref.NOT_ELIGIBLE] == 0).all()
    t = o["totals"]
    assert t[1] == cand.sum() and t[2] == ((s == ref.LOST) | (s == ref.COLLAPSED)).sum() and t[3] == (s == ref.COLLAPSED).sum() and t[4] == (s == ref.TOO_COSTLY).sum()
    assert (o["rank"][cand] >= 0).all() and (o["rank"][~cand] == -1).all()


def _topology(V, faces, keep=None):
    f = np.asarray(faces).reshape(-1, 3)
    if keep is not None:
        f = f[np.asarray(keep) != 0]
    use, parent = {}, list(range(V))

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
            "euler": len(named) - len(use) + len(f), "duplicates": len(triples) - len(set(triples))}


def _check_order(o, seed=0):
    """The ranks of the candidates are a permutation of 0 .. C-1 consistent with (cost ascending, priority descending, edge id ascending);
    every winner and every lost candidate ranks below the budget line, every deferred one at or above it."""
    E = o["E"]
    s, rank, cost = o["edge_state"][:E], o["rank"], o["edge_cost"][:E]
    cand = np.nonzero(rank >= 0)[0]
    assert sorted(rank[cand].tolist()) == list(range(len(cand)))
    prio = rc.priority(o["edge_vertices"][cand, 0], o["edge_vertices"][cand, 1], seed)
    keys = sorted(zip(cost[cand].tolist(), (-prio.astype(np.int64)).tolist(), cand.tolist()))
    assert [k[2] for k in keys] == cand[np.argsort(rank[cand])].tolist()
    return cand, rank, s


# ---- quadrics and costs on integers -------------------------------------------------------------------------------------------------------
def test_flat_integer_grid_costs_nothing():
    v, f = ref.integer_grid(6)
    q = ref.vertex_quadrics(v, f)
    assert q.shape == (49, 10) and (q[:, 6:] == 0).all() and (q[:, :5] == 0).all()  # b = c = 0; the normals are (0, 0, 1) times an area
    assert q[24, 5] == 6.0 and q[0, 5] == 2.0 and q[6, 5] == 1.0  # six faces of doubled area 1 inside, two or one at a corner
    o = _round(v, f, min_cos=COS_30)
    _fills(o)
    E = o["E"]
    cand = o["rank"] >= 0
    assert o["totals"][1] == cand.sum() > 50 and o["totals"][4] == 0
    assert (o["edge_cost"][:E][cand] == 0).all() and not np.signbit(o["edge_cost"][:E][cand]).any()  # every cost is exactly +0
    assert (o["out_quadrics"][:, 6:] == 0).all()  # and a merge of zero-cost collapses in a plane keeps b = c = 0
    assert o["totals"][3] >= 1


def test_raised_vertex_ranks_behind_the_flat_candidates_and_the_budget_line_holds():
    v, f = ref.integer_grid(6, raised=(3, 3))
    q = ref.vertex_quadrics(v, f)
    for budget in (ALL, 40, 7, 1):
        o = ref.decimate_round(v, f, q, budget, min_cos=0.0)
        _fills(o)
        cand, rank, s = _check_order(o)
        cost = o["edge_cost"][:o["E"]]
        zero, positive = cand[cost[cand] == 0], cand[cost[cand] > 0]
        assert len(zero) > 50 and len(positive) >= 10 and rank[zero].max() < rank[positive].min()
        assert set(cost[positive].tolist()) <= {9.0, 36.0}  # distances 3 to planes of doubled area 1, exact
        won, deferred = np.nonzero(s == ref.COLLAPSED)[0], np.nonzero(s == ref.DEFERRED)[0]
        assert (rank[won] < budget).all() and (rank[np.nonzero(s == ref.LOST)[0]] < budget).all() and (rank[deferred] >= budget).all()
        assert len(deferred) == max(0, len(cand) - budget) and 1 <= len(won) <= budget
        assert rank[won].min() == 0  # the first candidate in the order always wins


def test_budget_of_one_of_zero_and_above_the_candidate_count():
    v, f = ref.integer_grid(6, raised=(3, 3))
    q = ref.vertex_quadrics(v, f)
    one = ref.decimate_round(v, f, q, 1, min_cos=0.0)
    s = one["edge_state"][:one["E"]]
    assert one["totals"][2:4] == [1, 1] and one["rank"][s == ref.COLLAPSED].tolist() == [0] and (s == ref.LOST).sum() == 0
    assert one["out_keep"].sum() == len(f) - 2
    none = ref.decimate_round(v, f, q, 0, min_cos=0.0)
    _fills(none)
    assert none["totals"][1] == one["totals"][1] and none["totals"][2:4] == [0, 0] and (none["edge_state"][:none["E"]] == ref.DEFERRED).sum() == none["totals"][1]
    assert none["out_faces"].tobytes() == f.tobytes() and none["out_keep"].all() and none["out_quadrics"].tobytes() == q.tobytes()
    assert none["vertex_target"].tolist() == list(range(len(v)))
    many = ref.decimate_round(v, f, q, one["totals"][1] + 1, min_cos=0.0)
    assert (many["edge_state"] == ref.DEFERRED).sum() == 0 and many["totals"][2] == many["totals"][1]
    exact = ref.decimate_round(v, f, q, one["totals"][1], min_cos=0.0)
    assert exact["edge_state"].tobytes() == many["edge_state"].tobytes()


def test_direction_rule_cheaper_lo_wins_ties_go_to_hi_and_held_ends_are_not_walked():
    v, f = ref.integer_grid(6, raised=(3, 3))
    o = _round(v, f, min_cos=0.0)
    d = o["directions"]
    both = (d["guard"] == 0).all(1) & d["has_cost"].all(1)
    lo_cheaper = np.nonzero(both & (d["cost"][:, 1] < d["cost"][:, 0]))[0]
    hi_cheaper = np.nonzero(both & (d["cost"][:, 0] < d["cost"][:, 1]))[0]
    tied = np.nonzero(both & (d["cost"][:, 0] == d["cost"][:, 1]))[0]
    assert len(lo_cheaper) and len(hi_cheaper) and len(tied)
    ev, removed, cost = o["edge_vertices"], o["edge_removed"], o["edge_cost"]
    for i in lo_cheaper:  # hi -> lo passed its guards, but lo -> hi is cheaper: r = lo
        e = d["edge"][i]
        assert removed[e] == ev[e, 0] and cost[e] == d["cost"][i, 1]
    for i in hi_cheaper:
        e = d["edge"][i]
        assert removed[e] == ev[e, 1] and cost[e] == d["cost"][i, 0]
    for i in tied:
        assert removed[d["edge"][i]] == ev[d["edge"][i], 1]  # equal costs: r = hi
    free = o["vertex_free"]
    for i, e in enumerate(d["edge"]):  # a held end is never walked: it adds the HELD bit and nothing else, and is never removed
        for col, end in ((0, ev[e, 1]), (1, ev[e, 0])):
            assert (d["guard"][i, col] == rc.GUARD_HELD) == (not free[end])
            if not free[end]:
                assert removed[e] != end and not d["has_cost"][i, col]
    # by hand: the raised centre 24 at height 3 and its flat neighbour 23.  Q_23 holds the two tilted faces (23, 24, 17)... evaluated at
    # p_24; Q_24 holds six tilted faces evaluated at p_23.  Removing the peak costs what its own planes say about the plane below.
    edges = _edges(o)
    assert edges[(23, 24)][1] == 23 and edges[(23, 24)][3] == 36.0


def test_max_cost_at_equality_and_one_ulp_below():
    v, f = ref.integer_grid(6, raised=(3, 3))
    at = _round(v, f, min_cos=0.0, max_cost=np.float32(9.0))
    costs = at["edge_cost"][:at["E"]]
    cand = at["rank"] >= 0
    assert 9.0 in set(costs[cand].tolist()) and 36.0 not in set(costs[cand].tolist())  # <= passes at equality
    costly = at["edge_state"][:at["E"]] == ref.TOO_COSTLY
    assert costly.sum() == at["totals"][4] > 0 and set(costs[costly].tolist()) == {36.0} and (at["edge_removed"][:at["E"]][costly] == -1).all()
    below = _round(v, f, min_cos=0.0, max_cost=np.nextafter(np.float32(9.0), np.float32(0.0)))
    _fills(below)
    cand_b = below["rank"] >= 0
    assert set(below["edge_cost"][:below["E"]][cand_b].tolist()) == {0.0}
    assert set(below["edge_cost"][:below["E"]][below["edge_state"][:below["E"]] == ref.TOO_COSTLY].tolist()) == {9.0, 36.0}
    zero = _round(v, f, min_cos=0.0, max_cost=0.0)
    assert zero["totals"][1] == below["totals"][1]


def test_bad_quadric_rows_are_too_costly_and_noise_clamps_to_plus_zero():
    v, f = ref.integer_grid(6)
    q = ref.vertex_quadrics(v, f)
    for bad in (np.nan, np.inf, -np.inf):
        w = q.copy()
        w[24, 5] = bad  # the centre's a22: every direction that removes 24, or lands on it, reads a non-finite value?  only r's A and k's c
        o = ref.decimate_round(v, f, w, ALL, min_cos=COS_30)
        _fills(o)
        for (lo, hi), (state, removed, guard, cost) in _edges(o).items():
            assert removed != 24  # never a candidate through the bad row
        w = q.copy()
        w[:, 9] = bad  # every c: no direction has a cost
        o = ref.decimate_round(v, f, w, ALL, min_cos=COS_30)
        s = o["edge_state"][:o["E"]]
        assert o["totals"][1] == 0 and o["totals"][4] == (s == ref.TOO_COSTLY).sum() > 50 and np.isposinf(o["edge_cost"]).all()
    w = q.copy()
    w[:, 9] = -1e-30  # rounding noise below zero
    o = ref.decimate_round(v, f, w, ALL, min_cos=COS_30)
    cand = o["rank"] >= 0
    assert cand.sum() > 50 and (o["edge_cost"][:o["E"]][cand] == 0).all() and not np.signbit(o["edge_cost"][:o["E"]][cand]).any()
    w[:, 9] = -0.0
    o = ref.decimate_round(v, f, w, ALL, min_cos=COS_30)
    assert not np.signbit(o["edge_cost"]).any()
    won = o["edge_state"][:o["E"]] == ref.COLLAPSED
    k = np.where(o["edge_removed"][:o["E"]][won] == o["edge_vertices"][:o["E"]][won, 0], o["edge_vertices"][:o["E"]][won, 1], o["edge_vertices"][:o["E"]][won, 0])
    w[:, 9] = -1e-30
    o = ref.decimate_round(v, f, w, ALL, min_cos=COS_30)
    assert (o["out_quadrics"][k, 9] == np.float64(-1e-30) + np.float64(-1e-30)).all()  # c_k' gains cost_r unclamped


def test_non_finite_coordinates():
    v, f = ref.integer_grid(6, raised=(3, 3))
    for bad in (np.nan, np.inf):
        w = v.copy()
        w[24, 0] = bad
        q = ref.vertex_quadrics(w, f)
        assert (q[24] == 0).all() and np.isfinite(q).all()  # its own row is zero, and its faces add nothing to their other corners
        assert q[16, 5] == 4.0  # two of the six faces of vertex 16 name vertex 24
        o = ref.decimate_round(w, f, q, ALL, min_cos=0.0)
        _fills(o)
        assert not o["vertex_free"][24]
        for (lo, hi), (state, removed, guard, cost) in _edges(o).items():
            if 24 in (lo, hi):
                assert state == ref.NOT_ELIGIBLE
            assert removed != 24
    empty = ref.decimate_round(np.zeros((0, 3), np.float32), f, np.zeros((0, 10)), 5)
    assert empty["totals"] == [0, 0, 0, 0, 0] and empty["out_faces"].tolist() == f.tolist() and (empty["edge_state"] == ref.NO_EDGE).all()
    assert ref.decimate_round(v, np.zeros((0, 3), np.int32), np.ones((49, 10)), 5)["out_quadrics"].tolist() == np.ones((49, 10)).tolist()
    assert ref.vertex_quadrics(v, np.zeros((0, 3), np.int32)).tolist() == np.zeros((49, 10)).tolist()


# ---- the constructions inherited from the edge collapse -------------------------------------------------------------------------------------
def test_tetrahedron_is_guarded_by_the_link_and_is_never_reached():
    v, f = rc.TETRAHEDRON
    o = _round(v, f, min_cos=0.0)
    _fills(o)
    assert o["vertex_free"].all() and o["totals"] == [6, 0, 0, 0, 0]
    for state, removed, guard, cost in _edges(o).values():
        assert state == ref.GUARDED and removed == -1 and guard & rc.GUARD_LINK and not guard & rc.GUARD_HELD and cost == np.inf
    g, k, target, q, per_round, reached = ref.decimate_mesh(v, f, 2, min_cos=0.0)
    assert not reached and per_round == [] and np.array_equal(g, f)


def test_octahedron_collapses_once_per_round_down_to_the_tetrahedron():
    v, f = rc.OCTAHEDRON
    o = _round(v, f, min_cos=0.0)
    _fills(o)
    assert o["totals"][:4] == [12, 12, 12, 1]  # every vertex lies in the closed ring of every edge: one winner
    t = _topology(6, o["out_faces"], o["out_keep"])
    assert (t["vertices"], t["edges"], t["faces"], t["euler"]) == (5, 9, 6, 2) and t["boundary"] == t["nonmanifold"] == t["duplicates"] == 0
    g, k, target, q, per_round, reached = ref.decimate_mesh(v, f, 4, min_cos=0.0)
    assert reached and [t[3] for t in per_round] == [1, 1] and int(k.sum()) == 4
    g, k, target, q, per_round, reached = ref.decimate_mesh(v, f, 3, min_cos=0.0)  # below the tetrahedron nothing goes
    assert not reached and int(k.sum()) == 4


def test_ring_bound_pins_max_edge_and_masks():
    o = _round(*rc.fan(65, (1.9, 0.0, 0.0)), min_cos=0.0)
    assert o["totals"][:2] == [130, 0] and not o["vertex_free"].any()  # 65 corners at the centre: held, like the rim
    o = _round(*rc.fan(64, (1.9, 0.0, 0.0)), min_cos=0.0)
    assert o["vertex_free"].tolist() == [True] + [False] * 64 and o["totals"][1] > 0
    assert all(r in (-1, 0) for _, r, _, _ in _edges(o).values())
    q = ref.vertex_quadrics(*rc.fan(65, (1.9, 0.0, 0.0)))
    assert q[0, 5] > 0  # the quadrics know no ring cap
    # max_edge: 1 -> 0 of the square fan creates three edges of squared length 6.25 = 2.5^2
    v, f = rc.square_fan()
    assert _edges(_round(v, f, min_cos=0.0, max_edge=2.5))[(0, 1)][:3] in ((ref.COLLAPSED, 1, rc.GUARD_LONG), (ref.COLLAPSED, 1, 0), (ref.LOST, 1, rc.GUARD_LONG), (ref.LOST, 1, 0))
    below = _round(v, f, min_cos=0.0, max_edge=np.nextafter(np.float32(2.5), np.float32(0.0)))
    state, removed, guard, _ = _edges(below)[(0, 1)]
    assert removed != 1 and guard & rc.GUARD_LONG
    # pins
    v, f = rc.closed_fan(6, (1.5, 0.0, 0.0))
    for pinned, never in (([1, 0, 0, 0, 0, 0, 0, 0], 0), ([0, 1, 0, 0, 0, 0, 0, 0], 1)):
        o = _round(v, f, min_cos=COS_30, pinned=pinned)
        _fills(o)
        assert not o["vertex_free"][never] and all(r != never for _, r, _, _ in _edges(o).values())
        assert all(g & rc.GUARD_HELD for (lo, hi), (s, r, g, c) in _edges(o).items() if never in (lo, hi) and s != ref.NOT_ELIGIBLE)
    both = _round(v, f, min_cos=COS_30, pinned=[1, 1, 0, 0, 0, 0, 0, 0])
    assert _edges(both)[(0, 1)][0] == ref.NOT_ELIGIBLE
    masked = _round(v, f, min_cos=COS_30, keep=[1] * 11 + [0])
    _fills(masked)
    assert masked["vertex_free"].tolist() == [True, False, True, True, True, True, False, False] and masked["out_keep"][11] == 0
    g = np.concatenate([f, [[0, 1, 9], [2, 2, 3], [-1, 0, 1]]]).astype(np.int32)
    broken = _round(v, g, min_cos=COS_30)
    assert broken["out_faces"][12:].tolist() == [[0, 1, 9], [2, 2, 3], [-1, 0, 1]] and broken["out_keep"][12:].all()
    assert broken["edge_state"][:broken["E"]].tobytes() == _round(v, f, min_cos=COS_30)["edge_state"][:broken["E"]].tobytes()


# ---- independence and invariants ------------------------------------------------------------------------------------------------------------
def _meshes():
    yield "raised grid", ref.integer_grid(9, raised=(4, 4)), dict(min_cos=COS_30)
    yield "jittered grid", rc.jittered_grid(13, 13, 0.3, seed=3, z=0.1), dict(min_cos=COS_30, max_edge=2.5)
    yield "sphere", rc.jittered_sphere(12, 16, 0.02, seed=4), dict(min_cos=rc.min_cos_of(45.0))


@pytest.mark.parametrize("name", [name for name, _, _ in _meshes()])
def test_winners_are_independent_and_the_round_equals_them_one_by_one(name):
    (v, f), rule = next((mesh, rule) for n, mesh, rule in _meshes() if n == name)
    g, keep, q = f, None, ref.vertex_quadrics(v, f)
    total = 0
    for seed in range(3):
        o = ref.decimate_round(v, g, q, 12, keep=keep, seed=seed, **rule)
        _fills(o)
        _check_order(o, seed)
        E = o["E"]
        kept = g if keep is None else g[keep != 0]
        near = {}
        for a, b, c in kept.tolist():
            for p, r in ((a, b), (b, c), (c, a)):
                near.setdefault(p, set()).add(r)
                near.setdefault(r, set()).add(p)
        winners = [(int(r), int(lo + hi - r)) for (lo, hi), s, r in zip(o["edge_vertices"][:E].tolist(), o["edge_state"][:E], o["edge_removed"][:E]) if s == ref.COLLAPSED]
        assert len(winners) == o["totals"][3] <= 12
        triples = {tuple(sorted(t)) for t in kept.tolist()}
        zones = []
        for r, k in winners:
            common = near[r] & near[k]
            assert len(common) == 2 and all(tuple(sorted((r, k, x))) in triples for x in common)
            assert o["vertex_free"][r]
            zones.append(({r, k}, {r, k} | near[r] | near[k]))
        for i, (ends, _) in enumerate(zones):
            for j, (_, zone) in enumerate(zones):
                assert i == j or not ends & zone
        for order in (winners, winners[::-1]):  # one at a time, in two orders: the faces and the quadrics
            h, hk, hq = g, keep, q.copy()
            for r, k in order:
                h, hk = rc.apply_one(h, hk, r, k)
                Ad, cost_r = ref._cost_of_removed(hq[[r]], v[[k]].astype(np.float64) - v[[r]].astype(np.float64))
                row = hq[k].copy()
                row[:6] = hq[k, :6] + hq[r, :6]
                row[6:9] = hq[k, 6:9] + (Ad[0] + hq[r, 6:9])
                row[9] = hq[k, 9] + cost_r[0]
                hq[k] = row
            hk = np.ones(len(g), np.uint8) if hk is None else hk
            assert np.array_equal(h[hk != 0], o["out_faces"][o["out_keep"] != 0]) and np.array_equal(hk, o["out_keep"])
            assert hq.tobytes() == o["out_quadrics"].tobytes()
        total += len(winners)
        g, keep, q = o["out_faces"], o["out_keep"], o["out_quadrics"]
    assert total >= 3


@pytest.mark.parametrize("mode", ["carried", "memoryless"])
def test_decimate_mesh_keeps_the_counts_the_topology_and_the_budget(mode):
    v, f = rc.jittered_sphere(12, 16, 0.02, seed=4)
    V = len(v)
    start = _topology(V, f)
    assert start["boundary"] == start["nonmanifold"] == 0 and start["euler"] == 2 and start["pieces"] == 1
    for goal in (len(f) // 2, len(f) // 2 + 1, 101):
        g, keep, before, q = f, None, start, ref.vertex_quadrics(v, f)
        count = len(f)
        for seed in range(256):
            if count <= goal:
                break
            if mode == "memoryless" and seed:
                q = ref.vertex_quadrics(v, g, keep)
            o = ref.decimate_round(v, g, q, (count - goal + 1) // 2, keep=keep, seed=seed, min_cos=rc.min_cos_of(45.0))
            n = o["totals"][3]
            if n == 0:
                break
            after = _topology(V, o["out_faces"], o["out_keep"])
            assert (after["vertices"], after["edges"], after["faces"]) == (before["vertices"] - n, before["edges"] - 3 * n, before["faces"] - 2 * n)
            for key in ("pieces", "boundary", "nonmanifold", "euler", "duplicates"):
                assert after[key] == start[key], (key, seed)
            g, keep, q, before, count = o["out_faces"], o["out_keep"], o["out_quadrics"], after, count - 2 * n
        whole = ref.decimate_mesh(v, f, goal, quadrics=mode, min_cos=rc.min_cos_of(45.0))
        assert np.array_equal(whole[0], g) and np.array_equal(whole[1], keep) and whole[3].tobytes() == q.tobytes()
        faces_left = int(whole[1].sum())
        assert whole[5] and goal - 1 <= faces_left <= goal and faces_left == before["faces"]
        assert (whole[2] == np.arange(V)).sum() == before["vertices"]


def test_carried_quadrics_are_the_translated_sums_of_the_initial_ones():
    v, f = ref.integer_grid(8, raised=(4, 4), height=2)
    v[30, 2], v[22, 2], v[50, 2] = 1, -1, 3
    q0 = ref.vertex_quadrics(v, f)
    p = v.astype(np.float64)
    g, keep, q, count, goal = f, None, q0, len(f), 40
    target, paid = np.arange(len(v)), np.zeros(len(v))
    rounds = 0
    while count > goal:
        o = ref.decimate_round(v, g, q, (count - goal + 1) // 2, keep=keep, seed=rounds, min_cos=0.0)
        E = o["E"]
        won = np.nonzero(o["edge_state"][:E] == ref.COLLAPSED)[0]
        assert len(won)
        for e in won:  # c_k' = c_k + cost_r with cost_r unclamped, which holds c_r: what the removed vertex had paid moves on with it
            r = int(o["edge_removed"][e])
            k = int(o["edge_vertices"][e].sum()) - r
            _, cost_r = ref._cost_of_removed(q[[r]], p[[k]] - p[[r]])
            assert cost_r[0] >= paid[r] >= 0
            paid[k] = paid[k] + cost_r[0]
        g, keep, q = o["out_faces"], o["out_keep"], o["out_quadrics"]
        target = o["vertex_target"][target]
        count -= 2 * len(won)
        rounds += 1
    whole = ref.decimate_mesh(v, f, goal, min_cos=0.0)
    assert whole[5] and len(whole[4]) == rounds >= 3 and whole[3].tobytes() == q.tobytes() and np.array_equal(whole[2], target)
    members = {}
    for old, new in enumerate(target.tolist()):
        members.setdefault(new, []).append(old)
    assert sum(len(m) > 2 for m in members.values()) >= 1  # some survivor took more than one vertex: a chain of merges
    for k, merged in members.items():
        want = np.zeros(10)
        for r in merged:  # Q_r in the frame of k: x - p_r = (x - p_k) + t with t = p_k - p_r, so A stays, b gains A t, c gains t A t
            a00, a01, a02, a11, a12, a22 = q0[r, :6]
            A = np.array([[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]])
            t = p[k] - p[r]
            want[:6] += q0[r, :6]
            want[6:9] += A @ t
            want[9] += t @ A @ t
        assert q[k].tolist() == want.tolist(), k  # exact on integers
        assert q[k, 9] == paid[k]                 # and c is the accumulated cost
    assert paid[sorted(members)].sum() > 0  # the budget reached into the raised part: not every collapse was free


def test_subdivided_cube_at_max_cost_zero_keeps_its_shape_exactly():
    v, f = ref.subdivided_cube(8)
    assert len(f) == 768 and ref.signed_volume6(v, f) == 6 * 512
    t0 = _topology(len(v), f)
    assert t0["boundary"] == t0["nonmanifold"] == 0 and t0["euler"] == 2
    g, keep, target, q, per_round, reached = ref.decimate_mesh(v, f, 0, max_cost=0.0, min_cos=COS_30)
    assert not reached and int(keep.sum()) < 768 // 4  # the face count drops
    survivors = np.nonzero(target == np.arange(len(v)))[0]
    corners = [i for i, p in enumerate(v.tolist()) if all(c in (0.0, 8.0) for c in p)]
    assert len(corners) == 8 and set(corners) <= set(survivors.tolist())
    used = np.unique(g[keep != 0])
    assert set(used.tolist()) == set(survivors.tolist())
    assert all(any(c in (0.0, 8.0) for c in v[i].tolist()) for i in used)  # on the cube: no vertex moved
    assert ref.signed_volume6(v, g, keep) == 6 * 512  # in Python integers
    t1 = _topology(len(v), g, keep)
    assert t1["boundary"] == t1["nonmanifold"] == t1["duplicates"] == 0 and t1["euler"] == 2 and t1["pieces"] == 1
    assert all(t[3] <= t[2] for t in per_round)


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(decimate_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsz_last_error.restype = ctypes.c_char_p; "
            "l.tsz_workspace_bytes.restype = ctypes.c_size_t; print(l.tsz_workspace_bytes(100000, 200000) >= 4 * 18 * 3 * 200000, "
            "repr(l.tsz_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, decimate_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(decimate_path):
    out = subprocess.run(["nm", "-D", "--defined-only", decimate_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))
    assert sorted(_header_prototypes()) == NAMES and len(NAMES) == 4
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", decimate_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", decimate_path], capture_output=True, text=True).stdout
    assert "libts_decimate.so" in dynamic
    for other in ("libts2d.so", "libts_collapse.so", "libts_subdivide.so", "libts_flip.so"):
        assert other not in dynamic


def test_header_defines_no_struct_and_states_the_contract():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsv|tsc|tsq|tss|tsh|tsf|tsw|tsa|tsi|tsn|tsx|tsd|tse|tsp)_[a-z0-9_]+)\s*\(", text)
    assert "struct" not in text
    assert re.findall(r"#define (TSZ_\w+) (\d+)", text) == [
        ("TSZ_NO_EDGE", "0"), ("TSZ_NOT_ELIGIBLE", "1"), ("TSZ_TOO_COSTLY", "2"), ("TSZ_GUARDED", "3"), ("TSZ_LOST", "4"), ("TSZ_COLLAPSED", "5"),
        ("TSZ_DEFERRED", "6"), ("TSZ_GUARD_LINK", "1"), ("TSZ_GUARD_LONG", "2"), ("TSZ_GUARD_NORMAL", "4"), ("TSZ_GUARD_HELD", "8"), ("TSZ_MAX_RING", "64")]
    assert [ref.NO_EDGE, ref.NOT_ELIGIBLE, ref.TOO_COSTLY, ref.GUARDED, ref.LOST, ref.COLLAPSED, ref.DEFERRED] == list(range(7))
    collapse = open(os.path.join(ROOT, "include", "ts_collapse.h")).read()  # the guard bits and the ring bound are that header's
    for name, value in (("GUARD_LINK", 1), ("GUARD_LONG", 2), ("GUARD_NORMAL", 4), ("GUARD_HELD", 8), ("MAX_RING", 64), ("NO_EDGE", 0),
                        ("NOT_ELIGIBLE", 1), ("GUARDED", 3), ("LOST", 4), ("COLLAPSED", 5)):
        assert f"#define TSP_{name} {value}\n" in collapse and f"#define TSZ_{name} {value}\n" in open(HEADER).read()
    full = open(HEADER).read()
    for word in ("word for word", "TAKE PART", "ascending (lo, hi)", "CLEAN", "FREE and HELD", "TSZ_MAX_RING = 64", "ELIGIBLE", "without early exit",
                 "a00 a01 a02 a11 a12 a22 b0 b1 b2 c", "OWN FRAME", "y = x - p_v", "ascending corner index", "nine coordinates are finite",
                 "nx nx, nx ny, nx nz, ny ny, ny nz, nz nz", "no square root and no division", "ten zeros", "no ring cap",
                 "(a_i0 dx + a_i1 dy) + a_i2 dz", "cost_r = (dot(d, A_r d) + (dot(b_r, d) + dot(b_r, d))) + c_r", "cost = cost_r + c_k",
                 "HAS NO COST", "becomes +0", "monotone", "both where both ends are FREE", "cost <= (double)max_cost", "a tie goes to r = hi",
                 "TSZ_TOO_COSTLY", "+inf if none", "TSZ_GUARDED", "OR over all its directions", "max_collapses >= 0",
                 "cost ascending as\n * float64, priority descending, edge id ascending", "rank >= max_collapses", "TSZ_DEFERRED",
                 "never collapses more than max_collapses", "the first candidate in the order always wins", "unique\n * ranks",
                 "A_k' = A_k + A_r", "b_k' = b_k + (A_r d + b_r)", "c_k' = c_k + cost_r", "cost_r unclamped", "copied bit for bit", "distance two",
                 "in any order", "to their capacity", "{edges, candidates, in_budget, collapsed, too_costly}", "classifies\n *                  only",
                 "before any HIP call", "8-byte aligned", "536870911", "2147483647", "Monotonic", "three stable 32-bit\n * radix sorts", "Purity",
                 "-ffp-contract=off", "nineteenth"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(DECIMATE_SIGNATURES) and len(declared) == 4
    for name, arity in declared.items():
        assert len(DECIMATE_SIGNATURES[name][1]) == arity, name
    assert declared["tsz_decimate"] == 25 and declared["tsz_vertex_quadrics"] == 9
    abi = _abi_module()
    tables = [getattr(abi, n) for n in dir(abi) if n.endswith("SIGNATURES")]
    assert len(tables) >= 20 and abi.DECIMATE_SIGNATURES in tables
    for a in range(len(tables)):
        for b in range(a + 1, len(tables)):
            assert not set(tables[a]) & set(tables[b])
    args = DECIMATE_SIGNATURES["tsz_decimate"][1]
    assert args[7] == args[9] == args[10] == ctypes.c_float and args[8] == ctypes.c_int32 and args[11] == ctypes.c_uint32 and args[23] == ctypes.c_size_t
    assert DECIMATE_SIGNATURES["tsz_workspace_bytes"][0] == ctypes.c_size_t and DECIMATE_SIGNATURES["tsz_vertex_quadrics"][1][7] == ctypes.c_size_t
    # the prefix is this library's alone
    for path in (os.path.join(ROOT, "include"), os.path.join(ROOT, "triangle-splatting_amd", "csrc")):
        for name in os.listdir(path):
            if "decimate" not in name:
                assert not re.search(r"\btsz_", open(os.path.join(path, name)).read(), flags=re.I), name


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_decimate", ("build.py",))
    assert build.DECIMATE_SOURCES == {"mesh_decimate.hip": ["-ffp-contract=off"], "api_decimate.hip": []} and build.DECIMATE_SHARED == ["radix_sort"]
    assert build.decimate_units() == ["mesh_decimate", "api_decimate"]
    cmd = build.decimate_command("mesh_decimate", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert "-ffp-contract=off" not in build.decimate_command("api_decimate")
    assert build.decimate_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_decimate", "api_decimate", "radix_sort")]
    for others in (build.units(), build.collapse_units(), build.flip_units(), build.subdivide_units(), build.simplify_units()):
        assert not {"mesh_decimate", "api_decimate"} & set(others)
    assert build.DECIMATE_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_decimate.so")
    for header in ("ts_decimate_launch.h", "ts_collapse_round.h", "ts_mesh_edge_ids.h", "ts_mesh_edges.h", "ts_mesh_scan.h", "ts_mesh_common.h",
                   os.path.join("..", "..", "include", "ts_decimate.h")):
        assert header in build.HEADERS and os.path.exists(os.path.join(build.CSRC, header)), header
    with pytest.raises(ValueError):
        build.decimate_command("mesh_collapse")


def test_the_two_collapse_units_share_one_copy_of_the_round(decimate_path):
    build = _load("ts2d_build_decimate2", ("build.py",))
    for unit in ("mesh_decimate", "api_decimate"):
        stamp = open(os.path.join(build.OBJ_DIR, unit + ".o.cmd")).read()
        assert stamp.endswith(" ".join(build.decimate_command(unit, cc=stamp.splitlines()[1].split()[0])))
        assert ("-ffp-contract=off" in stamp) == (unit == "mesh_decimate")
    link = open(build.DECIMATE_LIB + ".cmd").read()
    assert "-soname,libts_decimate.so" in link and "radix_sort.o" in link and "mesh_collapse" not in link
    strip = lambda t: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", t, flags=re.S))
    shared = strip(open(os.path.join(build.CSRC, "ts_collapse_round.h")).read())
    units = {n: strip(open(os.path.join(build.CSRC, n)).read()) for n in ("mesh_collapse.hip", "mesh_decimate.hip")}
    for name in ("records_kernel", "edge_flags_kernel", "vertex_class_kernel", "direction_guards", "priority", "table_has", "lower_bound", "length2",
                 "best_of_edges", "best_of_ring", "decide_winner", "apply_kernel", "identity_kernel"):
        define = r"[\w>*&)]\s+%s\s*\((?:[^;{}()]|\([^;{}()]*\))*\)\s*\{" % name
        assert len(re.findall(define, shared)) == 1, name
        for unit, code in units.items():
            assert not re.findall(define, code), (unit, name)
            assert '#include "ts_collapse_round.h"' in code
    for unit, code in units.items():
        assert "struct D3" not in code and "struct Table" not in code and "0x9E3779B1" not in code
    code = units["mesh_decimate.hip"]
    for used in ("direction_guards(", "priority(", "best_of_edges(", "best_of_ring(", "decide_winner(", "sort_half_edges(", "number_edges(", "count4_into(",
                 "count_into(", "Carver w(", "ts_radix_sort_pairs("):
        assert used in code, used
    assert "atomic" not in code  # the counters go through count_into / count4_into: integer adds, nothing else
    assert not re.search(r"\bmesh_fill\(|\bmesh_copy\(|\bhipMem(?:set|cpy)\w*", code)
    assert not re.search(r"hipMalloc|hipFree|Synchronize", code)
    assert "sqrt" not in code and " / " not in code
    assert not re.search(r"double\s+\w+\[\s*(?:10|6|3)\s*\]", code)  # a quadric is held in named scalars, never in a per-thread array
    resources = open(os.path.join(ROOT, "profiles", "mesh_decimate_resources.txt")).read()
    rows = re.findall(r"^mesh_decimate\s+(\S+)\s+(\d+)/(\d+)/\s*(\d+)/(\d+)", resources, flags=re.M)
    assert {"quadrics_kernel", "classify_kernel", "cost_word_kernel", "rank_kernel", "best_kernel", "best2_kernel", "winners_kernel", "merge_kernel",
            "apply_kernel", "vertex_class_kernel"} <= {r[0] for r in rows}
    assert all(r[2] == "0" for r in rows)  # no kernel uses scratch


def test_size_query_is_monotone_in_both_counts(lib):
    sizes = (0, 1, 2, 3, 63, 682, 683, 1024, 1025, 4097, 100000, 416666, 416667, 833333, 833334, 2499999, 2500000, 2500001, 2600000, 5000000,
             5000001, 5000002)
    for fixed in (0, 1000, 3000000):
        prev_v = prev_f = -1
        for n in sizes:
            by_v, by_f = lib.tsz_workspace_bytes(n, fixed), lib.tsz_workspace_bytes(fixed, n)
            assert by_v >= prev_v and by_f >= prev_f, (n, fixed)
            assert by_f >= 4 * 18 * 3 * n and by_v >= 17 * n  # words per half-edge; four words and a byte per vertex
            prev_v, prev_f = by_v, by_f
    assert lib.tsz_workspace_bytes(-5, -5) == lib.tsz_workspace_bytes(0, 0)
    assert lib.tsz_workspace_bytes(10, 2 ** 31 - 1) == lib.tsz_workspace_bytes(10, MAX_FACES)


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null, aligned stand-in: an argument check never dereferences
    big = 1 << 40

    def refused(rc_, word, code=INVALID):
        assert rc_ == code, rc_
        text = lib.tsz_last_error()
        assert text and word.encode() in text, text

    def decimate(V=10, F=20, vertices=P, faces=P, keep=None, pinned=None, quadrics=P, max_cost=float("inf"), budget=5, max_edge=float("inf"),
                 min_cos=0.5, seed=0, out_faces=P, out_keep=P, target=P, out_q=P, ev=P, state=P, removed=P, guard=P, cost=P, totals=P, ws=P,
                 ws_bytes=big):
        return lib.tsz_decimate(V, F, vertices, faces, keep, pinned, quadrics, max_cost, budget, max_edge, min_cos, seed, out_faces, out_keep,
                                target, out_q, ev, state, removed, guard, cost, totals, ws, ws_bytes, None)

    def quadrics(V=10, F=20, vertices=P, faces=P, keep=None, out=P, ws=P, ws_bytes=big):
        return lib.tsz_vertex_quadrics(V, F, vertices, faces, keep, out, ws, ws_bytes, None)

    for call in (decimate, quadrics):
        refused(call(V=-1), ">= 0")
        refused(call(F=-1), ">= 0")
        refused(call(F=-(2 ** 31)), ">= 0")
        refused(call(F=MAX_FACES + 1), "exceeds", CAPACITY)
        refused(call(V=2 ** 31 - 1, F=1), "V + 3 F", CAPACITY)
        refused(call(V=2 ** 31 - 1 - 3 * 1000 + 1, F=1000), "V + 3 F", CAPACITY)
        refused(call(faces=None), "faces")
        refused(call(vertices=None), "vertices")
        refused(call(ws=None), "workspace")
        refused(call(ws_bytes=lib.tsz_workspace_bytes(10, 20) - 1), "too small")
    refused(quadrics(out=None), "out_quadrics")
    refused(quadrics(out=P + 4), "8-byte")
    refused(decimate(budget=-1), "max_collapses")
    refused(decimate(budget=-(2 ** 31)), "max_collapses")
    for bad in (-1.0, -1e-30, float("nan"), -float("inf")):
        refused(decimate(max_cost=bad), "max_cost")
    for bad in (0.0, -1.0, float("nan"), -float("inf")):
        refused(decimate(max_edge=bad), "max_edge")
    for bad in (1.5, -0.0000001, -1.0, float("nan"), float("inf"), -float("inf")):
        refused(decimate(min_cos=bad), "min_cos")
    refused(decimate(totals=None), "totals")
    for part in ("out_faces", "out_keep", "target", "out_q"):
        refused(decimate(**{part: None}), "all")
    refused(decimate(out_faces=None, out_keep=None, target=None), "all")
    refused(decimate(quadrics=None), "quadrics")
    refused(decimate(quadrics=P + 4), "8-byte")
    refused(decimate(quadrics=P + 1), "8-byte")
    refused(decimate(out_q=P + 4), "8-byte")
    refused(decimate(cost=P + 4), "8-byte")
    for part in ("ev", "state", "removed", "guard", "cost"):
        refused(decimate(**{part: None}), "edge_vertices")
    refused(decimate(F=0, totals=None), "totals")  # an empty call still needs its totals
    refused(decimate(F=0, out_faces=None), "all")


def test_python_module_checks_its_arguments():
    import torch
    import diff_recon_hip
    from diff_recon_hip import mesh_decimate
    assert set(diff_recon_hip._DECIMATE_NAMES) <= set(mesh_decimate.__all__) and diff_recon_hip.decimate_mesh is mesh_decimate.decimate_mesh
    assert "mesh_decimate.py" in diff_recon_hip.__doc__ and "libts_decimate.so" in diff_recon_hip.__doc__
    assert mesh_decimate.DECIMATE_STATES == {"no_edge": ref.NO_EDGE, "not_eligible": ref.NOT_ELIGIBLE, "too_costly": ref.TOO_COSTLY,
                                             "guarded": ref.GUARDED, "lost": ref.LOST, "collapsed": ref.COLLAPSED, "deferred": ref.DEFERRED}
    assert mesh_decimate.DECIMATE_GUARDS == {"link": rc.GUARD_LINK, "long": rc.GUARD_LONG, "normal": rc.GUARD_NORMAL, "held": rc.GUARD_HELD}
    assert mesh_decimate.TOTAL_NAMES == ref.TOTALS
    for deg in (0.0, 30.0, 45.0, 60.0, 89.0, 90.0):
        assert mesh_decimate._min_cos_of(deg) == float(rc.min_cos_of(deg))
    v = torch.tensor([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 3.0 ** 0.5, 0.0], [4.0, 0.0, 0.0]])
    f = torch.tensor([[0, 1, 2], [0, 1, 3]], dtype=torch.int32)
    q = torch.zeros((4, 10), dtype=torch.float64)
    with pytest.raises(RuntimeError):  # the kernels have no CPU fallback
        mesh_decimate.vertex_quadrics(v, f)
    with pytest.raises(RuntimeError):
        mesh_decimate.decimate_round(v, f, q, 1)
    for bad in (dict(max_collapses=-1), dict(max_collapses=1, max_cost=-1.0), dict(max_collapses=1, max_cost=float("nan")),
                dict(max_collapses=1, max_edge=0.0), dict(max_collapses=1, max_normal_deg=120.0)):
        with pytest.raises(ValueError):
            mesh_decimate.decimate_round(v, f, q, **bad)
    with pytest.raises(RuntimeError):
        mesh_decimate.decimate_round(v, f, q.float(), 1)
    with pytest.raises(RuntimeError):
        mesh_decimate.decimate_round(v, f, q[:3], 1)
    with pytest.raises(RuntimeError):
        mesh_decimate.decimate_round(v, f, q, 1, pinned=torch.ones(4))
    for bad in (dict(), dict(target_faces=1, ratio=0.5), dict(ratio=1.5), dict(target_faces=-1), dict(target_faces=1, max_rounds=0),
                dict(target_faces=1, quadrics="fresh")):
        with pytest.raises(ValueError):
            mesh_decimate.decimate_mesh(v, f, **bad)
    with pytest.raises(RuntimeError):  # a finite max_cost needs no target: the call gets as far as the device check
        mesh_decimate.decimate_mesh(v, f, max_cost=1.0)
