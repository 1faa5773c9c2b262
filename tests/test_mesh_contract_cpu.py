"""CPU tests of the quadric-error edge contraction (no GPU): the numpy reference of include/ts_contract.h on integer and dyadic meshes,
where every float64 operation is exact and equalities are exact -- midpoints, +0 costs, the fallback of a singular quadric, the clamp at its
bound, the carried quadrics in the survivor's new frame -- against ref_mesh_decimate where no survivor can move, against a brute-force
independence test that applies the winners one at a time in two orders, and against ref_mesh_decimate's volume on the lat-long sphere;
libts_contract.so is a library of its own with exactly the C ABI of the header, and every argument check answers before any HIP call."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_collapse as rc
import ref_mesh_contract as ref
import ref_mesh_decimate as rd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_contract.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tsu_contract", "tsu_last_error", "tsu_workspace_bytes"]
MAX_FACES = 536870911
COS_30 = rc.min_cos_of(30.0)
COS_45 = rc.min_cos_of(45.0)
ALL = 1 << 30  # a budget above every candidate count here


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    return _load("ts2d_abi_contract", ("diff_triangle_rasterization_2D", "_abi.py"))


CONTRACT_SIGNATURES = _abi_module().CONTRACT_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def contract_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_contract.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_contract.so"
    return path


@pytest.fixture(scope="module")
def lib(contract_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_contract(ctypes.CDLL(contract_path))


def _header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


def _round(v, f, budget=ALL, quadrics=None, **rule):
    q = rd.vertex_quadrics(v, f, rule.get("keep")) if quadrics is None else quadrics
    return ref.contract_round(v, f, q, budget, **rule)


def _edges(o):
    """{(lo, hi): (state, removed, guard, cost)} of the round's edge table."""
    E = o["E"]
    return {tuple(e): (int(s), int(r), int(g), float(c)) for e, s, r, g, c in
            zip(o["edge_vertices"][:E].tolist(), o["edge_state"][:E], o["edge_removed"][:E], o["edge_guard"][:E], o["edge_cost"][:E])}


def _fills(o):
    """The capacity beyond E holds the fill values, everything has its shape, and the columns agree with the states."""
    E, F, V = o["E"], len(o["out_faces"]), len(o["vertex_target"])
    N = 3 * F
    assert o["edge_vertices"].shape == (N, 2) and o["edge_state"].shape == o["edge_removed"].shape == o["edge_guard"].shape == o["edge_cost"].shape == (N,)
    assert o["edge_position"].shape == (N, 3) and o["edge_position"].dtype == np.float32
    assert o["out_keep"].shape == (F,) and o["out_quadrics"].shape == (V, 10) and o["out_vertices"].shape == (V, 3) and o["vertex_blend"].shape == (V,)
    assert o["out_vertices"].dtype == np.float32 and o["vertex_blend"].dtype == np.float64
    assert (o["edge_vertices"][E:] == -1).all() and (o["edge_state"][E:] == ref.NO_EDGE).all() and (o["edge_removed"][E:] == -1).all()
    assert (o["edge_guard"][E:] == 0).all() and np.isposinf(o["edge_cost"][E:]).all() and o["totals"][0] == E
    s = o["edge_state"][:E]
    cand = (s == ref.LOST) | (s == ref.COLLAPSED) | (s == ref.DEFERRED)
    assert ((o["edge_removed"][:E] >= 0) == cand).all() and np.isfinite(o["edge_cost"][:E][cand]).all()
    assert (np.signbit(o["edge_cost"][:E]) == 0).all()  # never -0, never negative
    assert np.isposinf(o["edge_cost"][:E][(s == ref.NOT_ELIGIBLE) | (s == ref.GUARDED)]).all() and (o["edge_guard"][:E][s == ref.NOT_ELIGIBLE] == 0).all()
    # p* of every candidate, the one quiet NaN everywhere else
    assert np.isfinite(o["edge_position"][:E][cand]).all()
    rest = np.ones(N, bool)
    rest[:E] = ~cand
    assert (o["edge_position"][rest].view(np.uint32) == 0x7FC00000).all()
    t = o["totals"]
    assert t[1] == cand.sum() and t[2] == ((s == ref.LOST) | (s == ref.COLLAPSED)).sum() and t[3] == (s == ref.COLLAPSED).sum() and t[4] == (s == ref.TOO_COSTLY).sum()
    assert (o["rank"][cand] >= 0).all() and (o["rank"][~cand] == -1).all()
    assert ((o["vertex_blend"] >= 0) & (o["vertex_blend"] <= 1)).all() and not np.signbit(o["vertex_blend"]).any()


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


def _winners(o):
    """[(r, k, e)] of the round."""
    E = o["E"]
    return [(int(r), int(lo + hi - r), e) for e, ((lo, hi), s, r) in enumerate(zip(o["edge_vertices"][:E].tolist(), o["edge_state"][:E], o["edge_removed"][:E]))
            if s == ref.COLLAPSED]


def even_grid(n=6, **more):
    v, f = rd.integer_grid(n, **more)
    return (v * 2).astype(np.float32), f


# ---- placement on integers ------------------------------------------------------------------------------------------------------------------
def test_flat_even_grid_places_every_survivor_at_the_midpoint_and_costs_nothing():
    v, f = even_grid(6)
    o = _round(v, f, min_cos=COS_30)
    _fills(o)
    E = o["E"]
    cand = o["rank"] >= 0
    placed = o["placed"] & cand
    assert cand.sum() > 50 and placed.sum() > 30 and o["totals"][4] == 0 and o["totals"][3] >= 1
    assert (o["edge_cost"][:E][cand] == 0).all() and not np.signbit(o["edge_cost"][:E][cand]).any()  # every cost is exactly +0
    ev = o["edge_vertices"][:E]
    mid = (v[ev[:, 0]].astype(np.float64) + v[ev[:, 1]].astype(np.float64)) / 2  # odd integers: exact in fp32
    assert o["edge_position"][:E][placed].tobytes() == mid[placed].astype(np.float32).tobytes()
    held = cand & ~o["placed"]
    assert held.sum() > 10  # onto the outline: the survivor stays, bit for bit
    k = ev[held].sum(1) - o["edge_removed"][:E][held]
    assert o["edge_position"][:E][held].tobytes() == v[k].tobytes()
    for r, k, e in _winners(o):
        assert o["out_vertices"][k].tobytes() == o["edge_position"][e].tobytes() and o["out_vertices"][r].tobytes() == v[r].tobytes()
        assert o["vertex_blend"][k] == (0.5 if o["placed"][e] else 0.0)
    assert (o["out_quadrics"][:, 6:] == 0).all()  # in a plane the merged quadric keeps b = c = 0 in the new frame too


def test_reach_zero_is_the_midpoint_bit_for_bit():
    for v, f in (rd.integer_grid(6, raised=(3, 3)), rc.jittered_grid(9, 9, 0.3, seed=2, z=0.2), rc.jittered_sphere(8, 10, 0.02, seed=3)):
        o = _round(v, f, min_cos=0.0, reach=0.0)
        _fills(o)
        E = o["E"]
        placed = o["placed"] & (o["rank"] >= 0)
        assert placed.sum() > 10
        s = o["sides"]
        d = v[s["k"]].astype(np.float64) - v[s["r"]].astype(np.float64)
        mid = np.full((E, 3), np.nan, np.float32)
        mid[s["edge"]] = (v[s["k"]].astype(np.float64) + (-d / 2)).astype(np.float32)
        assert o["edge_position"][:E][placed].tobytes() == mid[placed].tobytes()
        other = _round(v, f, min_cos=0.0, reach=0.0, regularization=0.5)  # and the solve no longer matters
        assert other["edge_position"].tobytes() == o["edge_position"].tobytes() and other["edge_cost"].tobytes() == o["edge_cost"].tobytes()


def test_regularization_zero_on_a_rank_one_quadric_falls_back_to_the_midpoint():
    v, f = even_grid(6)
    q = rd.vertex_quadrics(v, f)
    assert (q[:, :5] == 0).all() and (q[:, 5] > 0).any()  # only a22: rank one
    edge = ref.edge_quadric(q[[24]], q[[23]], v[[23]].astype(np.float64) - v[[24]].astype(np.float64))
    m = np.array([[1.0, 0.0, 0.0]])
    y, solved = ref.solve(edge, m, 0.0)
    assert not solved[0] and y.tolist() == m.tolist()  # det = 0 fails "det > 0"
    y, solved = ref.solve(edge, m, 1e-3)
    assert solved[0] and y[0, 2] == 0.0 and abs(y[0, 0] - 1.0) < 1e-12  # regularised: the plane keeps z, the pull keeps the midpoint
    o = _round(v, f, min_cos=COS_30, regularization=0.0)
    E = o["E"]
    placed = o["placed"] & (o["rank"] >= 0)
    ev = o["edge_vertices"][:E]
    mid = ((v[ev[:, 0]].astype(np.float64) + v[ev[:, 1]].astype(np.float64)) / 2).astype(np.float32)
    assert placed.sum() > 30 and o["edge_position"][:E][placed].tobytes() == mid[placed].tobytes()
    for bad in (np.nan, np.inf, -1.0):  # tr not finite, or not > 0
        w = edge.copy()
        w[0, 0] = bad
        w[0, 5] = 0.5 if bad == -1.0 else w[0, 5]
        y, solved = ref.solve(w, m, 1e-3)
        assert not solved[0] and y.tolist() == m.tolist()


def test_the_clamp_at_h_and_one_ulp_inside():
    d = np.array([[2.0, 0.0, -1.0]])  # m = (-1, 0, 0.5); max |d_i| = 2
    h = 0.5                           # reach 0.25
    for axis, m_axis in ((0, -1.0), (1, 0.0), (2, 0.5)):
        for sign in (1.0, -1.0):
            for off, clamped in ((h, False), (np.nextafter(h, 0.0), False), (np.nextafter(h, 1.0), True), (7.0, True)):
                q = np.zeros((1, 10))
                q[0, [0, 3, 5]] = 1.0  # A = I, lambda = 0: the solve returns -b exactly
                want = np.array([-1.0, 0.0, 0.5])
                want[axis] = m_axis + sign * off
                q[0, 6:9] = -want
                y, solved = ref.solve(q, -0.5 * d, 0.0)
                assert solved[0] and y[0].tolist() == want.tolist()
                got = ref.place(q, d, 0.0, 0.25)[0]
                if clamped:
                    want[axis] = m_axis + sign * h
                assert got.tolist() == want.tolist(), (axis, sign, off)
    # h = 0 where the edge has no extent, whatever the solve says
    q = np.zeros((1, 10))
    q[0, [0, 3, 5]], q[0, 6:9] = 1.0, [3.0, 4.0, 5.0]
    assert ref.place(q, np.zeros((1, 3)), 0.0, 1.0).tobytes() == (-0.5 * np.zeros((1, 3))).tobytes()
    # through a round: the survivor stays within reach of the midpoint, axis by axis, and a smaller reach moves some of them
    v, f = rc.jittered_sphere(8, 10, 0.02, seed=3)
    wide, tight = _round(v, f, min_cos=0.0, reach=1.0), _round(v, f, min_cos=0.0, reach=0.125)
    s = tight["sides"]
    both = tight["placed"][s["edge"]]
    dk = (v[s["k"]].astype(np.float64) - v[s["r"]].astype(np.float64))[both]
    off = tight["unrounded"][s["edge"]][both] - (-0.5 * dk)
    bound = 0.125 * np.abs(dk).max(1)
    assert (np.abs(off) <= bound[:, None]).all() and (np.abs(off) == bound[:, None]).any()
    assert (wide["unrounded"][s["edge"]][both] != tight["unrounded"][s["edge"]][both]).any()


# ---- where no survivor can move, the round is ref_mesh_decimate's ---------------------------------------------------------------------------
def test_with_every_vertex_pinned_but_an_independent_few_the_round_is_the_half_edge_collapse_byte_for_byte():
    for (v, f), stride, rule in ((rd.integer_grid(6, raised=(3, 3)), 3, dict(min_cos=0.0)),
                                 (rc.jittered_grid(9, 9, 0.3, seed=2, z=0.2), 5, dict(min_cos=COS_30, max_edge=2.5)),
                                 (rc.jittered_sphere(8, 10, 0.02, seed=3), 4, dict(min_cos=COS_45, max_cost=np.float32(0.01)))):
        near = {}
        for a, b, c in f.tolist():
            for x, y in ((a, b), (b, c), (c, a)):
                near.setdefault(x, set()).add(y)
                near.setdefault(y, set()).add(x)
        free = []
        for u in range(0, len(v), stride):  # greedily: no two free vertices adjacent, so no edge has two FREE ends
            if not near[u] & set(free):
                free.append(u)
        assert len(free) >= 5
        pinned = np.ones(len(v), np.uint8)
        pinned[free] = 0
        q = rd.vertex_quadrics(v, f)
        for seed in (0, 3):
            for budget in (ALL, 2):
                mine = ref.contract_round(v, f, q, budget, pinned=pinned, seed=seed, **rule)
                theirs = rd.decimate_round(v, f, q, budget, pinned=pinned, seed=seed, **rule)
                _fills(mine)
                assert not mine["placed"].any() and mine["totals"] == theirs["totals"] and mine["totals"][3] >= 1
                for name in ("out_faces", "out_keep", "vertex_target", "out_quadrics", "edge_vertices", "edge_state", "edge_removed", "edge_guard", "edge_cost"):
                    assert mine[name].tobytes() == theirs[name].tobytes(), name
                assert mine["out_vertices"].tobytes() == np.asarray(v, np.float32).tobytes() and (mine["vertex_blend"] == 0).all()


# ---- the guards at p* -------------------------------------------------------------------------------------------------------------------------
def _ring(f, a):
    """[(x, y)] of the ring faces (a, x, y) in the face's own order."""
    out = []
    for t in np.asarray(f).tolist():
        if a in t:
            i = t.index(a)
            out.append((t[(i + 1) % 3], t[(i + 2) % 3]))
    return out


def test_the_normal_guard_fails_on_a_ring_face_of_k_alone():
    v, f = rc.jittered_grid(9, 9, 0.3, seed=2, z=0.25)
    o = _round(v, f, min_cos=rc.min_cos_of(12.0))
    s = o["sides"]
    alone = np.nonzero((s["ring_of_k"] & rc.GUARD_NORMAL != 0) & (s["ring_of_r"] == 0) & o["placed"][s["edge"]])[0]
    assert len(alone) >= 1
    M = np.float64(float(rc.min_cos_of(12.0))) ** 2
    p = v.astype(np.float64)
    for i in alone[:5]:
        e, r, k = s["edge"][i], int(s["r"][i]), int(s["k"][i])
        assert o["edge_state"][e] == ref.GUARDED and o["edge_guard"][e] == rc.GUARD_NORMAL and o["edge_removed"][e] == -1
        assert (o["edge_position"][e].view(np.uint32) == 0x7FC00000).all()
        star = (p[k] + o["unrounded"][e]).astype(np.float32).astype(np.float64)  # a guarded edge reports no position: from the solve

        def turned(a, other):
            bad = 0
            for x, yy in _ring(f, a):
                if other in (x, yy):
                    continue
                n0, n1 = np.cross(p[x] - p[a], p[yy] - p[a]), np.cross(p[x] - star, p[yy] - star)
                Q0, Q1, D = n0 @ n0, n1 @ n1, n0 @ n1
                bad += not (Q1 > 0 and (Q0 == 0 or (D > 0 and D * D >= (M * Q0) * Q1 * (1 + 1e-9))))
            return bad
        assert turned(k, r) >= 1  # by plain numpy, with a hair of slack the other way


def test_long_is_measured_from_the_placed_position():
    v, f = rc.jittered_grid(9, 9, 0.3, seed=2, z=0.2)
    base = _round(v, f, min_cos=0.0)
    s = base["sides"]
    p = v.astype(np.float64)
    checked = 0
    for i in np.nonzero(base["placed"][s["edge"]] & (base["rank"][s["edge"]] >= 0))[0][:8]:
        e, r, k = s["edge"][i], int(s["r"][i]), int(s["k"][i])
        star = base["edge_position"][e].astype(np.float64)
        near = ({x for x, _ in _ring(f, r)} | {x for x, _ in _ring(f, k)}) - {r, k}
        far = max(float(((p[x] - star)[0] ** 2 + (p[x] - star)[1] ** 2) + (p[x] - star)[2] ** 2) for x in near)
        from_k = max(float(((p[x] - p[k]) ** 2).sum()) for x in {x for x, _ in _ring(f, r)} - {k})
        enough = np.float32(np.sqrt(far))
        while np.float64(enough) * np.float64(enough) < far:
            enough = np.nextafter(enough, np.float32(np.inf))
        while np.float64(np.nextafter(enough, np.float32(0))) ** 2 >= far:
            enough = np.nextafter(enough, np.float32(0))
        at = _round(v, f, min_cos=0.0, max_edge=enough)
        below = _round(v, f, min_cos=0.0, max_edge=np.nextafter(enough, np.float32(0)))
        assert not at["edge_guard"][e] & rc.GUARD_LONG and at["edge_position"][e].tobytes() == base["edge_position"][e].tobytes()
        assert below["edge_guard"][e] & rc.GUARD_LONG and below["edge_state"][e] == ref.GUARDED
        checked += far != from_k  # the bound is the placed survivor's, not the half-edge collapse's
    assert checked >= 4


def test_cost_and_guards_are_taken_at_the_rounded_position():
    """The cost of the unrounded solve and the cost at the fp32 position differ in every placed edge tried, and for some of them an fp32
    max_cost lies between the two: the state then follows the rounded one."""
    v, f = rc.jittered_grid(13, 13, 0.3, seed=3, z=0.1)
    q = rd.vertex_quadrics(v, f)
    o = ref.contract_round(v, f, q, ALL, min_cos=0.0)
    s = o["sides"]
    el, p = s["edge"], v.astype(np.float64)
    edge_q = ref.edge_quadric(q[s["r"]], q[s["k"]], p[s["k"]] - p[s["r"]])
    with np.errstate(all="ignore"):
        _, before = ref.quadric_at(edge_q, o["unrounded"][el])
    before = np.where(before > 0, before, 0.0)
    after = o["edge_cost"][el]
    placed = o["placed"][el] & (o["rank"][el] >= 0)
    assert placed.sum() > 300 and (before[placed] != after[placed]).mean() > 0.9
    lo, hi = np.minimum(before, after), np.maximum(before, after)
    t = hi.astype(np.float32)
    t = np.where(t.astype(np.float64) >= hi, np.nextafter(t, np.float32(0)), t)  # the largest fp32 below hi
    between = np.nonzero(placed & (before != after) & (t.astype(np.float64) >= lo) & (t > 0))[0]
    assert len(between) >= 10
    for i in between[:6]:
        bounded = ref.contract_round(v, f, q, ALL, min_cos=0.0, max_cost=t[i])
        want = ref.LOST if after[i] <= np.float64(t[i]) else ref.TOO_COSTLY
        unrounded_says = ref.LOST if before[i] <= np.float64(t[i]) else ref.TOO_COSTLY
        assert want != unrounded_says
        got = bounded["edge_state"][el[i]]
        assert (got in (ref.LOST, ref.COLLAPSED)) == (want == ref.LOST) and (got == ref.TOO_COSTLY) == (want == ref.TOO_COSTLY)
        assert bounded["edge_cost"][el[i]] == after[i]
    # y' is the offset of the fp32 position, not the solve's
    star = (p[s["k"]] + o["unrounded"][el]).astype(np.float32)
    assert o["edge_position"][el][placed].tobytes() == star[placed].tobytes()


# ---- the quadrics follow into the new frame ---------------------------------------------------------------------------------------------------
def test_carried_quadrics_evaluate_to_the_cost_and_the_next_cost_is_the_sum_of_the_original_plane_errors():
    """Integer heights on a grid, every coordinate times 64, and reach = 0: every p* of up to six generations of midpoints is an integer,
    every product and sum exact."""
    v, f = rd.integer_grid(8)
    v[:, 2] = np.random.RandomState(5).randint(-2, 3, len(v))
    v = (v * 64).astype(np.float32)
    q0 = rd.vertex_quadrics(v, f)
    p0 = v.astype(np.float64)
    corner = {}  # vertex -> its original ring faces' (normal, own position)
    for a, b, c in f.tolist():
        for u, x, y in ((a, b, c), (b, c, a), (c, a, b)):
            corner.setdefault(u, []).append(np.cross(p0[x] - p0[u], p0[y] - p0[u]))
    members = {u: [u] for u in range(len(v))}

    def from_scratch(us, at):
        return sum(float(n @ (at - p0[u])) ** 2 for u in us for n in corner[u])

    w, g, keep, q = v, f, None, q0
    second = 0
    for rnd in range(5):
        o = ref.contract_round(w, g, q, 20, keep=keep, seed=rnd, min_cos=0.0, reach=0.0)
        _fills(o)
        won = _winners(o)
        assert won
        for r, k, e in won:
            star = o["edge_position"][e].astype(np.float64)
            assert (star == np.round(star)).all()
            want = from_scratch(members[k] + members[r], star)
            assert o["edge_cost"][e] == want, (rnd, r, k)  # the sum of the ORIGINAL plane errors at p*, recomputed in float64
            assert o["out_quadrics"][k, 9] == want        # Q of the survivor at 0 in its new frame is the cost (unclamped; here >= 0)
            second += (len(members[k]) + len(members[r]) > 2) and want > 0
            members[k] = members[k] + members[r]
        for r, k, e in won:  # and the whole row is the translated sum of the initial rows
            row = np.zeros(10)
            for u in members[k]:
                a00, a01, a02, a11, a12, a22 = q0[u, :6]
                A = np.array([[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]])
                t = o["out_vertices"][k].astype(np.float64) - p0[u]
                row[:6] += q0[u, :6]
                row[6:9] += A @ t
                row[9] += t @ A @ t
            assert o["out_quadrics"][k].tolist() == row.tolist()
        w, g, keep, q = o["out_vertices"], o["out_faces"], o["out_keep"], o["out_quadrics"]
    assert second >= 1  # a second contraction of a moved survivor, at a positive cost


def test_unclamped_cost_goes_into_c_and_noise_clamps_to_plus_zero():
    v, f = even_grid(6)
    q = rd.vertex_quadrics(v, f)
    q[:, 9] = -1e-30
    o = ref.contract_round(v, f, q, ALL, min_cos=COS_30)
    _fills(o)
    cand = o["rank"] >= 0
    assert cand.sum() > 50 and (o["edge_cost"][:o["E"]][cand] == 0).all()
    for r, k, e in _winners(o):
        assert o["out_quadrics"][k, 9] == np.float64(-1e-30) + np.float64(-1e-30)


# ---- blend ------------------------------------------------------------------------------------------------------------------------------------
def test_vertex_blend_lies_in_the_unit_interval_and_is_zero_for_held_survivors():
    v, f = rc.jittered_grid(13, 13, 0.3, seed=3, z=0.1)
    pinned = (np.arange(len(v)) % 5 == 0).astype(np.uint8)  # held vertices inside the sheet too
    o = _round(v, f, min_cos=COS_30, max_edge=2.5, pinned=pinned)
    _fills(o)
    won = _winners(o)
    placed = [(r, k, e) for r, k, e in won if o["placed"][e]]
    held = [(r, k, e) for r, k, e in won if not o["placed"][e]]
    assert len(placed) >= 5 and len(held) >= 1
    for r, k, e in held:
        assert o["vertex_blend"][k] == 0 and o["out_vertices"][k].tobytes() == v[k].tobytes() and not o["vertex_free"][k]
    p = v.astype(np.float64)
    for r, k, e in placed:
        y, d = o["out_vertices"][k].astype(np.float64) - p[k], p[k] - p[r]
        assert o["vertex_blend"][k] == min(max(ref.rc._dot(y[None], -d[None])[0] / ref.rc._dot(d[None], d[None])[0], 0.0), 1.0)
    assert (o["vertex_blend"] > 0).sum() <= len(placed) and (o["vertex_blend"][[r for r, _, _ in won]] == 0).all()
    assert ref.blend_of(np.array([[1.0, 0, 0], [-3.0, 0, 0], [5.0, 0, 0], [1.0, 1.0, 1.0]]),
                        np.array([[2.0, 0, 0], [2.0, 0, 0], [-2.0, 0, 0], [0.0, 0, 0]])).tolist() == [0.0, 1.0, 1.0, 0.0]
    attr = np.arange(len(v), dtype=np.float32)[:, None] * np.ones((1, 2), np.float32)
    mixed = ref.blend_attributes(attr, o)
    for r, k, e in won:
        t = o["vertex_blend"][k]
        assert mixed[k].tolist() == [float(np.float32((1 - t) * k + t * r))] * 2 if t > 0 else mixed[k].tolist() == [float(k)] * 2


# ---- bad values and budgets -------------------------------------------------------------------------------------------------------------------
def test_bad_quadric_rows_non_finite_vertices_and_the_budget_line():
    v, f = even_grid(6)
    q = rd.vertex_quadrics(v, f)
    for bad in (np.nan, np.inf, -np.inf):
        w = q.copy()
        w[24, 5] = bad
        o = ref.contract_round(v, f, w, ALL, min_cos=COS_30)
        _fills(o)
        for (lo, hi), (state, removed, guard, cost) in _edges(o).items():
            assert 24 not in (lo, hi) or removed == -1  # no edge at the bad row has a cost: the edge quadric holds it
        assert o["totals"][4] > 0
        w = q.copy()
        w[:, 9] = bad
        o = ref.contract_round(v, f, w, ALL, min_cos=COS_30)
        assert o["totals"][1] == 0 and o["totals"][4] > 50 and np.isposinf(o["edge_cost"]).all() and np.isnan(o["edge_position"]).all()
    g = rd.integer_grid(6, raised=(3, 3))
    for bad in (np.nan, np.inf):
        w = g[0].copy()
        w[24, 0] = bad
        o = ref.contract_round(w, g[1], rd.vertex_quadrics(w, g[1]), ALL, min_cos=0.0)
        _fills(o)
        assert not o["vertex_free"][24]
        for (lo, hi), (state, removed, guard, cost) in _edges(o).items():
            assert state == ref.NOT_ELIGIBLE if 24 in (lo, hi) else removed != 24
    v, f = g
    q = rd.vertex_quadrics(v, f)
    one = ref.contract_round(v, f, q, 1, min_cos=0.0)
    s = one["edge_state"][:one["E"]]
    assert one["totals"][2:4] == [1, 1] and one["rank"][s == ref.COLLAPSED].tolist() == [0] and (s == ref.LOST).sum() == 0
    assert one["out_keep"].sum() == len(f) - 2
    none = ref.contract_round(v, f, q, 0, min_cos=0.0)
    _fills(none)
    assert none["totals"][1] == one["totals"][1] and none["totals"][2:4] == [0, 0] and (none["edge_state"][:none["E"]] == ref.DEFERRED).sum() == none["totals"][1]
    assert none["out_faces"].tobytes() == f.tobytes() and none["out_keep"].all() and none["out_quadrics"].tobytes() == q.tobytes()
    assert none["out_vertices"].tobytes() == v.tobytes() and (none["vertex_blend"] == 0).all() and none["vertex_target"].tolist() == list(range(len(v)))
    assert np.isfinite(none["edge_position"][:none["E"]][none["rank"] >= 0]).all()  # a deferred candidate still reports where it would go
    many = ref.contract_round(v, f, q, one["totals"][1] + 1, min_cos=0.0)
    assert (many["edge_state"] == ref.DEFERRED).sum() == 0 and many["totals"][2] == many["totals"][1]
    exact = ref.contract_round(v, f, q, one["totals"][1], min_cos=0.0)
    assert exact["edge_state"].tobytes() == many["edge_state"].tobytes()
    empty = ref.contract_round(np.zeros((0, 3), np.float32), f, np.zeros((0, 10)), 5)
    assert empty["totals"] == [0, 0, 0, 0, 0] and empty["out_faces"].tolist() == f.tolist() and (empty["edge_state"] == ref.NO_EDGE).all()
    assert np.isnan(empty["edge_position"]).all() and empty["edge_position"].shape == (3 * len(f), 3)
    nof = ref.contract_round(v, np.zeros((0, 3), np.int32), np.ones((49, 10)), 5)
    assert nof["out_quadrics"].tolist() == np.ones((49, 10)).tolist() and nof["out_vertices"].tobytes() == v.tobytes() and (nof["vertex_blend"] == 0).all()


def test_tetrahedron_octahedron_and_the_ring_bound():
    o = _round(*rc.TETRAHEDRON, min_cos=0.0)
    _fills(o)
    assert o["vertex_free"].all() and o["totals"] == [6, 0, 0, 0, 0]
    for state, removed, guard, cost in _edges(o).values():
        assert state == ref.GUARDED and removed == -1 and guard & rc.GUARD_LINK and not guard & rc.GUARD_HELD
    o = _round(*rc.OCTAHEDRON, min_cos=0.0)
    _fills(o)
    assert o["totals"][:4] == [12, 12, 12, 1] and o["placed"].all()
    t = _topology(6, o["out_faces"], o["out_keep"])
    assert (t["vertices"], t["edges"], t["faces"], t["euler"]) == (5, 9, 6, 2) and t["boundary"] == t["nonmanifold"] == t["duplicates"] == 0
    o = _round(*rc.fan(65, (1.9, 0.0, 0.0)), min_cos=0.0)
    assert o["totals"][:2] == [130, 0] and not o["vertex_free"].any()
    o = _round(*rc.fan(64, (1.9, 0.0, 0.0)), min_cos=0.0)
    assert o["vertex_free"].tolist() == [True] + [False] * 64 and o["totals"][1] > 0 and not o["placed"].any()


# ---- independence and invariants ------------------------------------------------------------------------------------------------------------
def _meshes():
    yield "raised grid", rd.integer_grid(9, raised=(4, 4)), dict(min_cos=COS_30)
    yield "jittered grid", rc.jittered_grid(13, 13, 0.3, seed=3, z=0.1), dict(min_cos=COS_30, max_edge=2.5)
    yield "sphere", rc.jittered_sphere(12, 16, 0.02, seed=4), dict(min_cos=COS_45)


def _one_at_a_time(w, g, keep, q, r, k, star, placed):
    """The contraction of {r, k} alone on the current state, on Python's own terms: faces, the moved vertex, the quadric in its new frame."""
    g, keep = rc.apply_one(g, keep, r, k)
    p = w.astype(np.float64)
    merged = ref.edge_quadric(q[[r]], q[[k]], p[[k]] - p[[r]])
    q = q.copy()
    if placed:
        y = star.astype(np.float64)[None] - p[[k]]
        Ay, cost = ref.quadric_at(merged, y)
        merged[0, 6:9] = merged[0, 6:9] + Ay[0]
        merged[0, 9] = cost[0]
        w = w.copy()
        w[k] = star
    q[k] = merged[0]
    return w, g, keep, q


@pytest.mark.parametrize("name", [name for name, _, _ in _meshes()])
def test_winners_are_independent_and_the_round_equals_them_one_by_one_in_two_orders(name):
    (v, f), rule = next((mesh, rule) for n, mesh, rule in _meshes() if n == name)
    w, g, keep, q = v, f, None, rd.vertex_quadrics(v, f)
    total = moved = 0
    for seed in range(3):
        o = ref.contract_round(w, g, q, 12, keep=keep, seed=seed, **rule)
        _fills(o)
        kept = g if keep is None else g[keep != 0]
        near = {}
        for a, b, c in kept.tolist():
            for x, y in ((a, b), (b, c), (c, a)):
                near.setdefault(x, set()).add(y)
                near.setdefault(y, set()).add(x)
        winners = _winners(o)
        assert len(winners) == o["totals"][3] <= 12
        triples = {tuple(sorted(t)) for t in kept.tolist()}
        zones = []
        for r, k, e in winners:
            common = near[r] & near[k]
            assert len(common) == 2 and all(tuple(sorted((r, k, x))) in triples for x in common)
            assert o["vertex_free"][r] and o["placed"][e] == bool(o["vertex_free"][k])
            zones.append(({r, k}, {r, k} | near[r] | near[k]))
        for i, (ends, _) in enumerate(zones):  # no winner has an end inside the closed ring of another winner's ends
            for j, (_, zone) in enumerate(zones):
                assert i == j or not ends & zone
        faces_seen = [{i for i, t in enumerate(g.tolist()) if (keep is None or keep[i]) and (r in t or k in t)} for r, k, _ in winners]
        for i in range(len(winners)):  # so no face whose guard was evaluated has a second moving corner
            for j in range(i + 1, len(winners)):
                assert not faces_seen[i] & faces_seen[j]
        for order in (winners, winners[::-1]):
            hw, hg, hk, hq = w, g, keep, q
            for r, k, e in order:
                hw, hg, hk, hq = _one_at_a_time(hw, hg, hk, hq, r, k, o["edge_position"][e], o["placed"][e])
            hk = np.ones(len(g), np.uint8) if hk is None else hk
            assert np.array_equal(hg[hk != 0], o["out_faces"][o["out_keep"] != 0]) and np.array_equal(hk, o["out_keep"])
            assert hq.tobytes() == o["out_quadrics"].tobytes() and hw.tobytes() == o["out_vertices"].tobytes()
        # and each winner, classified again alone AFTER the others were applied, is the same candidate: nothing it read has changed
        for r, k, e in winners:
            hw, hg, hk, hq = w, g, keep, q
            for r2, k2, e2 in winners:
                if e2 != e:
                    hw, hg, hk, hq = _one_at_a_time(hw, hg, hk, hq, r2, k2, o["edge_position"][e2], o["placed"][e2])
            pinned = np.ones(len(v), np.uint8)
            pinned[[r, k] if o["placed"][e] else [r]] = 0
            again = ref.contract_round(hw, hg, hq, ALL, keep=hk, pinned=pinned, seed=seed, **rule)
            lo, hi = min(r, k), max(r, k)
            state, removed, guard, cost = _edges(again)[(lo, hi)]
            assert state in (ref.LOST, ref.COLLAPSED) and removed == r and cost == o["edge_cost"][e] and guard & ~rc.GUARD_HELD == 0, (r, k)
            at = [i for i, t in enumerate(again["edge_vertices"][:again["E"]].tolist()) if t == [lo, hi]][0]
            assert again["edge_position"][at].tobytes() == o["edge_position"][e].tobytes()
        total += len(winners)
        moved += sum(bool(o["placed"][e]) for _, _, e in winners)
        w, g, keep, q = o["out_vertices"], o["out_faces"], o["out_keep"], o["out_quadrics"]
    assert total >= 3 and moved >= 2


@pytest.mark.parametrize("mode", ["carried", "memoryless"])
def test_contract_mesh_keeps_the_counts_the_topology_and_the_budget(mode):
    v, f = rc.jittered_sphere(12, 16, 0.02, seed=4)
    V = len(v)
    start = _topology(V, f)
    assert start["boundary"] == start["nonmanifold"] == 0 and start["euler"] == 2 and start["pieces"] == 1
    for goal in (len(f) // 2, len(f) // 2 + 1, 101):
        w, g, keep, before, q = v, f, None, start, rd.vertex_quadrics(v, f)
        count = len(f)
        for seed in range(256):
            if count <= goal:
                break
            if mode == "memoryless" and seed:
                q = rd.vertex_quadrics(w, g, keep)
            o = ref.contract_round(w, g, q, (count - goal + 1) // 2, keep=keep, seed=seed, min_cos=COS_45)
            n = o["totals"][3]
            if n == 0:
                break
            after = _topology(V, o["out_faces"], o["out_keep"])
            assert (after["vertices"], after["edges"], after["faces"]) == (before["vertices"] - n, before["edges"] - 3 * n, before["faces"] - 2 * n)
            for key in ("pieces", "boundary", "nonmanifold", "euler", "duplicates"):
                assert after[key] == start[key], (key, seed)
            w, g, keep, q, before, count = o["out_vertices"], o["out_faces"], o["out_keep"], o["out_quadrics"], after, count - 2 * n
        whole = ref.contract_mesh(v, f, goal, quadrics=mode, min_cos=COS_45)
        assert whole[0].tobytes() == w.tobytes() and np.array_equal(whole[1], g) and np.array_equal(whole[2], keep) and whole[4].tobytes() == q.tobytes()
        faces_left = int(whole[2].sum())
        assert whole[6] and goal - 1 <= faces_left <= goal and faces_left == before["faces"]
        assert (whole[3] == np.arange(V)).sum() == before["vertices"]
        assert np.isfinite(whole[0]).all()


def test_placement_keeps_the_volume_of_the_sphere_better_than_the_half_edge_collapse():
    """The lat-long sphere of the decimate tests to a quarter of its faces, both references at their defaults, float64 signed volume.  The
    claim was checked first and holds with no margin invented: 4.0147 (input), 3.8813 (contracted), 3.6212 (half-edge collapses)."""
    v, f = rc.jittered_sphere(12, 16, 0.02, seed=4)
    goal = len(f) // 4
    w, g, keep, _, _, _, reached = ref.contract_mesh(v, f, goal, min_cos=COS_45)
    h, hkeep, _, _, _, hreached = rd.decimate_mesh(v, f, goal, min_cos=COS_45)
    assert reached and hreached and int(keep.sum()) == int(hkeep.sum()) == goal
    full, placed, kept = ref.signed_volume(v, f), ref.signed_volume(w, g, keep), ref.signed_volume(v, h, hkeep)
    print(f"signed volume: input {full:.6f}, contract_mesh {placed:.6f}, decimate_mesh {kept:.6f} at {goal} faces")
    assert abs(placed - full) < abs(kept - full)


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(contract_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsu_last_error.restype = ctypes.c_char_p; "
            "l.tsu_workspace_bytes.restype = ctypes.c_size_t; print(l.tsu_workspace_bytes(100000, 200000) >= 4 * 18 * 3 * 200000, "
            "repr(l.tsu_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, contract_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(contract_path):
    out = subprocess.run(["nm", "-D", "--defined-only", contract_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))
    assert sorted(_header_prototypes()) == NAMES and len(NAMES) == 3
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", contract_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", contract_path], capture_output=True, text=True).stdout
    assert "libts_contract.so" in dynamic
    for other in ("libts2d.so", "libts_collapse.so", "libts_decimate.so", "libts_simplify.so", "libts_flip.so"):
        assert other not in dynamic


def test_header_defines_no_struct_and_states_the_contract():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsv|tsc|tsq|tss|tsh|tsf|tsw|tsa|tsi|tsn|tsx|tsd|tse|tsp|tsz)_[a-z0-9_]+)\s*\(", text)
    assert "struct" not in text
    assert re.findall(r"#define (TSU_\w+) (\d+)", text) == [
        ("TSU_NO_EDGE", "0"), ("TSU_NOT_ELIGIBLE", "1"), ("TSU_TOO_COSTLY", "2"), ("TSU_GUARDED", "3"), ("TSU_LOST", "4"), ("TSU_COLLAPSED", "5"),
        ("TSU_DEFERRED", "6"), ("TSU_GUARD_LINK", "1"), ("TSU_GUARD_LONG", "2"), ("TSU_GUARD_NORMAL", "4"), ("TSU_GUARD_HELD", "8"), ("TSU_MAX_RING", "64")]
    assert [ref.NO_EDGE, ref.NOT_ELIGIBLE, ref.TOO_COSTLY, ref.GUARDED, ref.LOST, ref.COLLAPSED, ref.DEFERRED] == list(range(7))
    full = open(HEADER).read()
    collapse = open(os.path.join(ROOT, "include", "ts_collapse.h")).read()  # the guard bits, the states and the ring bound are that header's
    for name, value in (("GUARD_LINK", 1), ("GUARD_LONG", 2), ("GUARD_NORMAL", 4), ("GUARD_HELD", 8), ("MAX_RING", 64), ("NO_EDGE", 0),
                        ("NOT_ELIGIBLE", 1), ("GUARDED", 3), ("LOST", 4), ("COLLAPSED", 5)):
        assert f"#define TSP_{name} {value}\n" in collapse and f"#define TSU_{name} {value}\n" in full
    for word in ("word for word", "TAKE PART", "ascending (lo, hi)", "CLEAN", "FREE and HELD", "TSU_MAX_RING = 64", "ELIGIBLE", "without early exit",
                 "a00 a01 a02 a11 a12 a22 b0 b1 b2 c", "OWN FRAME", "One decision per eligible EDGE", "k = lo, r = hi", "PLACED", "STAYS at p_k",
                 "d = p_k - p_r", "(a_i0 dx + a_i1 dy) + a_i2 dz", "cost_r = (dot(d, A_r d) + (dot(b_r, d) + dot(b_r, d))) + c_r",
                 "A = A_k + A_r", "b = b_k + (A_r d + b_r)", "c = c_k + cost_r", "m = -0.5 d", "tr = (a00 + a11) + a22", "mu = (double)lambda tr",
                 "r_i = mu m_i - b_i", "det = (a00 c00 + a01 c01) + a02 c02", "y_i = ((c_i0 r0 + c_i1 r1) + c_i2 r2) / det", "Any failed test gives y = m",
                 "h = (double)reach max(|dx|, |dy|, |dz|)", "no square root", "If h is 0, y = m", "bit for bit", "Rounding first",
                 "p* = (float)((double)p_k + y)", "y' = (double)p* - (double)p_k", "cost = (dot(y', A y') + (dot(b, y') + dot(b, y'))) + c",
                 "HAS NO COST", "becomes +0", "monotone", "TSU_GUARD_LINK", "length2(p*, p_x) <= (double)max_edge (double)max_edge",
                 "Q1 > 0 && (Q0 == 0 || (D > 0 && D D >= (M Q0) Q1))", "SURVIVING ring face", "r AND of k", "bounded because k is FREE",
                 "cost <= (double)max_cost", "TSU_TOO_COSTLY", "+inf if\n * it has none", "TSU_GUARDED", "max_collapses >= 0",
                 "cost ascending as float64, priority descending, edge id ascending", "rank >= max_collapses", "TSU_DEFERRED",
                 "never contracts more than max_collapses", "always wins", "unique ranks", "stays independent although k now moves",
                 "exactly one moving corner", "in any order", "the row of k becomes p*", "copied bit for bit", "NEW own frame", "A' = A",
                 "b' = b + A y'", "the cost before the clamp", "t = dot(y', -d) / dot(d, d)", "dot(d, d) == 0 gives t = 0", "(1 - t) attr_k + t attr_r",
                 "to their capacity", "{edges, candidates, in_budget, collapsed, too_costly}", "All six NULL", "0x7FC00000", "before any HIP call",
                 "8-byte\n * aligned", "finite\n * and >= 0", "536870911", "2147483647", "Monotonic", "Purity", "-ffp-contract=off", "twentieth"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(CONTRACT_SIGNATURES) and len(declared) == 3
    for name, arity in declared.items():
        assert len(CONTRACT_SIGNATURES[name][1]) == arity, name
    assert declared["tsu_contract"] == 30
    abi = _abi_module()
    tables = [getattr(abi, n) for n in dir(abi) if n.endswith("SIGNATURES")]
    assert len(tables) >= 21 and abi.CONTRACT_SIGNATURES in tables
    for a in range(len(tables)):
        for b in range(a + 1, len(tables)):
            assert not set(tables[a]) & set(tables[b])
    args = CONTRACT_SIGNATURES["tsu_contract"][1]
    assert args[7] == args[9] == args[10] == args[11] == args[12] == ctypes.c_float and args[8] == ctypes.c_int32 and args[13] == ctypes.c_uint32
    assert args[28] == ctypes.c_size_t and CONTRACT_SIGNATURES["tsu_workspace_bytes"][0] == ctypes.c_size_t
    # the prefix is this library's alone, and the new files name no other library's
    for path in (os.path.join(ROOT, "include"), os.path.join(ROOT, "triangle-splatting_amd", "csrc")):
        for name in os.listdir(path):
            text = open(os.path.join(path, name)).read()
            if "contract" not in name:
                assert not re.search(r"\btsu_", text, flags=re.I), name
            else:
                assert not re.search(r"\b(?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsv|tsc|tsq|tss|tsh|tsf|tsw|tsa|tsi|tsn|tsx|tsd|tse|tsp|tsz)_[a-z0-9_]*\s*\(", text, flags=re.I), name
                assert not re.search(r"\b(?:tsz|tsp|tsq)_", text, flags=re.I), name


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_contract", ("build.py",))
    assert build.CONTRACT_SOURCES == {"mesh_contract.hip": ["-ffp-contract=off"], "api_contract.hip": []} and build.CONTRACT_SHARED == ["radix_sort"]
    assert build.contract_units() == ["mesh_contract", "api_contract"]
    cmd = build.contract_command("mesh_contract", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert "-ffp-contract=off" not in build.contract_command("api_contract")
    assert build.contract_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_contract", "api_contract", "radix_sort")]
    for others in (build.units(), build.collapse_units(), build.decimate_units(), build.flip_units(), build.subdivide_units(), build.simplify_units()):
        assert not {"mesh_contract", "api_contract"} & set(others)
    assert build.CONTRACT_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_contract.so")
    for header in ("ts_contract_launch.h", "ts_collapse_round.h", "ts_mesh_edge_ids.h", "ts_mesh_edges.h", "ts_mesh_scan.h", "ts_mesh_common.h",
                   os.path.join("..", "..", "include", "ts_contract.h")):
        assert header in build.HEADERS and os.path.exists(os.path.join(build.CSRC, header)), header
    with pytest.raises(ValueError):
        build.contract_command("mesh_decimate")


def test_the_unit_shares_the_round_and_keeps_its_quadrics_in_registers(contract_path):
    build = _load("ts2d_build_contract2", ("build.py",))
    for unit in ("mesh_contract", "api_contract"):
        stamp = open(os.path.join(build.OBJ_DIR, unit + ".o.cmd")).read()
        assert stamp.endswith(" ".join(build.contract_command(unit, cc=stamp.splitlines()[1].split()[0])))
        assert ("-ffp-contract=off" in stamp) == (unit == "mesh_contract")
    link = open(build.CONTRACT_LIB + ".cmd").read()
    assert "-soname,libts_contract.so" in link and "radix_sort.o" in link and "mesh_collapse" not in link and "mesh_decimate" not in link
    strip = lambda t: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", t, flags=re.S))
    code = strip(open(os.path.join(build.CSRC, "mesh_contract.hip")).read())
    assert '#include "ts_collapse_round.h"' in code
    for name in ("records_kernel", "edge_flags_kernel", "vertex_class_kernel", "direction_guards", "priority", "table_has", "lower_bound", "length2",
                 "best_of_edges", "best_of_ring", "decide_winner", "apply_kernel", "identity_kernel"):
        define = r"[\w>*&)]\s+%s\s*\((?:[^;{}()]|\([^;{}()]*\))*\)\s*\{" % name
        assert not re.findall(define, code), name
    assert "struct D3" not in code and "struct Table" not in code and "0x9E3779B1" not in code
    for used in ("direction_guards(", "priority(", "best_of_edges(", "best_of_ring(", "decide_winner(", "sort_half_edges(", "number_edges(", "count4_into(",
                 "count_into(", "Carver w(", "ts_radix_sort_pairs(", "table_has(", "apply_kernel", "records_kernel", "vertex_class_kernel"):
        assert used in code, used
    assert "atomic" not in code  # the counters go through count_into / count4_into: integer adds, nothing else
    assert not re.search(r"\bmesh_fill\(|\bmesh_copy\(|\bhipMem(?:set|cpy)\w*", code)
    assert not re.search(r"hipMalloc|hipFree|Synchronize", code)
    assert "sqrt" not in code
    assert not re.search(r"double\s+\w+\[\s*\w*\s*\]", code)  # a quadric is held in named scalars, never in a per-thread array
    resources = open(os.path.join(ROOT, "profiles", "mesh_contract_resources.txt")).read()
    rows = re.findall(r"^mesh_contract\s+(\S+)\s+(\d+)/(\d+)/\s*(\d+)/(\d+)", resources, flags=re.M)
    assert {"classify_kernel", "cost_word_kernel", "rank_kernel", "best_kernel", "best2_kernel", "winners_kernel", "follow_kernel", "apply_kernel",
            "vertex_class_kernel", "begin_kernel"} <= {r[0] for r in rows}
    assert all(r[2] == "0" for r in rows)  # no kernel uses scratch
    # the two units this one shares the round with keep their figures
    for other in ("mesh_collapse", "mesh_decimate"):
        assert re.search(r"^%s\s+classify_kernel\s+\d+/0/64/7" % other, open(os.path.join(ROOT, "profiles", other + "_resources.txt")).read(), flags=re.M)


def test_size_query_is_monotone_in_both_counts(lib):
    sizes = (0, 1, 2, 3, 63, 682, 683, 1024, 1025, 4097, 100000, 416666, 416667, 833333, 833334, 2499999, 2500000, 2500001, 2600000, 5000000,
             5000001, 5000002)
    for fixed in (0, 1000, 3000000):
        prev_v = prev_f = -1
        for n in sizes:
            by_v, by_f = lib.tsu_workspace_bytes(n, fixed), lib.tsu_workspace_bytes(fixed, n)
            assert by_v >= prev_v and by_f >= prev_f, (n, fixed)
            assert by_f >= 4 * 18 * 3 * n and by_v >= 17 * n  # words per half-edge; four words and a byte per vertex
            prev_v, prev_f = by_v, by_f
    assert lib.tsu_workspace_bytes(-5, -5) == lib.tsu_workspace_bytes(0, 0)
    assert lib.tsu_workspace_bytes(10, 2 ** 31 - 1) == lib.tsu_workspace_bytes(10, MAX_FACES)


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null, aligned stand-in: an argument check never dereferences
    big = 1 << 40

    def refused(rc_, word, code=INVALID):
        assert rc_ == code, rc_
        text = lib.tsu_last_error()
        assert text and word.encode() in text, text

    def contract(V=10, F=20, vertices=P, faces=P, keep=None, pinned=None, quadrics=P, max_cost=float("inf"), budget=5, max_edge=float("inf"),
                 min_cos=0.5, lam=1e-3, reach=1.0, seed=0, out_faces=P, out_keep=P, target=P, out_v=P, out_q=P, blend=P, ev=P, state=P, removed=P,
                 guard=P, cost=P, position=P, totals=P, ws=P, ws_bytes=big):
        return lib.tsu_contract(V, F, vertices, faces, keep, pinned, quadrics, max_cost, budget, max_edge, min_cos, lam, reach, seed, out_faces,
                                out_keep, target, out_v, out_q, blend, ev, state, removed, guard, cost, position, totals, ws, ws_bytes, None)

    refused(contract(V=-1), ">= 0")
    refused(contract(F=-1), ">= 0")
    refused(contract(F=-(2 ** 31)), ">= 0")
    refused(contract(F=MAX_FACES + 1), "exceeds", CAPACITY)
    refused(contract(V=2 ** 31 - 1, F=1), "V + 3 F", CAPACITY)
    refused(contract(V=2 ** 31 - 1 - 3 * 1000 + 1, F=1000), "V + 3 F", CAPACITY)
    refused(contract(faces=None), "faces")
    refused(contract(vertices=None), "vertices")
    refused(contract(ws=None), "workspace")
    refused(contract(ws_bytes=lib.tsu_workspace_bytes(10, 20) - 1), "too small")
    refused(contract(budget=-1), "max_collapses")
    refused(contract(budget=-(2 ** 31)), "max_collapses")
    for bad in (-1.0, -1e-30, float("nan"), -float("inf")):
        refused(contract(max_cost=bad), "max_cost")
    for bad in (0.0, -1.0, float("nan"), -float("inf")):
        refused(contract(max_edge=bad), "max_edge")
    for bad in (1.5, -0.0000001, -1.0, float("nan"), float("inf"), -float("inf")):
        refused(contract(min_cos=bad), "min_cos")
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
        refused(contract(lam=bad), "lambda")
        refused(contract(reach=bad), "reach")
    refused(contract(totals=None), "totals")
    for part in ("out_faces", "out_keep", "target", "out_v", "out_q", "blend"):
        refused(contract(**{part: None}), "all")
    refused(contract(out_faces=None, out_keep=None, target=None, out_q=None, blend=None), "all")
    refused(contract(quadrics=None), "quadrics")
    for name in ("quadrics", "out_q", "blend", "cost"):
        refused(contract(**{name: P + 4}), "8-byte")
    refused(contract(quadrics=P + 1), "8-byte")
    for part in ("ev", "state", "removed", "guard", "cost", "position"):
        refused(contract(**{part: None}), "edge_vertices")
    refused(contract(F=0, totals=None), "totals")  # an empty call still needs its totals
    refused(contract(F=0, out_faces=None), "all")


def test_python_module_checks_its_arguments():
    import torch
    import diff_recon_hip
    from diff_recon_hip import mesh_contract
    assert set(diff_recon_hip._CONTRACT_NAMES) <= set(mesh_contract.__all__) and diff_recon_hip.contract_mesh is mesh_contract.contract_mesh
    assert "mesh_contract.py" in diff_recon_hip.__doc__ and "libts_contract.so" in diff_recon_hip.__doc__
    assert mesh_contract.CONTRACT_STATES == {"no_edge": ref.NO_EDGE, "not_eligible": ref.NOT_ELIGIBLE, "too_costly": ref.TOO_COSTLY,
                                             "guarded": ref.GUARDED, "lost": ref.LOST, "collapsed": ref.COLLAPSED, "deferred": ref.DEFERRED}
    assert mesh_contract.CONTRACT_GUARDS == {"link": rc.GUARD_LINK, "long": rc.GUARD_LONG, "normal": rc.GUARD_NORMAL, "held": rc.GUARD_HELD}
    assert mesh_contract.TOTAL_NAMES == ref.TOTALS
    import inspect
    from diff_recon_hip import mesh_decimate
    theirs, mine = inspect.signature(mesh_decimate.decimate_mesh).parameters, inspect.signature(mesh_contract.contract_mesh).parameters
    assert [n for n in mine if n in theirs] == list(theirs) and mine["regularization"].default == 1e-3 and mine["reach"].default == 1.0
    assert all(mine[n].default == theirs[n].default for n in theirs)
    v = torch.tensor([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 3.0 ** 0.5, 0.0], [4.0, 0.0, 0.0]])
    f = torch.tensor([[0, 1, 2], [0, 1, 3]], dtype=torch.int32)
    q = torch.zeros((4, 10), dtype=torch.float64)
    with pytest.raises(RuntimeError):  # the kernels have no CPU fallback
        mesh_contract.contract_round(v, f, q, 1)
    for bad in (dict(max_collapses=-1), dict(max_collapses=1, max_cost=-1.0), dict(max_collapses=1, max_cost=float("nan")),
                dict(max_collapses=1, max_edge=0.0), dict(max_collapses=1, max_normal_deg=120.0), dict(max_collapses=1, regularization=-1.0),
                dict(max_collapses=1, regularization=float("inf")), dict(max_collapses=1, reach=-0.5), dict(max_collapses=1, reach=float("nan"))):
        with pytest.raises(ValueError):
            mesh_contract.contract_round(v, f, q, **bad)
    with pytest.raises(RuntimeError):
        mesh_contract.contract_round(v, f, q.float(), 1)
    with pytest.raises(RuntimeError):
        mesh_contract.placed_edges(v, f, q[:3], 1)
    with pytest.raises(RuntimeError):
        mesh_contract.contract_round(v, f, q, 1, pinned=torch.ones(4))
    for bad in (dict(), dict(target_faces=1, ratio=0.5), dict(ratio=1.5), dict(target_faces=-1), dict(target_faces=1, max_rounds=0),
                dict(target_faces=1, quadrics="fresh"), dict(target_faces=1, reach=-1.0), dict(target_faces=1, regularization=float("nan"))):
        with pytest.raises(ValueError):
            mesh_contract.contract_mesh(v, f, **bad)
    with pytest.raises(RuntimeError):
        mesh_contract.contract_mesh(v, f, target_faces=1, attributes=torch.zeros((4, 2)), attribute_valid=torch.ones(3, dtype=torch.bool))
    with pytest.raises(RuntimeError):  # a finite max_cost needs no target: the call gets as far as the device check
        mesh_contract.contract_mesh(v, f, max_cost=1.0)
    # the blend of one round, on the CPU: both valid, only r valid, only k valid, neither
    attrs = torch.tensor([[0.0], [10.0], [20.0], [30.0], [40.0], [50.0], [60.0], [70.0]])
    target = torch.tensor([0, 0, 2, 2, 4, 4, 6, 6], dtype=torch.int32)  # 1 -> 0, 3 -> 2, 5 -> 4, 7 -> 6
    blend = torch.tensor([0.25, 0, 0.5, 0, 0.5, 0, 0.5, 0], dtype=torch.float64)
    valid = torch.tensor([True, True, False, True, True, False, False, False])
    out, ok = mesh_contract._blend_attributes(attrs, valid, target, blend)
    assert out[:, 0].tolist() == [2.5, 10.0, 30.0, 30.0, 40.0, 50.0, 60.0, 70.0] and ok.tolist() == [True, True, True, True, True, False, False, False]
    out, ok = mesh_contract._blend_attributes(attrs, None, target, blend)
    assert out[:, 0].tolist() == [2.5, 10.0, 25.0, 30.0, 45.0, 50.0, 65.0, 70.0] and ok is None
