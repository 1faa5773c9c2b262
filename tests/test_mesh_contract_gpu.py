"""GPU tests of the quadric-error edge contraction against tests/ref_mesh_contract.py, everything bit for bit and to its capacity:
out_faces, out_keep, vertex_target, out_vertices, out_quadrics, vertex_blend, edge_vertices, edge_state, edge_removed, edge_guard,
edge_cost and edge_position with their fill values, and totals, with and without the face- and vertex-side outputs; the hand
constructions, jittered grids, the lat-long sphere round by round to half its faces in both quadric modes, several scan tiles under a
budget that defers most candidates, a vertex of valence 65 next to one of 64, keep masks and broken faces, seeds, the empty calls,
contract_fused with colours, the example's report, purity and graph replay."""
import numpy as np
import pytest
import torch

import poison
import ref_mesh_collapse as rc
import ref_mesh_contract as ref
import ref_mesh_decimate as rd
import replay

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ref.NAMES
COS_30 = rc.min_cos_of(30.0)
COS_45 = rc.min_cos_of(45.0)
ALL = 1 << 30


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _faces(f):
    return _dev(np.asarray(f, np.int32).reshape(-1, 3))


def _same(got, want, what):
    """Equal shapes, dtypes and BYTES (the sign of a zero and the payload of a NaN count)."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a = np.ascontiguousarray(got).reshape(-1).view(np.uint8)
    b = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    diff = np.nonzero(a != b)[0] // got.dtype.itemsize
    assert len(diff) == 0, (what, len(diff), diff[:5], got.reshape(-1)[diff[:5]], want.reshape(-1)[diff[:5]])


def _gpu_quadrics(v, f, keep=None):
    from diff_recon_hip import vertex_quadrics
    return vertex_quadrics(_dev(np.asarray(v, np.float32).reshape(-1, 3)), _faces(f), None if keep is None else _dev(np.asarray(keep, np.uint8)))


def _gpu_round(v, f, q, budget, keep=None, pinned=None, max_cost=np.inf, max_edge=np.inf, min_cos=1.0, regularization=1e-3, reach=1.0, seed=0,
               classify_only=False):
    from diff_recon_hip import mesh_contract as mc
    fd = _faces(f)
    k = None if keep is None else _dev(np.asarray(keep, np.uint8))
    p = None if pinned is None else _dev(np.asarray(pinned, np.uint8))
    qd = q if isinstance(q, torch.Tensor) else _dev(np.asarray(q, np.float64).reshape(-1, 10))
    rule = (float(np.float32(max_cost)), float(max_edge), float(min_cos), p)
    return mc._contract_arrays(_dev(np.asarray(v, np.float32).reshape(-1, 3)), fd, k, qd, rule, (float(regularization), float(reach)), int(budget),
                               seed, classify_only, fd.device)


def _assert_round(v, f, q, budget=ALL, what="", **rule):
    """tsu_contract against the reference, every output to its capacity, with and without the face- and vertex-side outputs."""
    want = ref.contract_round(v, f, q, budget, **rule)
    for classify_only in (False, True):
        got = _gpu_round(v, f, q, budget, classify_only=classify_only, **rule)
        assert got[12].tolist() == want["totals"] and got[12].dtype == torch.int64, (what, got[12].tolist(), want["totals"])
        for name, t in zip(NAMES, got[:12]):
            if classify_only and name in ref.FACE_SIDE:
                assert t is None
            else:
                _same(t, want[name], (what, name, classify_only))
    return want


def _assert_mesh(v, f, goal, mode, deg, cos, what="", **rule):
    """Round by round with seed = round index and the budget of contract_mesh, the vertices moving; then contract_mesh as a whole against
    the same, as it stands and compacted, the vertices riding as attributes besides."""
    from diff_recon_hip import contract_mesh
    v0 = np.asarray(v, np.float32)
    v, g, k = v0, np.asarray(f, np.int32).reshape(-1, 3), None
    count = int(ref.takes_part(len(v), g, k).sum())
    target = np.arange(len(v), dtype=np.int32)
    q = rd.vertex_quadrics(v, g, k)
    _same(_gpu_quadrics(v, g, k), q, (what, "quadrics"))
    attr = v0.copy()
    per_round = []
    for r in range(256):
        if count <= goal:
            break
        if mode == "memoryless" and r:
            q = rd.vertex_quadrics(v, g, k)
            _same(_gpu_quadrics(v, g, k), q, (what, "quadrics", r))
        want = _assert_round(v, g, q, (count - goal + 1) // 2, (what, "round", r), keep=k, seed=r, min_cos=cos, **rule)
        if want["totals"][3] == 0:
            break
        per_round.append(want["totals"])
        attr = ref.blend_attributes(attr, want)
        v, g, k, q = want["out_vertices"], want["out_faces"], want["out_keep"], want["out_quadrics"]
        target = want["vertex_target"][target]
        count -= 2 * want["totals"][3]
    kw = dict(target_faces=goal, quadrics=mode, max_normal_deg=deg, max_edge=rule.get("max_edge", np.inf), max_cost=rule.get("max_cost", np.inf),
              regularization=rule.get("regularization", 1e-3), reach=rule.get("reach", 1.0))
    out = contract_mesh(_dev(v0), _faces(f), compact=False, attributes=_dev(v0), **kw)
    final_keep = np.ones(len(g), bool) if k is None else np.asarray(k) != 0
    _same(out.vertices, v, (what, "vertices"))
    _same(out.faces, g, (what, "faces"))
    assert np.array_equal(out.face_keep.cpu().numpy(), final_keep) and out.face_keep.dtype == torch.bool
    _same(out.vertex_map, target, (what, "vertex_map"))
    _same(out.quadrics, q, (what, "quadrics"))
    _same(out.attributes, attr, (what, "attributes"))
    assert out.reached == (count <= goal) == out.stats["reached"] and out.stats["rounds"] == len(per_round) and out.stats["participating_faces"] == count
    assert [[t[n] for n in ref.TOTALS] for t in out.stats["per_round"]] == per_round
    packed = contract_mesh(_dev(v0), _faces(f), compact=True, **kw)
    survives = target == np.arange(len(v))
    new_index = np.cumsum(survives) - 1
    _same(packed.vertices, v[survives], (what, "compact vertices"))
    _same(packed.quadrics, q[survives], (what, "compact quadrics"))
    _same(packed.vertex_map, new_index[target].astype(np.int32), (what, "compact vertex_map"))
    _same(packed.face_map, np.nonzero(final_keep)[0].astype(np.int32), (what, "face_map"))
    part = ref.takes_part(len(v), g) & final_keep
    assert np.array_equal(packed.faces.cpu().numpy()[part[final_keep]], new_index[g[part]].astype(np.int32)) and packed.face_keep is None
    return v, g, k, per_round, count


def spindle(valence=65):
    """Two adjacent hubs A = 0 and B = 1 over an open arc of m + 1 = valence - 1 rim points: A has `valence` ring faces, B one fewer (its
    fan skips the rim point r_1, which the face (r_1, r_0, r_2) closes).  Closed and manifold."""
    m = valence - 2
    a = np.linspace(0.2, 2 * np.pi - 0.2, m + 1)
    rim = np.stack([2 * np.cos(a), 2 * np.sin(a), 0.1 * np.sin(3 * a)], 1)
    v = np.concatenate([[[0.0, 0.0, 1.0], [0.3, 0.0, -1.0]], rim]).astype(np.float32)
    r = lambda i: 2 + i
    f = [(0, r(i), r(i + 1)) for i in range(m)] + [(0, r(m), 1), (0, 1, r(0))]
    f += [(1, r(i + 1), r(i)) for i in range(2, m)] + [(1, r(2), r(0)), (r(1), r(0), r(2))]
    return v, np.array(f, np.int32)


def few_free(v, f, free=(16, 19, 37)):
    """(pinned): every vertex pinned but an independent few -- no two of them adjacent, so no edge has two FREE ends."""
    pinned = np.ones(len(v), np.uint8)
    pinned[list(free)] = 0
    return pinned


# ---- the constructions ----------------------------------------------------------------------------------------------------------------------
def _constructions():
    flat = rd.integer_grid(6)
    even = ((flat[0] * 2).astype(np.float32), flat[1])
    grid = rd.integer_grid(6, raised=(3, 3))
    nan_q = rd.vertex_quadrics(*flat)
    nan_q[24, 5], nan_q[10, 9], nan_q[30, 0], nan_q[17, 9] = np.nan, np.inf, -np.inf, -1e-30
    yield "flat even grid", even, None, dict(min_cos=COS_30)
    yield "raised grid", grid, None, dict(min_cos=0.0)
    yield "raised grid, budget 7", grid, None, dict(min_cos=0.0, budget=7)
    yield "raised grid, budget 1", grid, None, dict(min_cos=0.0, budget=1)
    yield "raised grid, budget 0", grid, None, dict(min_cos=0.0, budget=0)
    yield "reach 0", grid, None, dict(min_cos=0.0, reach=0.0)
    yield "reach half", grid, None, dict(min_cos=0.0, reach=0.5)
    yield "regularization 0", grid, None, dict(min_cos=0.0, regularization=0.0)
    yield "regularization 1", grid, None, dict(min_cos=0.0, regularization=1.0)
    yield "max_cost small", grid, None, dict(min_cos=0.0, max_cost=np.float32(2.0))
    yield "max_cost zero", grid, None, dict(min_cos=0.0, max_cost=0.0)
    yield "bad quadric rows", flat, nan_q, dict(min_cos=COS_30)
    yield "few free", grid, None, dict(min_cos=0.0, pinned=few_free(*grid))
    yield "tetrahedron", rc.TETRAHEDRON, None, dict(min_cos=0.0)
    yield "octahedron", rc.OCTAHEDRON, None, dict(min_cos=0.0)
    yield "fan of 65", rc.fan(65, (1.9, 0.0, 0.0)), None, dict(min_cos=0.0)
    yield "fan of 64", rc.fan(64, (1.9, 0.0, 0.0)), None, dict(min_cos=0.0)
    yield "spindle 65 beside 64", spindle(65), None, dict(min_cos=0.0)
    yield "spindle 64 beside 63", spindle(64), None, dict(min_cos=0.0)
    yield "waisted tube", rc.waisted_tube(), None, dict(min_cos=0.0)
    yield "cube edge", rc.cube_with_edge_vertex(), None, dict(min_cos=COS_30)
    yield "max_edge 2.5", rc.square_fan(), None, dict(min_cos=0.0, max_edge=2.5)
    yield "max_edge 1.5", rc.jittered_grid(7, 7, 0.3, seed=2, z=0.1), None, dict(min_cos=COS_30, max_edge=1.5)
    fan = rc.closed_fan(6, (1.5, 0.0, 0.0))
    yield "closed fan", fan, None, dict(min_cos=COS_30)
    yield "pinned centre", fan, None, dict(min_cos=COS_30, pinned=[1, 0, 0, 0, 0, 0, 0, 0])
    yield "pinned both", fan, None, dict(min_cos=COS_30, pinned=[1, 1, 0, 0, 0, 0, 0, 0])
    yield "masked", fan, None, dict(min_cos=COS_30, keep=[1] * 11 + [0])
    yield "out of range", (fan[0], np.concatenate([fan[1], [[0, 1, 9], [2, 2, 3], [-1, 0, 1]]])), None, dict(min_cos=COS_30)
    for name, bad in (("nan", np.nan), ("inf", -np.inf)):
        w = grid[0].copy()
        w[24, 1] = bad
        yield name, (w, grid[1]), None, dict(min_cos=0.0)
    yield "cube 768", rd.subdivided_cube(8), None, dict(min_cos=COS_30, max_cost=0.0, budget=100)


@pytest.mark.parametrize("name", [c[0] for c in _constructions()])
def test_constructions_match_the_reference_bit_for_bit(name):
    (v, f), q, rule = next((mesh, q, dict(rule)) for n, mesh, q, rule in _constructions() if n == name)
    budget = rule.pop("budget", ALL)
    if q is None:
        q = rd.vertex_quadrics(v, f, rule.get("keep"))
    for seed in (0, 7):
        want = _assert_round(v, f, q, budget, name, seed=seed, **rule)
    E = want["E"]
    if name == "flat even grid":
        assert want["totals"][3] > 0 and (want["edge_cost"][:E][want["rank"] >= 0] == 0).all() and (want["vertex_blend"] > 0).any()
    if name == "tetrahedron":
        assert want["totals"] == [6, 0, 0, 0, 0]
    if name == "octahedron":
        assert want["totals"][:4] == [12, 12, 12, 1]
    if name == "fan of 65":
        assert want["totals"][:2] == [130, 0]
    if name == "spindle 65 beside 64":
        assert not want["vertex_free"][0] and want["vertex_free"][1] and not want["placed"][0]  # edge 0 is (A, B): one FREE end
    if name == "spindle 64 beside 63":
        assert want["vertex_free"][0] and want["vertex_free"][1] and want["placed"][0]
    if name == "raised grid, budget 7":
        assert want["totals"][2] == 7 and (want["edge_state"] == ref.DEFERRED).sum() == want["totals"][1] - 7
    if name == "raised grid, budget 0":
        assert want["totals"][2:4] == [0, 0] and want["out_quadrics"].tobytes() == q.tobytes() and want["out_vertices"].tobytes() == v.tobytes()
    if name == "bad quadric rows":
        assert want["totals"][4] > 0 and not np.signbit(want["edge_cost"]).any()
    if name == "few free":
        assert want["totals"][3] > 0 and not want["placed"].any() and want["out_vertices"].tobytes() == v.tobytes()
    if name == "raised grid":
        assert (want["out_vertices"] != v).any() and want["placed"].any()


# ---- grids and the sphere ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [(1, 1), (2, 2), (3, 3), (7, 7), (17, 17)])
def test_jittered_grids_match_round_by_round(cells):
    """F = 2, 8, 18, 98, 578, to a third of the faces (the outline is held, so small grids stop early)."""
    v, f = rc.jittered_grid(*cells, 0.3, seed={1: 1, 2: 1, 3: 1, 7: 7, 17: 17}[cells[0]], z=0.1)
    assert len(f) == 2 * cells[0] * cells[1]
    w, g, k, per_round, count = _assert_mesh(v, f, len(f) // 3, "carried", 30.0, COS_30, what=cells, max_edge=2.5)
    assert len(per_round) >= {1: 0, 2: 0, 3: 1, 7: 2, 17: 3}[cells[0]]
    print(f"F = {len(f)} -> {count}: {len(per_round)} rounds, collapses {[t[3] for t in per_round]}")


@pytest.mark.parametrize("mode", ["carried", "memoryless"])
def test_sphere_matches_round_by_round_to_half_its_faces(mode):
    v, f = rc.jittered_sphere(12, 16, 0.02, seed=4)
    w, g, k, per_round, count = _assert_mesh(v, f, len(f) // 2, mode, 45.0, COS_45, what=("sphere", mode))
    assert count in (len(f) // 2, len(f) // 2 - 1) and len(per_round) > 5 and (w != v).any()
    print(f"sphere {mode}, {len(f)} -> {count} faces: {len(per_round)} rounds, collapses {[t[3] for t in per_round]}")


def test_several_scan_tiles_and_a_budget_that_defers_most():
    """5000 faces: 15000 edge slots, eight 2048-wide scan tiles and more than one radix block; a budget of 300 defers nine in ten."""
    v, f = rc.jittered_grid(50, 50, 0.3, seed=5, z=0.1)
    assert len(f) == 5000 and -(-3 * len(f) // 2048) == 8
    q = rd.vertex_quadrics(v, f)
    want = _assert_round(v, f, q, 300, "large", min_cos=COS_30, max_edge=2.5)
    t = want["totals"]
    assert t[1] > 3000 and t[2] == 300 and 10 < t[3] <= 300
    assert (want["edge_state"] == ref.DEFERRED).sum() == t[1] - 300


# ---- keep masks, broken faces, seeds --------------------------------------------------------------------------------------------------------
def test_keep_masks_broken_faces_and_seeds_match_the_reference():
    v, f = rc.jittered_grid(17, 17, 0.3, seed=4, z=0.1)
    rng = np.random.default_rng(3)
    keep = (rng.integers(0, 5, len(f)) != 0).astype(np.uint8)
    f = f.copy()
    f[rng.integers(0, len(f), 6)] = [[0, 0, 1], [-1, 2, 3], [1, 2, len(v)], [5, 6, 5], [2 ** 31 - 1, 0, 1], [7, 7, 7]]
    v = v.copy()
    v[rng.integers(0, len(v), 4)] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]]
    pinned = (rng.integers(0, 8, len(v)) == 0).astype(np.uint8)
    for k in (None, keep, np.zeros(len(f), np.uint8)):
        q = rd.vertex_quadrics(v, f, k)
        for seed in (0, 1, 0xFFFFFFFF):
            want = _assert_round(v, f, q, 60, "keep", keep=k, seed=seed, pinned=pinned if seed else None, min_cos=COS_30, max_edge=2.5)
        if k is keep:
            assert want["totals"][3] > 0 and np.array_equal(want["out_faces"][keep == 0], f[keep == 0]) and not want["out_keep"][keep == 0].any()


def test_round_and_classification_through_the_public_calls():
    from diff_recon_hip import contract_round, placed_edges, vertex_quadrics
    v, f = rd.integer_grid(12, raised=(6, 6))
    vd, fd = _dev(v), _faces(f)
    q = vertex_quadrics(vd, fd)
    states = set()
    for seed in range(3):
        r = contract_round(vd, fd, q, 30, max_normal_deg=90.0, seed=seed)
        c = placed_edges(vd, fd, q, 30, max_normal_deg=90.0, seed=seed)
        want = ref.contract_round(v, f, q.cpu().numpy(), 30, min_cos=rc.min_cos_of(90.0), seed=seed)
        E = want["E"]
        assert {n: r.stats[n] for n in ref.TOTALS} == dict(zip(ref.TOTALS, want["totals"]))
        assert r.stats["deferred"] == want["totals"][1] - 30 and r.stats["guarded"] == int((want["edge_state"][:E] == ref.GUARDED).sum())
        won = want["edge_state"][:E] == ref.COLLAPSED
        assert r.stats["max_cost_collapsed"] == want["edge_cost"][:E][won].max()
        for got, name in ((r.edge_state, "edge_state"), (r.edge_vertices, "edge_vertices"), (r.edge_removed, "edge_removed"), (r.edge_guard, "edge_guard"),
                          (r.edge_cost, "edge_cost"), (r.edge_position, "edge_position"), (r.faces, "out_faces"), (r.vertex_target, "vertex_target"),
                          (r.quadrics, "out_quadrics"), (r.vertices, "out_vertices"), (r.vertex_blend, "vertex_blend")):
            _same(got, want[name][:E] if name.startswith("edge") else want[name], name)
        assert np.array_equal(r.face_keep.cpu().numpy(), want["out_keep"] != 0) and int((~r.face_keep).sum()) == 2 * r.stats["collapsed"]
        assert c.faces is None and c.face_keep is None and c.vertex_target is None and c.quadrics is None and c.vertices is None and c.vertex_blend is None
        assert torch.equal(c.edge_state, r.edge_state) and torch.equal(c.edge_cost, r.edge_cost) and c.stats == r.stats
        assert c.edge_position.cpu().numpy().tobytes() == r.edge_position.cpu().numpy().tobytes()
        states.add(r.edge_state.cpu().numpy().tobytes())
    assert len(states) > 1  # flat ties: the seed picks the set


# ---- the empty calls --------------------------------------------------------------------------------------------------------------------------
def test_no_faces_and_no_vertices_write_the_empty_result():
    from diff_recon_hip import contract_mesh, contract_round, placed_edges
    f0 = torch.zeros((0, 3), device=DEV, dtype=torch.int32)
    for V in (0, 5):
        vd = torch.ones((V, 3), device=DEV)
        q = torch.full((V, 10), 3.0, device=DEV, dtype=torch.float64)
        for call in (contract_round, placed_edges):
            r = call(vd, f0, q, 4)
            assert r.edge_vertices.shape == (0, 2) and r.edge_state.shape == r.edge_removed.shape == r.edge_guard.shape == r.edge_cost.shape == (0,)
            assert r.edge_position.shape == (0, 3) and {n: r.stats[n] for n in ref.TOTALS} == dict.fromkeys(ref.TOTALS, 0)
        r = contract_round(vd, f0, q, 4)
        assert r.faces.shape == (0, 3) and r.face_keep.shape == (0,) and r.vertex_target.tolist() == list(range(V)) and torch.equal(r.quadrics, q)
        assert torch.equal(r.vertices, vd) and r.vertex_blend.tolist() == [0.0] * V
        d = contract_mesh(vd, f0, target_faces=0)
        assert d.reached and d.faces.shape == (0, 3) and d.stats["rounds"] == 0 and d.vertices.shape == (V, 3)
    f = np.array([[0, 1, 2], [3, 4, 5], [-1, 7, 2 ** 31 - 1], [0, 0, 0]])  # faces without vertices: nothing takes part, everything is still written
    for keep in (None, [1, 0, 1, 0]):
        want = _assert_round(np.zeros((0, 3), np.float32), f, np.zeros((0, 10)), 3, "V = 0", keep=keep)
        assert want["totals"] == [0, 0, 0, 0, 0] and np.array_equal(want["out_faces"], f.astype(np.int32))
        assert want["out_keep"].tolist() == ([1, 1, 1, 1] if keep is None else keep) and np.isnan(want["edge_position"]).all()


# ---- contract_fused ---------------------------------------------------------------------------------------------------------------------------
def test_contract_fused_returns_the_kind_of_mesh_it_was_given_with_colours_blended():
    from diff_recon_hip import contract_fused, weld_mesh
    from diff_recon_hip.color_volume import ColoredMesh
    v, f = rc.jittered_grid(9, 9, 0.3, seed=7, z=0.1)
    goal = 100
    w, g, k, target, q, per_round, reached = ref.contract_mesh(v, f, goal, min_cos=COS_30)
    assert reached and len(per_round) >= 2 and (w != v).any()
    survives, kept = target == np.arange(len(v)), k != 0
    new_index = np.cumsum(survives) - 1
    colour = np.random.default_rng(3).uniform(0, 1, (len(f), 3)).astype(np.float32)
    m = weld_mesh(_dev(v), _faces(f), _dev(colour), eps=0.0)
    assert torch.equal(m.faces.cpu(), torch.from_numpy(f))
    out = contract_fused(m, target_faces=goal)
    assert type(out) is type(m) and "contract" not in m.stats and out.stats["contract"]["reached"] and out.stats["contract"]["rounds"] == len(per_round)
    _same(out.vertices, w[survives], "vertices")
    _same(out.faces, new_index[g[kept]].astype(np.int32), "faces")
    _same(out.faces_color, colour[kept], "faces_color")
    _same(out.vertex_map, new_index[target][m.vertex_map.cpu().numpy()].astype(np.int32), "vertex_map")
    _same(out.stats["contract"]["quadrics_after"], q[survives], "quadrics")
    assert out.stats["num_vertices"] == int(survives.sum()) and out.stats["num_faces"] == int(kept.sum()) in (goal, goal - 1)
    # colours: one round, every vertex valid -- the reference's blend -- and by validity
    vc = np.random.default_rng(4).uniform(0, 1, (len(v), 3)).astype(np.float32)
    one = ref.contract_round(v, f, rd.vertex_quadrics(v, f), (len(f) - len(f) // 2 + 1) // 2, min_cos=COS_30, seed=0)
    lives = one["vertex_target"] == np.arange(len(v))
    moved = one["vertex_blend"] > 0
    assert moved.sum() >= 3
    c = ColoredMesh(_dev(v), _faces(f), _dev(vc), _dev(np.ones(len(v), bool)), {"num_vertices": len(v), "num_faces": len(f)})
    out = contract_fused(c, ratio=0.5, max_rounds=1)
    assert type(out) is ColoredMesh and not out.stats["contract"]["reached"] and out.color_valid.all() and out.color_valid.dtype == torch.bool
    blended = ref.blend_attributes(vc, one)
    assert (blended[moved] != vc[moved]).any()
    _same(out.vertex_color, blended[lives], "vertex_color")
    _same(out.vertices, one["out_vertices"][lives], "moved vertices")
    _same(out.faces, (np.cumsum(lives) - 1)[one["out_faces"][one["out_keep"] != 0]].astype(np.int32), "one round")
    valid = np.random.default_rng(5).integers(0, 2, len(v)).astype(bool)
    out = contract_fused(c._replace(color_valid=_dev(valid)), ratio=0.5, max_rounds=1)
    r_of = np.full(len(v), -1)
    gone = np.nonzero(~lives)[0]
    r_of[one["vertex_target"][gone]] = gone
    want_c, want_valid = vc.copy(), valid.copy()
    for kk in np.nonzero(moved)[0]:
        rr = r_of[kk]
        if valid[kk] and valid[rr]:
            want_c[kk] = blended[kk]
        elif valid[rr]:
            want_c[kk], want_valid[kk] = vc[rr], True
    _same(out.vertex_color, want_c[lives], "vertex_color by validity")
    assert np.array_equal(out.color_valid.cpu().numpy(), want_valid[lives])
    # a soup has only boundary edges: every vertex is held, nothing collapses, and the report says so
    soup = np.random.default_rng(6).uniform(0, 1, (40, 3, 3)).astype(np.float32)
    s = weld_mesh(_dev(soup.reshape(-1, 3)), _faces(np.arange(120).reshape(-1, 3)), None, eps=0.0)
    out = contract_fused(s, target_faces=10)
    assert not out.stats["contract"]["reached"] and out.stats["contract"]["rounds"] == 0 and out.faces.shape[0] == 40


def test_example_reports_the_mesh_decimated_with_optimal_placement():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    fused = train_synthetic.mesh_scores(m, "2D", extract=24, decimate_faces=200, decimate_placement="optimal", **cfg)["fused"]
    d = fused["decimated"]
    lines = train_synthetic.decimate_faces_report(d)
    print("\n".join(lines))
    assert d["placement"] == "optimal" and d["of"] == "fused" and d["before"]["faces"] == fused["topology"]["faces"] > 400
    assert d["collapses"] > 50 and d["faces"] == d["before"]["faces"] - 2 * d["collapses"] and d["faces"] >= 199
    assert d["vertices"] == d["before"]["vertices"] - d["collapses"] and d["reached"] == (d["faces"] <= 200)
    assert len(lines) == 3 and f"{d['collapses']} quadric-error contractions, survivors placed at the quadric's minimum, in {d['rounds']} rounds" in lines[0]
    assert "against the mesh it came from" in lines[2]
    assert d["to_source"]["hausdorff"] < 0.5 * float(np.linalg.norm(np.ptp(m._vertex.detach().reshape(-1, 3).cpu().numpy(), axis=0)))
    plain = train_synthetic.mesh_scores(m, "2D", weld=0.02, split_edges=20.0, **cfg)["welded"]
    goal = plain["split"]["faces"] - 60
    t = train_synthetic.mesh_scores(m, "2D", weld=0.02, split_edges=20.0, decimate_faces=goal, decimate_placement="optimal", **cfg)["welded"]["decimated"]
    lines = train_synthetic.decimate_faces_report(t)
    print("\n".join(lines))
    assert t["placement"] == "optimal" and t["faces"] == t["before"]["faces"] - 2 * t["collapses"] and t["faces"] >= goal - 1 and t["collapses"] > 0
    assert len(lines) == 3 and "contractions" in lines[0] and f"mean PSNR {t['before']['mean_psnr']:.2f} -> {t['mean_psnr']:.2f} dB" in lines[2]


# ---- determinism and purity -------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_pure_and_deterministic():
    v, f = rc.jittered_grid(17, 17, 0.3, seed=11, z=0.1)
    keep = (np.random.default_rng(8).integers(0, 6, len(f)) != 0).astype(np.uint8)
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]], np.float32)
    rule = dict(min_cos=COS_30, max_edge=2.5, max_cost=np.float32(0.05))

    def call(pattern):  # the workspace and every output come from torch.empty and are poisoned, with guard bytes either side
        out = {}
        for tag, k, classify_only in (("all", None, False), ("kept", keep, False), ("classified", keep, True)):
            q = _gpu_quadrics(v, f, k)
            got = _gpu_round(v, f, q, 25, keep=k, seed=5, classify_only=classify_only, **rule)
            out.update({f"{tag}.{n}": t for n, t in zip(NAMES + ("totals",), got) if t is not None})
        small = _gpu_round(quad, [[0, 1, 2]], _gpu_quadrics(quad, [[0, 1, 2]]), 5)  # the one-face table
        out.update({f"one.{n}": t for n, t in zip(NAMES + ("totals",), small)})
        return out

    base = poison.assert_pure(call)  # twice on zeros first: the same call repeated gives identical bytes
    q = rd.vertex_quadrics(v, f, keep)
    want = ref.contract_round(v, f, q, 25, keep=keep, seed=5, **rule)
    for name in NAMES:
        assert base[f"kept.{name}"].numpy().tobytes() == want[name].tobytes(), name
    assert base["classified.edge_state"].numpy().tobytes() == want["edge_state"].tobytes() and "classified.out_faces" not in base
    assert base["classified.edge_position"].numpy().tobytes() == want["edge_position"].tobytes()
    assert want["totals"][1] > 25 == want["totals"][2] > want["totals"][3] > 0 and want["totals"][4] > 0


# ---- graph replay -----------------------------------------------------------------------------------------------------------------------------
def contract_call(inputs):
    """The quadrics and two rounds in one graph, the second reading the first's out_vertices / out_faces / out_keep / out_quadrics at
    capacity with no host step between; and the classification alone."""
    from diff_recon_hip import mesh_contract as mc
    from diff_recon_hip import mesh_decimate as md
    v, f, keep = inputs["v"], inputs["f"], inputs["keep"]
    rule = (400.0, 20.0, md._min_cos_of(30.0), None)
    place = (1e-3, 1.0)
    names = NAMES + ("totals",)
    q = md._quadrics_of(v, f, keep, DEV)
    first = mc._contract_arrays(v, f, keep, q, rule, place, 40, 7, False, DEV)
    out = dict(zip(names, first), quadrics=q)
    again = mc._contract_arrays(first[3], first[0], first[1], first[4], rule, place, 40, 8, False, DEV)
    out.update({f"{n}_2": t for n, t in zip(names, again)})
    only = mc._contract_arrays(v, f, keep, q, rule, place, 40, 7, True, DEV)
    out.update({f"{n}_classified": t for n, t in zip(names[6:], only[6:])})
    return out


def test_ts_contract_h_replays_from_a_graph():
    from test_graph_replay_gpu import REPLAYS, grid_pair, one_face_pair
    a, b = grid_pair()  # 20 x 20 sheared and jittered, B with every 7th face dropped
    base_a, base_b, n = replay.assert_replays(contract_call, a, b, differ=("totals", "totals_2", "totals_classified", "edge_state", "quadrics", "edge_cost",
                                                                           "edge_position", "out_vertices"))
    assert n == REPLAYS
    ta, tb = base_a["totals"].view(torch.int64).tolist(), base_b["totals"].view(torch.int64).tolist()
    assert ta[3] > 0 and tb[3] > 0 and ta != tb and base_a["totals_2"].view(torch.int64).tolist()[3] > 0
    a, b = one_face_pair()
    base_a, base_b, n = replay.assert_replays(contract_call, a, b, differ=("totals", "edge_state"))
    assert n == REPLAYS and base_a["totals"].view(torch.int64).tolist() == [3, 0, 0, 0, 0] and base_b["totals"].view(torch.int64).tolist() == [0, 0, 0, 0, 0]
