"""GPU tests of the quadric-error decimation against tests/ref_mesh_decimate.py, everything bit for bit and to its capacity: the vertex
quadrics, out_faces, out_keep, vertex_target, out_quadrics, edge_vertices, edge_state, edge_removed, edge_guard, edge_cost with their fill
values, and totals, with and without the face-side outputs; the hand constructions, jittered grids, the lat-long sphere round by round to
half its faces in both quadric modes, more scan tiles than a workgroup has lanes under a budget that defers most candidates, a vertex of
valence above 64, keep masks and broken faces, seeds, the empty calls, decimate_fused, purity and graph replay."""
import numpy as np
import pytest
import torch

import poison
import ref_mesh_collapse as rc
import ref_mesh_decimate as ref
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


def _gpu_round(v, f, q, budget, keep=None, pinned=None, max_cost=np.inf, max_edge=np.inf, min_cos=1.0, seed=0, classify_only=False):
    from diff_recon_hip import mesh_decimate as md
    fd = _faces(f)
    k = None if keep is None else _dev(np.asarray(keep, np.uint8))
    p = None if pinned is None else _dev(np.asarray(pinned, np.uint8))
    qd = q if isinstance(q, torch.Tensor) else _dev(np.asarray(q, np.float64).reshape(-1, 10))
    rule = (float(np.float32(max_cost)), float(max_edge), float(min_cos), p)
    return md._decimate_arrays(_dev(np.asarray(v, np.float32).reshape(-1, 3)), fd, k, qd, rule, int(budget), seed, classify_only, fd.device)


def _assert_quadrics(v, f, keep=None, what=""):
    want = ref.vertex_quadrics(v, f, keep)
    _same(_gpu_quadrics(v, f, keep), want, (what, "vertex_quadrics"))
    return want


def _assert_round(v, f, q, budget=ALL, what="", **rule):
    """tsz_decimate against the reference, every output to its capacity, with and without the face-side outputs."""
    want = ref.decimate_round(v, f, q, budget, **rule)
    for classify_only in (False, True):
        got = _gpu_round(v, f, q, budget, classify_only=classify_only, **rule)
        assert got[9].tolist() == want["totals"] and got[9].dtype == torch.int64, (what, got[9].tolist(), want["totals"])
        for name, t in zip(NAMES, got[:9]):
            if classify_only and name in NAMES[:4]:
                assert t is None
            else:
                _same(t, want[name], (what, name, classify_only))
    return want


def _assert_mesh(v, f, goal, mode, deg, cos, what="", keep=None, **rule):
    """Round by round with seed = round index and the budget of decimate_mesh, then decimate_mesh as a whole against the same, as it stands
    and compacted."""
    from diff_recon_hip import decimate_mesh
    v = np.asarray(v, np.float32)
    g, k = np.asarray(f, np.int32).reshape(-1, 3), keep
    count = int(ref.takes_part(len(v), g, k).sum())
    target = np.arange(len(v), dtype=np.int32)
    q = _assert_quadrics(v, g, k, what)
    per_round = []
    for r in range(256):
        if count <= goal:
            break
        if mode == "memoryless" and r:
            q = _assert_quadrics(v, g, k, (what, r))
        want = _assert_round(v, g, q, (count - goal + 1) // 2, (what, "round", r), keep=k, seed=r, min_cos=cos, **rule)
        if want["totals"][3] == 0:
            break
        per_round.append(want["totals"])
        g, k, q = want["out_faces"], want["out_keep"], want["out_quadrics"]
        target = want["vertex_target"][target]
        count -= 2 * want["totals"][3]
    kw = dict(target_faces=goal, quadrics=mode, max_normal_deg=deg, keep=None if keep is None else _dev(np.asarray(keep, np.uint8)),
              max_edge=rule.get("max_edge", np.inf), max_cost=rule.get("max_cost", np.inf))
    out = decimate_mesh(_dev(v), _faces(f), compact=False, **kw)
    final_keep = np.ones(len(g), bool) if k is None else np.asarray(k) != 0
    _same(out.faces, g, (what, "faces"))
    assert np.array_equal(out.face_keep.cpu().numpy(), final_keep) and out.face_keep.dtype == torch.bool
    _same(out.vertex_map, target, (what, "vertex_map"))
    _same(out.quadrics, q, (what, "quadrics"))
    assert out.reached == (count <= goal) == out.stats["reached"] and out.stats["rounds"] == len(per_round) and out.stats["participating_faces"] == count
    assert [[t[n] for n in ref.TOTALS] for t in out.stats["per_round"]] == per_round
    assert all(t["in_budget"] >= t["collapsed"] >= 1 and t["max_cost_collapsed"] >= 0 for t in out.stats["per_round"])
    packed = decimate_mesh(_dev(v), _faces(f), compact=True, attributes=_dev(v), **kw)
    survives = target == np.arange(len(v))
    new_index = np.cumsum(survives) - 1
    _same(packed.vertices, v[survives], (what, "compact vertices"))
    _same(packed.attributes, v[survives], (what, "compact attributes"))
    _same(packed.quadrics, q[survives], (what, "compact quadrics"))
    _same(packed.vertex_map, new_index[target].astype(np.int32), (what, "compact vertex_map"))
    _same(packed.face_map, np.nonzero(final_keep)[0].astype(np.int32), (what, "face_map"))
    part = ref.takes_part(len(v), g) & final_keep
    assert np.array_equal(packed.faces.cpu().numpy()[part[final_keep]], new_index[g[part]].astype(np.int32)) and packed.face_keep is None
    assert packed.stats["num_vertices"] == int(survives.sum()) and packed.stats["num_faces"] == int(final_keep.sum())
    return g, k, per_round, count


# ---- the constructions ----------------------------------------------------------------------------------------------------------------------
def _constructions():
    grid = ref.integer_grid(6, raised=(3, 3))
    nan_q = ref.vertex_quadrics(*ref.integer_grid(6))
    nan_q[24, 5], nan_q[10, 9], nan_q[30, 0], nan_q[17, 9] = np.nan, np.inf, -np.inf, -1e-30
    yield "flat grid", ref.integer_grid(6), None, dict(min_cos=COS_30)
    yield "raised grid", grid, None, dict(min_cos=0.0)
    yield "raised grid, budget 7", grid, None, dict(min_cos=0.0, budget=7)
    yield "raised grid, budget 1", grid, None, dict(min_cos=0.0, budget=1)
    yield "raised grid, budget 0", grid, None, dict(min_cos=0.0, budget=0)
    yield "max_cost at equality", grid, None, dict(min_cos=0.0, max_cost=np.float32(9.0))
    yield "max_cost just below", grid, None, dict(min_cos=0.0, max_cost=np.nextafter(np.float32(9.0), np.float32(0.0)))
    yield "max_cost zero", grid, None, dict(min_cos=0.0, max_cost=0.0)
    yield "bad quadric rows", ref.integer_grid(6), nan_q, dict(min_cos=COS_30)
    yield "tetrahedron", rc.TETRAHEDRON, None, dict(min_cos=0.0)
    yield "octahedron", rc.OCTAHEDRON, None, dict(min_cos=0.0)
    yield "fan of 65", rc.fan(65, (1.9, 0.0, 0.0)), None, dict(min_cos=0.0)
    yield "fan of 64", rc.fan(64, (1.9, 0.0, 0.0)), None, dict(min_cos=0.0)
    yield "waisted tube", rc.waisted_tube(), None, dict(min_cos=0.0)
    yield "cube edge", rc.cube_with_edge_vertex(), None, dict(min_cos=COS_30)
    yield "max_edge at equality", rc.square_fan(), None, dict(min_cos=0.0, max_edge=2.5)
    yield "max_edge just below", rc.square_fan(), None, dict(min_cos=0.0, max_edge=np.nextafter(np.float32(2.5), np.float32(0.0)))
    fan = rc.closed_fan(6, (1.5, 0.0, 0.0))
    yield "pinned centre", fan, None, dict(min_cos=COS_30, pinned=[1, 0, 0, 0, 0, 0, 0, 0])
    yield "pinned both", fan, None, dict(min_cos=COS_30, pinned=[1, 1, 0, 0, 0, 0, 0, 0])
    yield "masked", fan, None, dict(min_cos=COS_30, keep=[1] * 11 + [0])
    yield "out of range", (fan[0], np.concatenate([fan[1], [[0, 1, 9], [2, 2, 3], [-1, 0, 1]]])), None, dict(min_cos=COS_30)
    for name, bad in (("nan", np.nan), ("inf", -np.inf)):
        w = grid[0].copy()
        w[24, 1] = bad
        yield name, (w, grid[1]), None, dict(min_cos=0.0)
    yield "cube 768", ref.subdivided_cube(8), None, dict(min_cos=COS_30, max_cost=0.0, budget=100)


@pytest.mark.parametrize("name", [c[0] for c in _constructions()])
def test_constructions_match_the_reference_bit_for_bit(name):
    (v, f), q, rule = next((mesh, q, dict(rule)) for n, mesh, q, rule in _constructions() if n == name)
    budget = rule.pop("budget", ALL)
    if q is None:
        q = _assert_quadrics(v, f, rule.get("keep"), name)
    for seed in (0, 7):
        want = _assert_round(v, f, q, budget, name, seed=seed, **rule)
    if name == "tetrahedron":
        assert want["totals"] == [6, 0, 0, 0, 0]
    if name == "octahedron":
        assert want["totals"][:4] == [12, 12, 12, 1]
    if name == "fan of 65":
        assert want["totals"][:2] == [130, 0]
    if name == "raised grid, budget 7":
        assert want["totals"][2] == 7 and (want["edge_state"] == ref.DEFERRED).sum() == want["totals"][1] - 7
    if name == "raised grid, budget 0":
        assert want["totals"][2:4] == [0, 0] and want["out_quadrics"].tobytes() == q.tobytes()
    if name == "max_cost just below":
        assert want["totals"][4] > 0
    if name == "bad quadric rows":
        assert want["totals"][4] > 0 and not np.signbit(want["edge_cost"]).any()


def test_quadrics_of_a_vertex_of_valence_above_64():
    for n in (65, 200):
        v, f = rc.closed_fan(n, (0.3, 0.1, 0.5))
        v = (v * np.float32(1.37)).astype(np.float32)  # inexact products: the order of the sum shows
        q = _assert_quadrics(v, f, what=n)
        assert q[0, 5] > 0 and q[0, 0] > 0
        want = _assert_round(v, f, q, ALL, n, min_cos=0.0)
        assert not want["vertex_free"][0] and not want["vertex_free"][n + 1]


# ---- grids and the sphere ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [(1, 1), (2, 2), (3, 3), (7, 7), (17, 17)])
def test_jittered_grids_match_round_by_round(cells):
    """F = 2, 8, 18, 98, 578, to a third of the faces (the outline is held, so small grids stop early)."""
    v, f = rc.jittered_grid(*cells, 0.3, seed={1: 1, 2: 1, 3: 1, 7: 7, 17: 17}[cells[0]], z=0.1)
    assert len(f) == 2 * cells[0] * cells[1]
    g, k, per_round, count = _assert_mesh(v, f, len(f) // 3, "carried", 30.0, COS_30, what=cells, max_edge=2.5)
    assert len(per_round) >= {1: 0, 2: 0, 3: 1, 7: 2, 17: 3}[cells[0]]
    print(f"F = {len(f)} -> {count}: {len(per_round)} rounds, collapses {[t[3] for t in per_round]}")


@pytest.mark.parametrize("mode", ["carried", "memoryless"])
def test_sphere_matches_round_by_round_to_half_its_faces(mode):
    v, f = rc.jittered_sphere(12, 16, 0.02, seed=4)
    g, k, per_round, count = _assert_mesh(v, f, len(f) // 2, mode, 45.0, COS_45, what=("sphere", mode))
    assert count in (len(f) // 2, len(f) // 2 - 1) and len(per_round) > 5
    print(f"sphere {mode}, {len(f)} -> {count} faces: {len(per_round)} rounds, collapses {[t[3] for t in per_round]}")


def test_more_scan_blocks_than_one_workgroup_has_lanes_and_a_budget_that_defers_most():
    """180000 faces: 264 scan tiles of half-edges; every interior edge is a candidate, and a budget of 20000 defers nine in ten."""
    v, f = rc.jittered_grid(300, 300, 0.3, seed=5, z=0.1)
    assert len(f) == 180000 and -(-3 * len(f) // 2048) > 256
    q = _assert_quadrics(v, f, what="large")
    want = _assert_round(v, f, q, 20000, "large", min_cos=COS_30, max_edge=2.5)
    t = want["totals"]
    assert t[1] > 150000 and t[2] == 20000 and 500 < t[3] <= 20000
    assert (want["edge_state"] == ref.DEFERRED).sum() == t[1] - 20000


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
        q = _assert_quadrics(v, f, k, "keep")
        for seed in (0, 1, 0xFFFFFFFF):
            want = _assert_round(v, f, q, 60, "keep", keep=k, seed=seed, pinned=pinned if seed else None, min_cos=COS_30, max_edge=2.5)
        if k is keep:
            assert want["totals"][3] > 0 and np.array_equal(want["out_faces"][keep == 0], f[keep == 0]) and not want["out_keep"][keep == 0].any()


def test_round_and_classification_through_the_public_calls():
    from diff_recon_hip import cheapest_edges, decimate_round, vertex_quadrics
    v, f = ref.integer_grid(12, raised=(6, 6))
    vd, fd = _dev(v), _faces(f)
    q = vertex_quadrics(vd, fd)
    states = set()
    for seed in range(3):
        r = decimate_round(vd, fd, q, 30, max_normal_deg=90.0, seed=seed)
        c = cheapest_edges(vd, fd, q, 30, max_normal_deg=90.0, seed=seed)
        want = ref.decimate_round(v, f, q.cpu().numpy(), 30, min_cos=rc.min_cos_of(90.0), seed=seed)
        E = want["E"]
        assert {n: r.stats[n] for n in ref.TOTALS} == dict(zip(ref.TOTALS, want["totals"]))
        assert r.stats["deferred"] == want["totals"][1] - 30 and r.stats["guarded"] == int((want["edge_state"][:E] == ref.GUARDED).sum())
        won = want["edge_state"][:E] == ref.COLLAPSED
        assert r.stats["max_cost_collapsed"] == want["edge_cost"][:E][won].max()
        for got, name in ((r.edge_state, "edge_state"), (r.edge_vertices, "edge_vertices"), (r.edge_removed, "edge_removed"), (r.edge_guard, "edge_guard"),
                          (r.edge_cost, "edge_cost"), (r.faces, "out_faces"), (r.vertex_target, "vertex_target"), (r.quadrics, "out_quadrics")):
            _same(got, want[name][:E] if name.startswith("edge") else want[name], name)
        assert np.array_equal(r.face_keep.cpu().numpy(), want["out_keep"] != 0) and int((~r.face_keep).sum()) == 2 * r.stats["collapsed"]
        assert c.faces is None and c.face_keep is None and c.vertex_target is None and c.quadrics is None
        assert torch.equal(c.edge_state, r.edge_state) and torch.equal(c.edge_cost, r.edge_cost) and c.stats == r.stats
        states.add(r.edge_state.cpu().numpy().tobytes())
    assert len(states) > 1  # flat ties: the seed picks the set


# ---- the empty calls --------------------------------------------------------------------------------------------------------------------------
def test_no_faces_and_no_vertices_write_the_empty_result():
    from diff_recon_hip import cheapest_edges, decimate_mesh, decimate_round, vertex_quadrics
    f0 = torch.zeros((0, 3), device=DEV, dtype=torch.int32)
    for V in (0, 5):
        vd = torch.ones((V, 3), device=DEV)
        q = torch.full((V, 10), 3.0, device=DEV, dtype=torch.float64)
        assert vertex_quadrics(vd, f0).tolist() == [[0.0] * 10] * V
        for call in (decimate_round, cheapest_edges):
            r = call(vd, f0, q, 4)
            assert r.edge_vertices.shape == (0, 2) and r.edge_state.shape == r.edge_removed.shape == r.edge_guard.shape == r.edge_cost.shape == (0,)
            assert {n: r.stats[n] for n in ref.TOTALS} == dict.fromkeys(ref.TOTALS, 0)
        r = decimate_round(vd, f0, q, 4)
        assert r.faces.shape == (0, 3) and r.face_keep.shape == (0,) and r.vertex_target.tolist() == list(range(V)) and torch.equal(r.quadrics, q)
        d = decimate_mesh(vd, f0, target_faces=0)
        assert d.reached and d.faces.shape == (0, 3) and d.stats["rounds"] == 0 and d.vertices.shape == (V, 3)
    f = np.array([[0, 1, 2], [3, 4, 5], [-1, 7, 2 ** 31 - 1], [0, 0, 0]])  # faces without vertices: nothing takes part, everything is still written
    for keep in (None, [1, 0, 1, 0]):
        want = _assert_round(np.zeros((0, 3), np.float32), f, np.zeros((0, 10)), 3, "V = 0", keep=keep)
        assert want["totals"] == [0, 0, 0, 0, 0] and np.array_equal(want["out_faces"], f.astype(np.int32))
        assert want["out_keep"].tolist() == ([1, 1, 1, 1] if keep is None else keep)
        assert _gpu_quadrics(np.zeros((0, 3), np.float32), f, keep).shape == (0, 10)


# ---- decimate_fused ---------------------------------------------------------------------------------------------------------------------------
def test_decimate_fused_returns_the_kind_of_mesh_it_was_given():
    from diff_recon_hip import decimate_fused, weld_mesh
    from diff_recon_hip.color_volume import ColoredMesh
    v, f = rc.jittered_grid(9, 9, 0.3, seed=7, z=0.1)
    goal = 100
    g, k, target, q, per_round, reached = ref.decimate_mesh(v, f, goal, min_cos=COS_30)
    assert reached and len(per_round) >= 2
    survives, kept = target == np.arange(len(v)), k != 0
    new_index = np.cumsum(survives) - 1
    colour = np.random.default_rng(3).uniform(0, 1, (len(f), 3)).astype(np.float32)
    w = weld_mesh(_dev(v), _faces(f), _dev(colour), eps=0.0)
    assert torch.equal(w.faces.cpu(), torch.from_numpy(f))
    out = decimate_fused(w, target_faces=goal)
    assert type(out) is type(w) and "decimate" not in w.stats and out.stats["decimate"]["reached"] and out.stats["decimate"]["rounds"] == len(per_round)
    _same(out.vertices, v[survives], "vertices")
    _same(out.faces, new_index[g[kept]].astype(np.int32), "faces")
    _same(out.faces_color, colour[kept], "faces_color")
    _same(out.vertex_map, new_index[target][w.vertex_map.cpu().numpy()].astype(np.int32), "vertex_map")
    _same(out.stats["decimate"]["quadrics_after"], q[survives], "quadrics")
    assert out.stats["num_vertices"] == int(survives.sum()) and out.stats["num_faces"] == int(kept.sum()) in (goal, goal - 1)
    vc = np.random.default_rng(4).uniform(0, 1, (len(v), 3)).astype(np.float32)
    valid = np.random.default_rng(5).integers(0, 2, len(v)).astype(bool)
    c = ColoredMesh(_dev(v), _faces(f), _dev(vc), _dev(valid), {"num_vertices": len(v), "num_faces": len(f)})
    out = decimate_fused(c, ratio=0.5, max_rounds=1)
    one = ref.decimate_round(v, f, ref.vertex_quadrics(v, f), (len(f) - len(f) // 2 + 1) // 2, min_cos=COS_30, seed=0)
    lives = one["vertex_target"] == np.arange(len(v))
    assert type(out) is ColoredMesh and not out.stats["decimate"]["reached"]
    _same(out.vertex_color, vc[lives], "vertex_color")
    assert np.array_equal(out.color_valid.cpu().numpy(), valid[lives]) and out.color_valid.dtype == torch.bool
    _same(out.faces, (np.cumsum(lives) - 1)[one["out_faces"][one["out_keep"] != 0]].astype(np.int32), "one round")
    # a soup has only boundary edges: every vertex is held, nothing collapses, and the report says so
    soup = np.random.default_rng(6).uniform(0, 1, (40, 3, 3)).astype(np.float32)
    s = weld_mesh(_dev(soup.reshape(-1, 3)), _faces(np.arange(120).reshape(-1, 3)), None, eps=0.0)
    out = decimate_fused(s, target_faces=10)
    assert not out.stats["decimate"]["reached"] and out.stats["decimate"]["rounds"] == 0 and out.faces.shape[0] == 40


def test_example_reports_the_decimated_mesh():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    plain = train_synthetic.mesh_scores(m, "2D", weld=0.02, split_edges=20.0, **cfg)["welded"]  # the split gives the welded soup interior vertices
    goal = plain["split"]["faces"] - 60
    res = train_synthetic.mesh_scores(m, "2D", weld=0.02, split_edges=20.0, decimate_faces=goal, **cfg)["welded"]
    t = res["decimated"]
    lines = train_synthetic.decimate_faces_report(t)
    print("\n".join(lines))
    assert "decimated" not in plain and {k: v for k, v in res.items() if k != "decimated"} == plain  # no other entry changes
    assert len(lines) == 3 and lines[0].startswith(f"decimated welded mesh: {t['collapses']} quadric-error collapses in {t['rounds']} rounds")
    assert f"{t['before']['vertices']} -> {t['vertices']} vertices, {t['before']['faces']} -> {t['faces']} faces" in lines[0]
    assert f"mean PSNR {t['before']['mean_psnr']:.2f} -> {t['mean_psnr']:.2f} dB" in lines[2]
    assert t["before"]["faces"] == plain["split"]["faces"] and t["target_faces"] == goal  # behind the other steps
    assert t["faces"] == t["before"]["faces"] - 2 * t["collapses"] and t["vertices"] == t["before"]["vertices"] - t["collapses"]
    assert t["reached"] == (t["faces"] <= goal) and t["faces"] >= goal - 1 and t["collapses"] > 0
    assert ("did NOT reach" in lines[0]) == (not t["reached"]) and (f"reached {goal} faces" in lines[0]) == t["reached"]
    soup = train_synthetic.mesh_scores(m, "2D", weld=0.0, decimate_faces=100, **cfg)["welded"]["decimated"]  # a soup: only boundary edges
    line = train_synthetic.decimate_faces_report(soup)[0]
    assert soup["collapses"] == 0 and not soup["reached"] and soup["faces"] == soup["before"]["faces"] and "nothing collapses" in line
    fused = train_synthetic.mesh_scores(m, "2D", extract=24, decimate_faces=200, **cfg)["fused"]
    d = fused["decimated"]
    lines = train_synthetic.decimate_faces_report(d)
    print("\n".join(lines))
    assert d["of"] == "fused" and d["before"]["faces"] == fused["topology"]["faces"] > 400
    assert d["collapses"] > 50 and d["faces"] == d["before"]["faces"] - 2 * d["collapses"] and d["faces"] >= 199
    assert len(lines) == 3 and "against the mesh it came from" in lines[2] and d["to_source"]["hausdorff"] < 0.5 * float(np.linalg.norm(np.ptp(m._vertex.detach().reshape(-1, 3).cpu().numpy(), axis=0)))


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
            out[f"{tag}.quadrics"] = q
            got = _gpu_round(v, f, q, 25, keep=k, seed=5, classify_only=classify_only, **rule)
            out.update({f"{tag}.{n}": t for n, t in zip(NAMES + ("totals",), got) if t is not None})
        small = _gpu_round(quad, [[0, 1, 2]], _gpu_quadrics(quad, [[0, 1, 2]]), 5)  # the one-face table
        out.update({f"one.{n}": t for n, t in zip(NAMES + ("totals",), small)})
        return out

    base = poison.assert_pure(call)  # twice on zeros first: the same call repeated gives identical bytes
    q = ref.vertex_quadrics(v, f, keep)
    want = ref.decimate_round(v, f, q, 25, keep=keep, seed=5, **rule)
    assert base["kept.quadrics"].numpy().tobytes() == q.tobytes()
    for name in NAMES:
        assert base[f"kept.{name}"].numpy().tobytes() == want[name].tobytes(), name
    assert base["classified.edge_state"].numpy().tobytes() == want["edge_state"].tobytes() and "classified.out_faces" not in base
    assert want["totals"][1] > 25 == want["totals"][2] > want["totals"][3] > 0 and want["totals"][4] > 0


# ---- graph replay -----------------------------------------------------------------------------------------------------------------------------
def decimate_call(inputs):
    """The quadrics and two rounds in one graph, the second reading the first's out_faces / out_keep / out_quadrics at capacity with no
    host step between; and the classification alone."""
    from diff_recon_hip import mesh_decimate as md
    v, f, keep = inputs["v"], inputs["f"], inputs["keep"]
    rule = (400.0, 20.0, md._min_cos_of(30.0), None)
    names = NAMES + ("totals",)
    q = md._quadrics_of(v, f, keep, DEV)
    first = md._decimate_arrays(v, f, keep, q, rule, 40, 7, False, DEV)
    out = dict(zip(names, first), quadrics=q)
    again = md._decimate_arrays(v, first[0], first[1], first[3], rule, 40, 8, False, DEV)
    out.update({f"{n}_2": t for n, t in zip(names, again)})
    only = md._decimate_arrays(v, f, keep, q, rule, 40, 7, True, DEV)
    out.update({f"{n}_classified": t for n, t in zip(names[4:], only[4:])})
    return out


def test_ts_decimate_h_replays_from_a_graph():
    from test_graph_replay_gpu import REPLAYS, grid_pair, one_face_pair
    a, b = grid_pair()  # 20 x 20 sheared and jittered, B with every 7th face dropped
    base_a, base_b, n = replay.assert_replays(decimate_call, a, b, differ=("totals", "totals_2", "totals_classified", "edge_state", "quadrics", "edge_cost"))
    assert n == REPLAYS
    ta, tb = base_a["totals"].view(torch.int64).tolist(), base_b["totals"].view(torch.int64).tolist()
    assert ta[3] > 0 and tb[3] > 0 and ta != tb and base_a["totals_2"].view(torch.int64).tolist()[3] > 0
    a, b = one_face_pair()
    base_a, base_b, n = replay.assert_replays(decimate_call, a, b, differ=("totals", "edge_state"))
    assert n == REPLAYS and base_a["totals"].view(torch.int64).tolist() == [3, 0, 0, 0, 0] and base_b["totals"].view(torch.int64).tolist() == [0, 0, 0, 0, 0]
