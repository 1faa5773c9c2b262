"""GPU tests of the edge collapse against tests/ref_mesh_collapse.py, everything bit for bit and to its capacity: out_faces, out_keep,
vertex_target, edge_vertices, edge_state, edge_removed, edge_guard with their fill values, and totals, with and without the face outputs;
the hand constructions, jittered grids and the lat-long sphere round by round to convergence, more scan tiles than a workgroup has lanes,
keep masks and broken faces, both modes, seeds, the empty calls, collapse_fused, isotropic_remesh, purity and graph replay."""
import numpy as np
import pytest
import torch

import poison
import ref_mesh_collapse as ref
import replay
from test_mesh_smooth_gpu import _latlong_sphere

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ref.NAMES
COS_30 = ref.min_cos_of(30.0)
GRID_RULE = dict(min_edge=0.8, max_edge=2.2, min_cos=COS_30)  # the jittered grids: unit spacing, edges from 0.4 to 2; all four guards act


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _faces(f):
    return _dev(np.asarray(f, np.int32).reshape(-1, 3))


def _same(got, want, what):
    """Equal shapes, dtypes and BYTES."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = np.nonzero(np.ascontiguousarray(got).reshape(-1) != np.ascontiguousarray(want).reshape(-1))[0]
    assert len(diff) == 0, (what, len(diff), diff[:5], got.reshape(-1)[diff[:5]], want.reshape(-1)[diff[:5]])


def _gpu_round(v, f, keep=None, pinned=None, min_edge=None, vertex_limit=None, max_edge=np.inf, min_cos=1.0, seed=0, classify_only=False):
    from diff_recon_hip import mesh_collapse as mc
    fd = _faces(f)
    k = None if keep is None else _dev(np.asarray(keep, np.uint8))
    p = None if pinned is None else _dev(np.asarray(pinned, np.uint8))
    limit = None if vertex_limit is None else _dev(np.asarray(vertex_limit, np.float32))
    mode = mc.MARK_SHORTER if vertex_limit is None else mc.MARK_VERTEX_LIMIT
    return mc._collapse_arrays(_dev(np.asarray(v, np.float32).reshape(-1, 3)), fd, k, p, mode, float(min_edge or 0.0), limit, float(max_edge),
                               float(min_cos), seed, classify_only, fd.device)


def _assert_round(v, f, what="", **rule):
    """tsp_collapse against the reference, every output to its capacity, with and without the face outputs."""
    want = ref.collapse_round(v, f, **rule)
    for classify_only in (False, True):
        got = _gpu_round(v, f, classify_only=classify_only, **rule)
        assert got[7].tolist() == want["totals"] and got[7].dtype == torch.int64, (what, got[7].tolist(), want["totals"])
        for name, t in zip(NAMES, got[:7]):
            if classify_only and name in NAMES[:3]:
                assert t is None
            else:
                _same(t, want[name], (what, name, classify_only))
    return want


def _assert_all_rounds(v, f, keep=None, max_rounds=64, what="", **rule):
    """Round by round with seed = round index until one collapses nothing; then collapse_short_edges as a whole against the same, as it
    stands and compacted."""
    from diff_recon_hip import collapse_short_edges
    v = np.asarray(v, np.float32)
    g, k, per_round, converged = np.asarray(f, np.int32).reshape(-1, 3), keep, [], False
    target = np.arange(len(v), dtype=np.int32)
    for r in range(max_rounds):
        want = _assert_round(v, g, (what, "round", r), keep=k, seed=r, **rule)
        if want["totals"][3] == 0:
            converged = True
            break
        per_round.append(want["totals"])
        g, k = want["out_faces"], want["out_keep"]
        target = want["vertex_target"][target]
    kw = dict(min_edge=rule.get("min_edge"), max_edge=rule.get("max_edge", np.inf), max_rounds=max_rounds,
              vertex_limit=None if rule.get("vertex_limit") is None else _dev(np.asarray(rule["vertex_limit"], np.float32)),
              pinned=None if rule.get("pinned") is None else _dev(np.asarray(rule["pinned"], np.uint8)),
              keep=None if keep is None else _dev(np.asarray(keep, np.uint8)))
    deg = 30.0 if rule.get("min_cos", COS_30) == COS_30 else 90.0
    assert float(ref.min_cos_of(deg)) == float(rule.get("min_cos", COS_30))
    out = collapse_short_edges(_dev(v), _faces(f), max_normal_deg=deg, compact=False, **kw)
    final_keep = np.ones(len(g), bool) if k is None else np.asarray(k) != 0
    _same(out.faces, g, (what, "faces"))
    assert np.array_equal(out.face_keep.cpu().numpy(), final_keep) and out.face_keep.dtype == torch.bool
    _same(out.vertex_map, target, (what, "vertex_map"))
    assert out.converged == converged == out.stats["converged"] and out.stats["rounds"] == len(per_round)
    assert [[t[n] for n in ("edges", "short", "candidates", "collapsed")] for t in out.stats["per_round"]] == per_round
    assert out.stats["collapsed"] == sum(t[3] for t in per_round)
    packed = collapse_short_edges(_dev(v), _faces(f), max_normal_deg=deg, compact=True, attributes=_dev(v), **kw)
    survives = target == np.arange(len(v))
    new_index = np.cumsum(survives) - 1
    _same(packed.vertices, v[survives], (what, "compact vertices"))
    _same(packed.attributes, v[survives], (what, "compact attributes"))
    _same(packed.vertex_map, new_index[target].astype(np.int32), (what, "compact vertex_map"))
    _same(packed.face_map, np.nonzero(final_keep)[0].astype(np.int32), (what, "face_map"))
    part = ref.takes_part(len(v), g) & final_keep
    assert np.array_equal(packed.faces.cpu().numpy()[part[final_keep]], new_index[g[part]].astype(np.int32)) and packed.face_keep is None
    assert packed.stats["num_vertices"] == int(survives.sum()) and packed.stats["num_faces"] == int(final_keep.sum())
    return g, k, per_round, converged


# ---- the hand constructions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.hand_constructions()))
def test_hand_constructions_match_the_reference_bit_for_bit(name):
    v, f, rule = ref.hand_constructions()[name]
    for seed in (0, 7):
        want = _assert_round(v, f, name, seed=seed, **rule)
    if name == "hexagon fan":
        assert want["totals"] == [12, 1, 1, 1] and want["out_keep"].sum() == 4
    if name == "octahedron":
        assert want["totals"] == [12, 12, 12, 1]
    if name == "fan of 65":
        assert want["totals"] == [130, 0, 0, 0]
    if name == "fan of 64":
        assert want["totals"] == [128, 1, 1, 1]


# ---- grids and the sphere, all rounds to convergence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [(1, 1), (2, 2), (3, 3), (7, 7), (17, 17)])
def test_jittered_grids_match_round_by_round_until_they_converge(cells):
    """F = 2, 8, 18, 98, 578.  One cell has no interior vertex, so nothing is eligible; the one interior vertex of 2 x 2 cells has a short
    edge that the length guard holds; from 3 x 3 cells on edges collapse."""
    v, f = ref.jittered_grid(*cells, 0.3, seed={1: 1, 2: 1, 3: 1, 7: 7, 17: 17}[cells[0]], z=0.1)
    assert len(f) == 2 * cells[0] * cells[1]
    g, k, per_round, converged = _assert_all_rounds(v, f, what=cells, **GRID_RULE)
    assert converged and len(per_round) >= {1: 0, 2: 0, 3: 1, 7: 2, 17: 3}[cells[0]]
    if cells[0] == 2:
        assert ref.collapse_round(v, f, **GRID_RULE)["totals"][1:] == [1, 0, 0]
    print(f"F = {len(f)}: {len(per_round)} rounds, collapses {[t[3] for t in per_round]}")


def test_latlong_sphere_matches_round_by_round_until_it_converges():
    v, f = _latlong_sphere()  # radius 0.6, 14 rings of 20: edges of 0.03 at the poles, 0.19 at the equator
    g, k, per_round, converged = _assert_all_rounds(v, f, what="sphere", min_edge=0.1, max_edge=0.3, min_cos=COS_30)
    assert converged and sum(t[3] for t in per_round) > 20
    print(f"lat-long sphere, {len(f)} faces: {len(per_round)} rounds, collapses {[t[3] for t in per_round]}")


def test_more_scan_blocks_than_one_workgroup_has_lanes():
    """180000 faces: 264 scan tiles of half-edges, so a lane of the offsets kernel owns two.  About 2700 pinched vertices: short edges
    sparse enough for the reference's ring walks."""
    v, f = ref.pinched_grid(300, 300)
    assert len(f) == 180000 and -(-3 * len(f) // 2048) > 256
    want = _assert_round(v, f, "large", min_edge=0.5, max_edge=1.8, min_cos=COS_30)
    assert 2000 < want["totals"][3] < 10000
    again = _assert_round(v, want["out_faces"], "large, second round", keep=want["out_keep"], min_edge=0.5, max_edge=1.8, min_cos=COS_30, seed=1)
    assert again["totals"][3] < want["totals"][3]


# ---- keep masks, broken faces, both modes, seeds ----------------------------------------------------------------------------------------------
def test_keep_masks_and_broken_faces_match_the_reference():
    v, f = ref.jittered_grid(17, 17, 0.3, seed=4, z=0.1)
    rng = np.random.default_rng(3)
    keep = (rng.integers(0, 5, len(f)) != 0).astype(np.uint8)
    f = f.copy()
    f[rng.integers(0, len(f), 6)] = [[0, 0, 1], [-1, 2, 3], [1, 2, len(v)], [5, 6, 5], [2 ** 31 - 1, 0, 1], [7, 7, 7]]
    v = v.copy()
    v[rng.integers(0, len(v), 4)] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]]
    pinned = (rng.integers(0, 8, len(v)) == 0).astype(np.uint8)
    for k in (None, keep, np.zeros(len(f), np.uint8)):
        for seed in (0, 1, 0xFFFFFFFF):
            want = _assert_round(v, f, "keep", keep=k, seed=seed, pinned=pinned if seed else None, **GRID_RULE)
        if k is keep:
            assert want["totals"][3] > 0 and np.array_equal(want["out_faces"][keep == 0], f[keep == 0]) and not want["out_keep"][keep == 0].any()


def test_vertex_limit_mode_matches_the_reference():
    v, f = ref.jittered_grid(17, 17, 0.3, seed=6, z=0.1)
    limit = np.random.default_rng(5).uniform(0.5, 1.1, len(v)).astype(np.float32)
    limit[::37] = np.nan
    g, k, per_round, converged = _assert_all_rounds(v, f, what="limit", vertex_limit=limit, max_edge=2.2, min_cos=COS_30)
    assert converged and sum(t[3] for t in per_round) > 10


def test_seed_changes_the_winners_but_not_the_candidates():
    from diff_recon_hip import collapse_edges, short_edges
    v, f = ref.jittered_grid(12, 12, 0.0)  # regular: every edge along a row or a column has length 1, so the priorities decide
    rule = dict(min_edge=1.2, max_edge=2.5, min_cos=COS_30)
    vd, fd = _dev(v), _faces(f)
    first, states = collapse_edges(vd, fd, min_edge=1.2, max_edge=2.5), set()
    for seed in range(4):
        r, c = collapse_edges(vd, fd, min_edge=1.2, max_edge=2.5, seed=seed), short_edges(vd, fd, min_edge=1.2, max_edge=2.5, seed=seed)
        want = ref.collapse_round(v, f, seed=seed, **rule)
        E = want["E"]
        assert {n: r.stats[n] for n in ("edges", "short", "candidates", "collapsed")} == dict(zip(("edges", "short", "candidates", "collapsed"), want["totals"]))
        guarded = want["edge_state"][:E] == ref.GUARDED
        assert r.stats["guarded"] == want["totals"][1] - want["totals"][2] == int(guarded.sum())
        for name, bit in (("link", 1), ("long", 2), ("normal", 4), ("held", 8)):
            assert r.stats[f"guarded_{name}"] == int((guarded & ((want["edge_guard"][:E] & bit) != 0)).sum())
        for got, name in ((r.edge_state, "edge_state"), (r.edge_vertices, "edge_vertices"), (r.edge_removed, "edge_removed"), (r.edge_guard, "edge_guard"),
                          (r.faces, "out_faces"), (r.vertex_target, "vertex_target")):
            _same(got, want[name][:E] if name.startswith("edge") else want[name], name)
        assert np.array_equal(r.face_keep.cpu().numpy(), want["out_keep"] != 0)
        assert c.faces is None and c.face_keep is None and c.vertex_target is None and torch.equal(c.edge_state, r.edge_state) and c.stats == r.stats
        assert torch.equal(r.edge_state >= ref.LOST, first.edge_state >= ref.LOST)  # the same candidates
        assert int((~r.face_keep).sum()) == 2 * r.stats["collapsed"]
        states.add(r.edge_state.cpu().numpy().tobytes())
    assert len(states) > 1 and first.stats["candidates"] > first.stats["collapsed"] > 0


# ---- the empty calls --------------------------------------------------------------------------------------------------------------------------
def test_no_faces_and_no_vertices_write_the_empty_result():
    from diff_recon_hip import collapse_edges, collapse_short_edges, short_edges
    f0 = torch.zeros((0, 3), device=DEV, dtype=torch.int32)
    for V in (0, 5):
        vd = torch.ones((V, 3), device=DEV)
        for call in (collapse_edges, short_edges):
            r = call(vd, f0, min_edge=1.0)
            assert r.edge_vertices.shape == (0, 2) and r.edge_state.shape == (0,) and r.edge_removed.shape == (0,) and r.edge_guard.shape == (0,)
            assert {n: r.stats[n] for n in ("edges", "short", "candidates", "collapsed", "guarded")} == dict(edges=0, short=0, candidates=0, collapsed=0, guarded=0)
        r = collapse_edges(vd, f0, min_edge=1.0)
        assert r.faces.shape == (0, 3) and r.face_keep.shape == (0,) and r.vertex_target.tolist() == list(range(V))
        d = collapse_short_edges(vd, f0, min_edge=1.0)
        assert d.converged and d.faces.shape == (0, 3) and d.stats["rounds"] == 0 and d.vertices.shape == (V, 3)
    f = np.array([[0, 1, 2], [3, 4, 5], [-1, 7, 2 ** 31 - 1], [0, 0, 0]])  # faces without vertices: nothing takes part, everything is still written
    for keep in (None, [1, 0, 1, 0]):
        want = _assert_round(np.zeros((0, 3), np.float32), f, "V = 0", keep=keep, min_edge=1.0)
        assert want["totals"] == [0, 0, 0, 0] and np.array_equal(want["out_faces"], f.astype(np.int32))
        assert want["out_keep"].tolist() == ([1, 1, 1, 1] if keep is None else keep)


# ---- collapse_fused ---------------------------------------------------------------------------------------------------------------------------
def test_collapse_fused_returns_the_kind_of_mesh_it_was_given():
    from diff_recon_hip import collapse_fused, weld_mesh
    from diff_recon_hip.color_volume import ColoredMesh
    v, f = ref.jittered_grid(7, 7, 0.3, seed=7, z=0.1)
    g, k, target, per_round, converged = ref.collapse_short_edges(v, f, **GRID_RULE)
    assert converged and len(per_round) >= 1
    survives, kept = target == np.arange(len(v)), k != 0
    new_index = np.cumsum(survives) - 1
    colour = np.random.default_rng(3).uniform(0, 1, (len(f), 3)).astype(np.float32)
    w = weld_mesh(_dev(v), _faces(f), _dev(colour), eps=0.0)
    assert torch.equal(w.faces.cpu(), torch.from_numpy(f))  # nothing to weld: the indexed mesh is the input
    out = collapse_fused(w, 0.8, max_edge=2.2)
    assert type(out) is type(w) and "collapse" not in w.stats and out.stats["collapse"]["converged"] and out.stats["collapse"]["rounds"] == len(per_round)
    _same(out.vertices, v[survives], "vertices")
    _same(out.faces, new_index[g[kept]].astype(np.int32), "faces")
    _same(out.faces_color, colour[kept], "faces_color")
    _same(out.vertex_map, new_index[target][w.vertex_map.cpu().numpy()].astype(np.int32), "vertex_map")
    assert out.stats["num_vertices"] == int(survives.sum()) and out.stats["num_faces"] == int(kept.sum())
    vc = np.random.default_rng(4).uniform(0, 1, (len(v), 3)).astype(np.float32)
    valid = np.random.default_rng(5).integers(0, 2, len(v)).astype(bool)
    c = ColoredMesh(_dev(v), _faces(f), _dev(vc), _dev(valid), {"num_vertices": len(v), "num_faces": len(f)})
    out = collapse_fused(c, 0.8, max_edge=2.2, max_rounds=1)
    one = ref.collapse_round(v, f, seed=0, **GRID_RULE)
    lives = one["vertex_target"] == np.arange(len(v))
    assert type(out) is ColoredMesh and not out.stats["collapse"]["converged"]
    _same(out.vertex_color, vc[lives], "vertex_color")
    assert np.array_equal(out.color_valid.cpu().numpy(), valid[lives]) and out.color_valid.dtype == torch.bool
    _same(out.faces, (np.cumsum(lives) - 1)[one["out_faces"][one["out_keep"] != 0]].astype(np.int32), "one round")


# ---- isotropic_remesh -------------------------------------------------------------------------------------------------------------------------
def _edge_lengths(v, f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    e = np.unique(e, axis=0)
    return e, np.sqrt(((v[e[:, 0]].astype(np.float64) - v[e[:, 1]]) ** 2).sum(1))


def test_isotropic_remesh_keeps_the_topology_and_removes_the_needles():
    from diff_recon_hip import isotropic_remesh, mesh_topology, remesh, short_edges, triangle_quality
    v, f = _latlong_sphere()
    m = remesh((_dev(v), _faces(f)), 12)  # marching tetrahedra: needles wherever the sphere passes close to a grid vertex
    target = 1.5 * float(m.stats["voxel_size"])
    low, high = 0.8 * target, 4.0 / 3.0 * target
    before = mesh_topology(m.vertices.shape[0], m.faces)
    assert before["boundary"] == 0 and before["nonmanifold"] == 0 and before["pieces"] == 1 and before["euler"] == 2
    q0 = triangle_quality(m.vertices, m.faces)
    out = isotropic_remesh(m.vertices, m.faces, target, iterations=3)
    V, F = out.vertices.shape[0], out.faces.shape[0]
    after = mesh_topology(V, out.faces)
    assert {k: after[k] for k in ("boundary", "nonmanifold", "pieces", "euler")} == {k: before[k] for k in ("boundary", "nonmanifold", "pieces", "euler")}
    assert after["vertices_referenced"] == V and after["faces"] == F  # compacted: no vertex and no face is left over
    assert all(step["split"]["converged"] and step["collapse"]["converged"] and step["flip"]["converged"] for step in out.stats["iterations"])
    assert out.stats["closing"]["split"]["converged"] and out.stats["closing"]["collapse"]["converged"]
    e, length = _edge_lengths(out.vertices.cpu().numpy(), out.faces.cpu().numpy())
    s = short_edges(out.vertices, out.faces, min_edge=low, max_edge=high)
    q1 = triangle_quality(out.vertices, out.faces)
    print(f"remeshed sphere: V {m.vertices.shape[0]} -> {V}, F {m.faces.shape[0]} -> {F}, quality min {float(q0.min()):.4f} -> {float(q1.min()):.4f}, "
          f"median {float(q0.median()):.3f} -> {float(q1.median()):.3f}, edges {out.stats['before']['edge_length']} -> {out.stats['after']['edge_length']}, "
          f"target {target:.4f}, still short {s.stats['short']} (guarded {s.stats['guarded']}), above 4/3 target {int((length > high).sum())}, "
          f"last flips {out.stats['iterations'][-1]['flip']['flipped']}, closing {out.stats['closing']}")
    # the shortest edge is >= 4/5 target unless guarded: nothing that is still short could collapse
    assert s.stats["candidates"] == 0 and s.stats["short"] == s.stats["guarded"]
    assert length[length < np.float32(low)].shape[0] == s.stats["short"]  # a closed manifold: every edge is eligible, so every short edge is counted
    # the longest is <= 4/3 target: the splits converged, and the collapses are bound by max_edge
    assert length.max() <= high * (1 + 1e-6)
    assert float(q1.min()) >= float(q0.min())
    assert out.stats["before"]["quality"][0] == pytest.approx(float(q0.min())) and out.stats["after"]["num_faces"] == F


def test_example_reports_the_collapsed_mesh():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    plain = train_synthetic.mesh_scores(m, "2D", weld=0.02, split_edges=20.0, flip_edges=True, **cfg)["welded"]
    res = train_synthetic.mesh_scores(m, "2D", weld=0.02, split_edges=20.0, flip_edges=True, collapse_edges=12.0, **cfg)["welded"]
    t = res["collapsed"]
    lines = train_synthetic.collapse_edges_report(t)
    print("\n".join(lines))
    assert "collapsed" not in plain and {k: v for k, v in res.items() if k != "collapsed"} == plain  # no other entry changes
    assert len(lines) == 3 and lines[0].startswith(f"collapsed mesh: {t['collapses']} collapses of edges below 12 in {t['rounds']} rounds")
    assert f"{t['before']['vertices']} -> {t['vertices']} vertices, {t['before']['faces']} -> {t['faces']} faces" in lines[0]
    assert f"mean PSNR {t['before']['mean_psnr']:.2f} -> {t['mean_psnr']:.2f} dB" in lines[2]
    assert t["before"]["faces"] == res["split"]["faces"] and t["before"]["mean_psnr"] == res["split"]["flipped"]["mean_psnr"]  # behind the other steps
    assert t["converged"] and t["faces"] == t["before"]["faces"] - 2 * t["collapses"] and t["vertices"] == t["before"]["vertices"] - t["collapses"]
    assert t["collapses"] > 0 and 0.0 <= t["quality"][0] <= t["quality"][1] <= 1.0
    only = train_synthetic.mesh_scores(m, "2D", weld=0.02, collapse_edges=12.0, **cfg)["welded"]  # without the other steps: the welded mesh itself
    assert only["collapsed"]["before"]["faces"] == int(only["stats"]["num_faces"]) and "split" not in only


# ---- determinism and purity -------------------------------------------------------------------------------------------------------------------
def test_the_round_is_pure_and_deterministic():
    v, f = ref.jittered_grid(17, 17, 0.3, seed=11, z=0.1)
    keep = (np.random.default_rng(8).integers(0, 6, len(f)) != 0).astype(np.uint8)
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]], np.float32)

    def call(pattern):  # the workspace and every output come from torch.empty and are poisoned, with guard bytes either side
        out = {}
        for tag, k, classify_only in (("all", None, False), ("kept", keep, False), ("classified", keep, True)):
            got = _gpu_round(v, f, keep=k, seed=5, classify_only=classify_only, **GRID_RULE)
            out.update({f"{tag}.{n}": t for n, t in zip(NAMES + ("totals",), got) if t is not None})
        small = _gpu_round(quad, [[0, 1, 2]], min_edge=5.0)  # the one-face table
        out.update({f"one.{n}": t for n, t in zip(NAMES + ("totals",), small)})
        return out

    base = poison.assert_pure(call)  # twice on zeros first: the same call repeated gives identical bytes
    want = ref.collapse_round(v, f, keep=keep, seed=5, **GRID_RULE)
    for name in NAMES:
        assert base[f"kept.{name}"].numpy().tobytes() == want[name].tobytes(), name
    assert base["classified.edge_state"].numpy().tobytes() == want["edge_state"].tobytes() and "classified.out_faces" not in base
    assert want["totals"][2] > want["totals"][3] > 0


# ---- graph replay -----------------------------------------------------------------------------------------------------------------------------
def collapse_call(inputs):
    """Two rounds in one graph, the second reading the first's out_faces / out_keep at capacity with no host step between; and the
    classification alone."""
    from diff_recon_hip import mesh_collapse as mc
    v, f, keep = inputs["v"], inputs["f"], inputs["keep"]
    rule = (mc.MARK_SHORTER, 7.0, None, 20.0, mc.min_cos_of(30.0))
    names = NAMES + ("totals",)
    first = mc._collapse_arrays(v, f, keep, None, *rule, 7, False, DEV)
    out = dict(zip(names, first))
    again = mc._collapse_arrays(v, first[0], first[1], None, *rule, 8, False, DEV)
    out.update({f"{n}_2": t for n, t in zip(names, again)})
    only = mc._collapse_arrays(v, f, keep, None, *rule, 7, True, DEV)
    out.update({f"{n}_classified": t for n, t in zip(names[3:], only[3:])})
    return out


def test_ts_collapse_h_replays_from_a_graph():
    from test_graph_replay_gpu import REPLAYS, grid_pair, one_face_pair
    a, b = grid_pair()  # 20 x 20, spacing 6 x 8 jittered by 1: the edges along the rows fall either side of 7
    base_a, base_b, n = replay.assert_replays(collapse_call, a, b, differ=("totals", "totals_2", "totals_classified", "edge_state"))
    assert n == REPLAYS
    ta, tb = base_a["totals"].view(torch.int64).tolist(), base_b["totals"].view(torch.int64).tolist()
    assert ta[3] > 10 and tb[3] > 0 and ta != tb and base_a["totals_2"].view(torch.int64).tolist()[3] > 0
    a, b = one_face_pair()
    base_a, base_b, n = replay.assert_replays(collapse_call, a, b, differ=("totals", "edge_state"))
    assert n == REPLAYS and base_a["totals"].view(torch.int64).tolist() == [3, 0, 0, 0] and base_b["totals"].view(torch.int64).tolist() == [0, 0, 0, 0]
