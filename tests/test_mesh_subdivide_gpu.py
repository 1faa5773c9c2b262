"""GPU tests of the edge table and the edge split against tests/ref_mesh_subdivide.py, everything bit for bit and to its capacity: edge_vertices,
edge_use, edge_length2, half_edge_edge and counts; new_vertices, new_attributes, new_attr_valid, new_vertex_edge, out_faces, out_face_parent
with their fill values, and totals; the three mark modes, keep masks, NaN / Inf vertices, out-of-range and repeated indices, attributes of
mixed validity; the empty calls; the counts beside vertex_adjacency's and mesh_topology's; the rounds; two levels of a closed solid; purity."""
import functools

import numpy as np
import pytest
import torch

import poison
import ref_mesh_simplify as fixtures
import ref_mesh_subdivide as ref
from test_mesh_smooth_gpu import _latlong_sphere, _soup

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 2, 8, 9, 65, 521]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _faces(f):
    return _dev(np.asarray(f, np.int32).reshape(-1, 3))


def _opt(a, dtype):
    return None if a is None else _dev(np.asarray(a, dtype))


def _same(got, want, what):
    """Equal shapes, dtypes and BYTES: NaN payloads and the sign of zero count."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    word = {4: np.uint32, 8: np.uint64, 1: np.uint8}[g.dtype.itemsize]
    g, w = g.view(word), w.view(word)
    diff = np.nonzero(g != w)[0]
    assert len(diff) == 0, (what, len(diff), diff[:5], g[diff[:5]], w[diff[:5]])


def _gpu_edges(V, f, keep=None, v=None):
    from diff_recon_hip import mesh_subdivide
    fd = _faces(f)
    return mesh_subdivide._edges_arrays(V, fd, _opt(keep, np.uint8), _opt(v, np.float32), fd.device)


def _gpu_split(v, f, keep=None, mode=ref.MARK_ALL, max_edge=0.0, limit=None, attrs=None, valid=None):
    from diff_recon_hip import mesh_subdivide
    fd = _faces(f)
    return mesh_subdivide._split_arrays(_dev(np.asarray(v, np.float32).reshape(-1, 3)), fd, _opt(keep, np.uint8), mode, float(max_edge),
                                        _opt(limit, np.float32), _opt(attrs, np.float32), _opt(valid, np.uint8), fd.device)


def _assert_edges(v, f, keep=None):
    """tsd_edges with and without lengths against the reference, every output to its capacity."""
    V = len(v)
    want = ref.edges(V, f, keep, v)
    for vertices in (v, None):
        ev, use, length2, hee, counts = _gpu_edges(V, f, keep, vertices)
        _same(ev, want["edge_vertices"], "edge_vertices")
        _same(use, want["edge_use"], "edge_use")
        _same(hee, want["half_edge_edge"], "half_edge_edge")
        assert counts.tolist() == want["counts"] and counts.dtype == torch.int64
        if vertices is None:
            assert length2 is None
        else:
            _same(length2, want["edge_length2"], "edge_length2")
    return want


def _assert_split(v, f, keep=None, mode=ref.MARK_ALL, max_edge=0.0, limit=None, attrs=None, valid=None):
    """tsd_split against the reference, every output to its capacity."""
    want = ref.split(v, f, keep, mode, max_edge, limit, attrs, valid)
    nv, na, nvalid, nedge, out_faces, parent, totals = _gpu_split(v, f, keep, mode, max_edge, limit, attrs, valid)
    what = (mode, len(f))
    _same(nv, want["new_vertices"], ("new_vertices", what))
    _same(nedge, want["new_vertex_edge"], ("new_vertex_edge", what))
    _same(out_faces, want["out_faces"], ("out_faces", what))
    _same(parent, want["out_face_parent"], ("out_face_parent", what))
    assert totals.tolist() == want["totals"] and totals.dtype == torch.int64, (totals.tolist(), want["totals"], what)
    if want["new_attributes"] is None:
        assert na is None and nvalid is None
    else:
        _same(na, want["new_attributes"], ("new_attributes", what))
        _same(nvalid, want["new_attr_valid"], ("new_attr_valid", what))
    return want


def _median_edge(v, f, keep=None):
    t = ref.edges(len(v), f, keep, v)
    l2 = t["edge_length2"][:t["E"]][t["finite"]]
    return float(np.sqrt(np.median(l2))) if len(l2) else 1.0


def _all_modes(v, f, keep=None, attrs=None, valid=None, seed=0):
    """The three mark modes on one mesh: all edges; the edges above the median length (about half of them, so every face case occurs); a
    per-vertex limit with NaN, zero and huge entries."""
    v = np.asarray(v, np.float32)
    med = _median_edge(v, f, keep)
    rng = np.random.default_rng(seed)
    limit = (med * rng.uniform(0.5, 1.5, len(v))).astype(np.float32)
    if len(v) > 4:
        limit[rng.integers(0, len(v), 3)] = (np.nan, 0.0, 1e30)
    out = [_assert_split(v, f, keep, ref.MARK_ALL, 0.0, None, attrs, valid),
           _assert_split(v, f, keep, ref.MARK_LONGER, med, None, attrs, valid),
           _assert_split(v, f, keep, ref.MARK_VERTEX_LIMIT, 0.0, limit, attrs, valid)]
    return out


@functools.lru_cache(maxsize=None)
def _solid():
    v, f = fixtures.sphere_mesh()  # closed: 4834 vertices, 9664 faces
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def _attributes(V, channels, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, (V, channels)).astype(np.float32), (rng.integers(0, 3, V) != 0).astype(np.uint8)


# ---- the first F faces of a closed solid, and a random soup of F faces --------------------------------------------------------------------------
@pytest.mark.parametrize("F", SIZES)
def test_faces_of_a_closed_solid_match_the_reference_bit_for_bit(F):
    v, f = _solid()
    f = f[:F]
    _assert_edges(v, f)
    cases = {n: [] for n in range(5)}
    for want in _all_modes(v, f, seed=F):
        pieces = np.bincount(want["out_face_parent"][:want["totals"][2]], minlength=F)
        for n in range(1, 5):
            cases[n].append(int((pieces == n).sum()))
    print(f"F = {F}: faces with 1 / 2 / 3 / 4 pieces per mode {[cases[n] for n in range(1, 5)]}")
    if F >= 65:
        assert all(sum(cases[n]) > 0 for n in range(1, 5))  # every face case occurred


@pytest.mark.parametrize("F", SIZES)
def test_random_soups_match_the_reference_bit_for_bit(F):
    """test_mesh_smooth_gpu's soup cut to F faces: from F = 521 on with indices -1 and V, repeated indices, duplicated, rotated and reversed
    triples, a hub, NaN / Inf vertices and coincident vertices (zero-length edges); every mode with and without its keep mask."""
    V = max((F + 1) // 2, 1)
    v, f, keep, _ = _soup(V)
    f, keep = f[:F], keep[:F]
    for k in (None, keep):
        want = _assert_edges(v, f, k)
        _all_modes(v, f, k, seed=F)
        part = ref.participation(V, f, k)
        if F >= 521:
            assert (~part).sum() > 0 and want["counts"][3] > 0 and not want["finite"].all()


def test_whole_solid_and_large_soup_span_several_blocks():
    """9664 faces of the closed solid (15 scan tiles of half-edges) and a soup of 2050 faces with everything the soup has."""
    v, f = _solid()
    want = _assert_edges(v, f)
    assert want["counts"] == [3 * len(f) // 2, 0, 3 * len(f) // 2, 0]
    a, valid = _attributes(len(v), 3, 1)
    for s in _all_modes(v, f, attrs=a, valid=valid, seed=3):
        n, nf = s["totals"][1], s["totals"][2]
        t = ref.edges(len(v) + n, s["out_faces"][:nf])
        assert t["counts"][1] == t["counts"][3] == 0  # conforming: the split solid is still closed
    v, f, keep, _ = _soup(1025)
    a, valid = _attributes(1025, 1, 2)
    _assert_edges(v, f, keep)
    _all_modes(v, f, keep, a, valid, seed=4)


def test_more_scan_blocks_than_one_workgroup_has_lanes():
    """180000 faces: 264 scan tiles of half-edges, so a lane of the offsets kernel owns two."""
    rng = np.random.default_rng(77)
    V = 60000
    v = rng.uniform(-1, 1, (V, 3)).astype(np.float32)
    f = rng.integers(0, V, (180000, 3)).astype(np.int32)
    want = _assert_split(v, f, None, ref.MARK_LONGER, 1.1)
    assert 0 < want["totals"][1] < want["totals"][0] and -(-3 * len(f) // 2048) > 256


# ---- keep masks, attributes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [0, 1, 3])
def test_attributes_of_mixed_validity_match_the_reference(channels):
    v, f = _solid()
    f = f[:521]
    keep = (np.random.default_rng(5).integers(0, 4, len(f)) != 0).astype(np.uint8)
    a, valid = _attributes(len(v), channels, 10 + channels)
    for k in (None, keep):
        for ok in (None, valid):
            out = _all_modes(v, f, k, a if channels else None, ok if channels else None, seed=channels)
            if channels and ok is not None:
                n = out[0]["totals"][1]
                flags = out[0]["new_attr_valid"][:n]
                ends = out[0]["new_vertex_edge"][:n]
                assert (flags == 0).sum() > 0 and ((valid[ends[:, 0]] != valid[ends[:, 1]]).sum()) > 0  # neither end, and exactly one
    if channels == 0:  # the wrapper with a (V, 0) attribute tensor: valid iff an end is
        from diff_recon_hip import split_edges
        r = split_edges(_dev(v), _faces(f), vertex_attributes=_dev(a), attribute_valid=_dev(valid))
        _, _, wa, wvalid, _, _, _ = ref.split_mesh(v, f, attributes=a, attr_valid=valid)
        assert r.vertex_attributes.shape == wa.shape and np.array_equal(r.attribute_valid.cpu().numpy(), wvalid)


def test_masked_neighbours_keep_their_long_edge():
    v, f = _solid()
    f = f[:65]
    keep = np.ones(65, np.uint8)
    keep[::3] = 0
    want = _assert_split(v, f, keep)
    rows = want["out_faces"][:want["totals"][2]]
    parent = want["out_face_parent"][:want["totals"][2]]
    assert np.array_equal(rows[np.isin(parent, np.nonzero(keep == 0)[0])], f[keep == 0])  # bit for bit, one piece each


# ---- the empty calls ------------------------------------------------------------------------------------------------------------------------------
def test_no_faces_and_no_vertices_write_the_empty_result():
    from diff_recon_hip import mesh_edges, split_edges, split_long_edges, subdivide_mesh
    f0 = torch.zeros((0, 3), device=DEV, dtype=torch.int32)
    for V in (0, 5):
        e = mesh_edges(V, f0, vertices=torch.zeros((V, 3), device=DEV))
        assert e.edge_vertices.shape == (0, 2) and e.edge_use.shape == (0,) and e.length.shape == (0,) and e.half_edge_edge.shape == (0,)
        assert e.stats == dict.fromkeys(ref.COUNT_NAMES, 0)
        for call in (split_edges, lambda *a, **k: split_long_edges(*a, max_edge=1.0, **k), subdivide_mesh):
            out = call(torch.ones((V, 3), device=DEV), f0, vertex_attributes=torch.ones((V, 2), device=DEV))
            assert out.vertices.shape == (V, 3) and out.faces.shape == (0, 3) and out.face_parent.shape == (0,) and not out.new_vertex.any()
            assert out.vertex_attributes.shape == (V, 2) and out.attribute_valid.all() and out.vertex_edge.shape == (V, 2)
    f = np.array([[0, 1, 2], [3, 4, 5], [-1, 7, 2 ** 31 - 1], [0, 0, 0]])  # faces without vertices: nothing takes part, everything is still written
    v0 = np.zeros((0, 3), np.float32)
    want = _assert_edges(v0, f)
    assert want["counts"] == [0] * 4 and (want["half_edge_edge"] == -1).all()
    for mode, kw in ((ref.MARK_ALL, {}), (ref.MARK_LONGER, {"max_edge": 0.5}), (ref.MARK_VERTEX_LIMIT, {"limit": np.zeros(0, np.float32)})):
        s = _assert_split(v0, f, mode=mode, attrs=np.zeros((0, 2), np.float32), **kw)
        assert s["totals"] == [0, 0, 4, 0] and np.array_equal(s["out_faces"][:4], f.astype(np.int32))


# ---- the counts beside the neighbours' ------------------------------------------------------------------------------------------------------------
def test_edge_counts_are_half_of_the_adjacency_s_and_equal_the_topology_s():
    from diff_recon_hip import mesh_edges, mesh_topology, vertex_adjacency
    v, f = _solid()
    cut = f[:3000]  # an open piece of the solid: boundary and manifold edges
    for V, faces, keep in ((len(v), f, None), (len(v), cut, None), (len(v), cut, (np.arange(3000) % 7 != 0))):
        fd, kd = _faces(faces), _opt(keep, np.bool_)
        e, adj, top = mesh_edges(V, fd, kd, _dev(v)), vertex_adjacency(V, fd, kd), mesh_topology(V, fd, kd)
        assert {k: 2 * e.stats[k] for k in ("boundary", "manifold", "nonmanifold")} == {k: adj.stats[k] for k in ("boundary", "manifold", "nonmanifold")}
        assert 2 * e.stats["edges"] == adj.stats["entries"]
        assert [e.stats[k] for k in ref.COUNT_NAMES] == [top[k] for k in ref.COUNT_NAMES]  # no repeated index here, so the weld's rule agrees
        assert e.edge_vertices.shape == (e.stats["edges"], 2) and e.length.dtype == torch.float64
        want = ref.edges(V, faces, keep, v)
        _same(e.length, np.sqrt(want["edge_length2"][:want["E"]]), "length")
        assert (e.edge_vertices[:, 0] < e.edge_vertices[:, 1]).all()
    sv, sf, skeep, _ = _soup(1025)  # repeated indices take no part here, as in vertex_adjacency
    e, adj = mesh_edges(1025, _faces(sf), _dev(skeep), _dev(sv)), vertex_adjacency(1025, _faces(sf), _dev(skeep))
    assert [2 * e.stats[k] for k in ref.COUNT_NAMES] == [adj.stats[k] for k in ("entries", "boundary", "manifold", "nonmanifold")] and e.stats["nonmanifold"] > 0
    assert mesh_edges(1025, _faces(sf)).length is None


# ---- the rounds -------------------------------------------------------------------------------------------------------------------------------------
def _assert_rounds(r, want, V0):
    _same(r.vertices, want["vertices"], "vertices")
    _same(r.faces, want["faces"], "faces")
    _same(r.face_parent, want["face_parent"], "face_parent")
    _same(r.vertex_edge, want["vertex_edge"], "vertex_edge")
    assert r.stats["rounds"] == want["rounds"] and r.stats["converged"] == want["converged"]
    assert [[t[k] for k in ref.TOTAL_NAMES] for t in r.stats["per_round"]] == want["per_round"]
    assert r.new_vertex.tolist() == [False] * V0 + [True] * (len(want["vertices"]) - V0)
    if want["attributes"] is not None:
        _same(r.vertex_attributes, want["attributes"], "vertex_attributes")
        assert np.array_equal(r.attribute_valid.cpu().numpy(), want["valid"]) and r.attribute_valid.dtype == torch.bool


@pytest.mark.parametrize("rounds", [2, 3])
def test_rounds_of_split_long_edges_match_the_reference_iterated(rounds):
    from diff_recon_hip import split_long_edges
    v, f = _latlong_sphere()
    med = _median_edge(v, f)
    max_edge = med * {2: 0.45, 3: 0.3}[rounds]  # the longest edge is 1.7 median edges: 2 and 3 halvings
    a, valid = _attributes(len(v), 3, 7)
    colour = np.arange(len(f), dtype=np.float32)[:, None] * np.ones((1, 3), np.float32)
    want = ref.split_rounds(v, f, 16, max_edge=max_edge, attributes=a, attr_valid=valid)
    assert want["rounds"] == rounds and want["converged"]
    r = split_long_edges(_dev(v), _faces(f), max_edge=max_edge, vertex_attributes=_dev(a), attribute_valid=_dev(valid), face_attributes=_dev(colour))
    _assert_rounds(r, want, len(v))
    _same(r.face_attributes, colour[want["face_parent"]], "face_attributes")
    t = ref.edges(len(want["vertices"]), want["faces"], vertices=want["vertices"])
    assert t["edge_length2"][:t["E"]].max() <= np.float64(np.float32(max_edge)) ** 2 and t["counts"][1] == t["counts"][3] == 0
    # stopped early: not converged, and the same mesh as the reference stopped there
    short = split_long_edges(_dev(v), _faces(f), max_edge=max_edge, max_rounds=rounds - 1)
    _assert_rounds(short, ref.split_rounds(v, f, rounds - 1, max_edge=max_edge), len(v))
    assert not short.stats["converged"]
    # a per-vertex limit, with a keep mask that the pieces inherit, with and without a validity mask beside it
    limit = (med * np.random.default_rng(rounds).uniform(0.3, 2.0, len(v))).astype(np.float32)
    keep = np.arange(len(f)) % 5 != 0
    for ok in (None, valid):
        want = ref.split_rounds(v, f, 16, vertex_limit=limit, attributes=a, attr_valid=ok, keep=keep)
        r = split_long_edges(_dev(v), _faces(f), vertex_limit=_dev(limit), vertex_attributes=_dev(a), attribute_valid=_opt(ok, np.uint8),
                             keep=_dev(keep))
        _assert_rounds(r, want, len(v))
        assert want["rounds"] >= 2 and want["converged"]


@pytest.mark.parametrize("solid", ["cube", "sphere"])
def test_two_levels_of_a_closed_solid_stay_closed_and_cross_nowhere(solid):
    """The cube grid has coordinates that are multiples of 4, so both levels of midpoints are exact, the 16 pieces of a parent lie exactly in
    its plane and self_intersections' float64 predicates decide exactly: no crossing before, none after.  On the lat-long sphere the
    midpoints are rounded to fp32, the pieces of a parent are coplanar only to that rounding, and the overlap query (whose header says it is
    no proof about the geometry of the real numbers) reports rounding noise of nearly coplanar pairs as crossings: 165 on the MI355X.  That
    figure is printed, not asserted; everything else is asserted on both solids."""
    from diff_recon_hip import mesh_topology, self_intersections, subdivide_mesh
    v, f = ref.cube_grid(4, 4) if solid == "cube" else _latlong_sphere()
    vd, fd = _dev(v), _faces(f)
    before = mesh_topology(len(v), fd)
    assert before["boundary"] == 0 and self_intersections((vd, fd)).stats["crossing"] == 0
    r = subdivide_mesh(vd, fd, levels=2)
    _assert_rounds(r, ref.split_rounds(v, f, 2), len(v))
    after = mesh_topology(r.vertices.shape[0], r.faces)
    assert r.faces.shape[0] == 16 * len(f) and r.stats["rounds"] == 2
    assert (after["boundary"], after["nonmanifold"], after["pieces"], after["euler"]) == (0, 0, before["pieces"], before["euler"])
    crossing = self_intersections((r.vertices, r.faces)).stats["crossing"]
    print(f"{solid}: {len(f)} -> {r.faces.shape[0]} faces, {crossing} crossing pairs reported after two levels")
    if solid == "cube":
        assert crossing == 0
    assert torch.equal(r.face_parent, torch.arange(len(f), device=DEV, dtype=torch.int32).repeat_interleave(16))


def test_split_fused_returns_the_kind_of_mesh_it_was_given():
    from diff_recon_hip import mesh_edges, split_fused, weld_mesh
    from diff_recon_hip.color_volume import ColoredMesh
    v, f = _latlong_sphere()
    colour = np.random.default_rng(3).uniform(0, 1, (len(f), 3)).astype(np.float32)
    w = weld_mesh(_dev(v), _faces(f), _dev(colour), eps=0.0)
    med = _median_edge(v, f)
    out = split_fused(w, 0.6 * med)
    assert type(out) is type(w) and out.vertex_map is w.vertex_map and out.face_keep is w.face_keep
    parent = out.stats["split"]["face_parent"]
    assert torch.equal(out.faces_color, w.faces_color[parent.to(torch.int64)]) and out.stats["split"]["converged"]
    assert out.stats["num_faces"] == out.faces.shape[0] > w.faces.shape[0] and out.stats["num_vertices"] == out.vertices.shape[0]
    assert float(mesh_edges(out.vertices.shape[0], out.faces, vertices=out.vertices).length.max()) <= np.float32(0.6 * med)
    vc, valid = _attributes(len(v), 3, 9)
    c = ColoredMesh(_dev(v), _faces(f), _dev(vc), _dev(valid != 0), {"num_vertices": len(v), "num_faces": len(f)})
    out = split_fused(c, 0.6 * med)
    want = ref.split_rounds(v, f, 16, max_edge=0.6 * med, attributes=vc, attr_valid=valid)
    assert type(out) is ColoredMesh and np.array_equal(out.color_valid.cpu().numpy(), want["valid"])
    _same(out.vertex_color, np.where(want["valid"][:, None], want["attributes"], np.float32(0.5)), "vertex_color")
    _same(out.faces, want["faces"], "faces")


def test_example_reports_the_split_mesh():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    plain = train_synthetic.mesh_scores(m, "2D", weld=0.02, **cfg)["welded"]
    res = train_synthetic.mesh_scores(m, "2D", weld=0.02, split_edges=20.0, **cfg)["welded"]
    s = res["split"]
    lines = train_synthetic.split_edges_report(s)
    print("\n".join(lines))
    same = ("psnr", "ssim", "mean_psnr", "mean_ssim", "topology", "eps", "soup")
    assert "split" not in plain and set(res) == set(plain) | {"split"} and {k: res[k] for k in same} == {k: plain[k] for k in same}  # no other entry changes
    assert len(lines) == 2 and lines[0].startswith(f"split mesh, no edge above 20: faces {s['before']['faces']} -> {s['faces']} in {s['rounds']} rounds")
    assert f"mean PSNR {s['before']['mean_psnr']:.2f} -> {s['mean_psnr']:.2f} dB" in lines[1]
    assert s["converged"] and s["faces"] > s["before"]["faces"] == plain["topology"]["faces"] and s["max_edge"] == 20.0


# ---- determinism and purity ---------------------------------------------------------------------------------------------------------------------
def test_both_calls_are_pure_and_deterministic():
    v, f, keep, _ = _soup(1025)
    a, valid = _attributes(1025, 3, 6)
    med = _median_edge(v, f, keep)
    limit = (med * np.random.default_rng(1).uniform(0.5, 1.5, 1025)).astype(np.float32)

    def call(pattern):  # every workspace and every output comes from torch.empty and is poisoned, with guard bytes either side
        ev, use, length2, hee, counts = _gpu_edges(1025, f, keep, v)
        out = {"edge_vertices": ev, "edge_use": use, "edge_length2": length2, "half_edge_edge": hee, "counts": counts}
        for mode, name in ((ref.MARK_ALL, "all"), (ref.MARK_LONGER, "longer"), (ref.MARK_VERTEX_LIMIT, "limit")):
            names = ("new_vertices", "new_attributes", "new_attr_valid", "new_vertex_edge", "out_faces", "out_face_parent", "totals")
            out.update({f"{name}.{n}": t for n, t in zip(names, _gpu_split(v, f, keep, mode, med, limit, a, valid))})
        return out

    base = poison.assert_pure(call)  # twice on zeros first: the same call repeated gives identical bytes
    want = ref.split(v, f, keep, ref.MARK_LONGER, med, None, a, valid)
    assert base["longer.out_faces"].numpy().tobytes() == want["out_faces"].tobytes()
    assert base["longer.new_vertices"].numpy().tobytes() == want["new_vertices"].tobytes()
    assert base["edge_length2"].numpy().tobytes() == ref.edges(1025, f, keep, v)["edge_length2"].tobytes()
    assert 0 < want["totals"][1] < want["totals"][0] and want["totals"][3] > 0
