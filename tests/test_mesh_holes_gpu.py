"""GPU tests of hole filling against tests/ref_mesh_holes.py, everything bit for bit and to its capacity: half_edge_loop, loop_offsets,
loop_half_edges, counts, loop_status, the new vertices / attributes / valid bytes / faces / new_face_loop and totals; the no-ops; determinism
and purity; mesh_topology of the filled meshes; fill_fused on the device's own level set; smoothing the caps alone; the example's line."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import poison
import ref_mesh_holes as ref
import ref_mesh_simplify as fixtures
import ref_mesh_smooth
import ref_volume
from test_mesh_smooth_gpu import _latlong_sphere, _soup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
LIMITS = (0, 3, 8, None)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _faces(f):
    return _dev(np.asarray(f, np.int32).reshape(-1, 3))


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    if g.dtype.itemsize == 4:
        g, w = g.view(np.uint32), w.view(np.uint32)
    diff = np.nonzero(g != w)[0]
    assert len(diff) == 0, (what, len(diff), diff[:5], g[diff[:5]], w[diff[:5]])


def _gpu_loops(V, f, keep=None, table=None):
    """All of tsh_loops' outputs to their capacity, on the device, with the reference's adjacency table (or `table`) as the input."""
    from diff_recon_hip import mesh_holes
    fd = _faces(f)
    offsets, neighbors, edge_faces, entries = table if table is not None else (ref.table_of(V, f, keep) if V else (np.zeros(1, np.int32),) * 3 + (0,))
    nd, ed = (_dev(np.asarray(x, np.int32)) for x in (neighbors, edge_faces))
    return mesh_holes._loops_arrays(V, fd, None if keep is None else _dev(keep), _dev(np.asarray(offsets, np.int32)), nd, ed, int(entries), fd.device)


def _assert_loops(got, want):
    half_edge_loop, loop_offsets, loop_half_edges, counts = got
    _same(half_edge_loop, want["half_edge_loop"], "half_edge_loop")
    _same(loop_offsets, want["loop_offsets"], "loop_offsets")        # all F + 1 entries: the member total past the loops
    _same(loop_half_edges, want["loop_half_edges"], "loop_half_edges")  # all 3 F entries: -1 past the member total
    assert counts.tolist() == want["counts"] and counts.dtype == torch.int64


def _assert_fill(v, f, lp, limit, attributes=None, attr_valid=None):
    """tsh_fill on the reference's loops (trimmed, as boundary_loops hands them on) against ref.fill, every output to its capacity."""
    from diff_recon_hip import mesh_holes
    n, members = lp["num_loops"], lp["num_members"]
    want = ref.fill(v, f, lp, ref.UNBOUNDED if limit is None else limit, attributes, attr_valid)
    vd, fd = _dev(np.asarray(v, np.float32)), _faces(f)
    got = mesh_holes._fill_arrays(vd, fd, _dev(lp["loop_offsets"][:n + 1]), _dev(lp["loop_half_edges"][:members]), n, members,
                                  mesh_holes.UNBOUNDED if limit is None else limit, None if attributes is None else _dev(attributes),
                                  None if attr_valid is None else _dev(attr_valid), vd.device)
    status, new_vertices, new_attrs, new_valid, new_faces, new_face_loop, totals = got
    _same(status, want["loop_status"], ("loop_status", limit))
    _same(new_vertices, want["new_vertices"], ("new_vertices", limit))
    if attributes is not None:
        _same(new_attrs, want["new_attributes"], ("new_attributes", limit))
        _same(new_valid, want["new_attr_valid"], ("new_attr_valid", limit))
    _same(new_faces, want["new_faces"], ("new_faces", limit))
    _same(new_face_loop, want["new_face_loop"], ("new_face_loop", limit))
    assert totals.tolist() == want["totals"] and totals.dtype == torch.int64
    return want


def _assert_everything(v, f, keep=None, table=None, attributes=None, attr_valid=None, limits=LIMITS):
    V = len(v)
    want = ref.loops(V, f, keep, table)
    _assert_loops(_gpu_loops(V, f, keep, table), want)
    fills = {limit: _assert_fill(v, f, want, limit, attributes, attr_valid) for limit in limits}
    return want, fills


# ---- the CPU fixtures -------------------------------------------------------------------------------------------------------------------------
def _pinched_sphere():
    v, f = fixtures.sphere_mesh()
    fan = np.nonzero((f == 100).any(1))[0]
    pair = next((a, b) for a in fan for b in fan if a < b and len(set(f[a]) & set(f[b])) == 1)
    return v, np.delete(f, pair, axis=0)


FIXTURES = {
    "punched": ref.punched_sphere,
    "capped": ref.capped_sphere,
    "plane": lambda: fixtures.plane_grid()[:2],
    "fused": ref.fused_sphere,
    "nan_blocks": ref.nan_block_sphere,
    "lone": lambda: (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]])),
    "pinched": _pinched_sphere,
    "closed": fixtures.sphere_mesh,
}
CLOSES = ("punched", "capped", "plane", "fused", "nan_blocks")


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return FIXTURES[name]()


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixtures_match_the_reference_bit_for_bit(name):
    v, f = _fixture(name)
    rng = np.random.default_rng(17)
    attributes = rng.uniform(0, 1, (len(v), 3)).astype(np.float32)
    attr_valid = (rng.integers(0, 3, len(v)) != 0).astype(np.uint8)
    want, fills = _assert_everything(v, f, attributes=attributes, attr_valid=attr_valid)
    if name == "punched":
        assert want["counts"] == [108, 108, 17, 0] and fills[None]["totals"] == [17, 12, 98] and fills[8]["totals"][0] == 13
        assert fills[3]["totals"] == [5, 0, 5] and fills[0]["totals"] == [0, 0, 0]
    if name == "pinched":
        assert want["counts"] == [6, 0, 0, 1]
    if name == "lone":
        assert fills[None]["loop_status"].tolist() == [ref.LONE_FACE] and fills[0]["loop_status"].tolist() == [ref.TOO_LONG]


@pytest.mark.parametrize("name", CLOSES)
def test_filled_fixtures_are_closed_on_the_device(name):
    from diff_recon_hip import boundary_loops, fill_holes, loop_vertices, mesh_topology
    v, f = _fixture(name)
    vd, fd = _dev(v), _faces(f)
    before = mesh_topology(len(v), fd)
    filled = fill_holes(vd, fd)
    after = mesh_topology(filled.vertices.shape[0], filled.faces)
    assert before["boundary"] > 0 and (after["boundary"], after["nonmanifold"], after["euler"]) == (0, 0, 2)
    # the old vertices and faces come first, bit for bit; the masks and the statistics
    V, F = len(v), len(f)
    assert torch.equal(filled.vertices[:V].view(torch.int32), vd.view(torch.int32)) and torch.equal(filled.faces[:F], fd)
    assert filled.new_vertex.dtype == torch.bool and not filled.new_vertex[:V].any() and filled.new_vertex[V:].all()
    assert (filled.face_loop[:F] == -1).all() and (filled.face_loop[F:] >= 0).all() and filled.face_loop.dtype == torch.int32
    want = ref.loops(V, f)
    lengths = ref.loop_lengths(want)
    s = filled.stats
    assert [s[k] for k in ("boundary_half_edges", "loop_half_edges", "loops", "nonsimple_vertices")] == want["counts"] and s["open_half_edges"] == 0
    assert s["filled_loops"] == s["filled"] == len(lengths) and s["too_long"] == s["lone_face"] == s["dead"] == 0 and s["longest_loop"] == lengths.max()
    assert s["new_vertices"] == filled.vertices.shape[0] - V == int((lengths > 3).sum()) and s["new_faces"] == filled.faces.shape[0] - F
    assert filled.vertex_attributes is None and filled.attribute_valid is None
    # the trimmed loops and their vertices
    loops = boundary_loops(V, fd)
    assert loops.loop_offsets.shape == (len(lengths) + 1,) and loops.loop_half_edges.shape == (int(lengths.sum()),)
    tails = loop_vertices(loops, fd)
    assert np.array_equal(tails.cpu().numpy(), want["tail"][want["loop_half_edges"][:want["num_members"]]]) and tails.dtype == torch.int32
    again = fill_holes(vd, fd, loops=loops)
    assert torch.equal(again.faces, filled.faces) and torch.equal(again.vertices.view(torch.int32), filled.vertices.view(torch.int32))
    if name == "fused":
        none = fill_holes(vd, fd, max_loop_edges=32)
        assert none.stats["filled_loops"] == 0 and none.stats["too_long"] == 12 and none.faces.shape[0] == F and none.vertices.shape[0] == V


# ---- open bands: long loops across blocks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(3, 4, 5), (255, 256, 257, 4, 3), (1025, 5, 2049, 3)])
def test_open_bands_match_the_reference_bit_for_bit(sizes):
    v, f = ref.open_bands(sizes, seed=len(sizes))
    rng = np.random.default_rng(3)
    attributes = rng.uniform(-1, 1, (len(v), 2)).astype(np.float32)
    want, fills = _assert_everything(v, f, attributes=attributes, limits=(0, 3, 8, 256, None))
    assert sorted(ref.loop_lengths(want).tolist()) == sorted(list(sizes) * 2) and want["counts"][3] == 0
    assert fills[None]["totals"][0] == 2 * len(sizes) and fills[256]["totals"][0] == 2 * sum(n <= 256 for n in sizes)
    from diff_recon_hip import fill_holes, mesh_topology
    filled = fill_holes(_dev(v), _faces(f))
    topo = mesh_topology(filled.vertices.shape[0], filled.faces)
    assert topo["boundary"] == 0 and topo["nonmanifold"] == 0 and topo["pieces"] == len(sizes) and topo["euler"] == 2 * len(sizes)


# ---- random soups -----------------------------------------------------------------------------------------------------------------------------
def _holes_soup(V):
    """test_mesh_smooth_gpu's soup -- indices -1 and V, repeated indices, duplicated, rotated and reversed triples, NaN / inf vertices --
    and, from V = 257 on, two closed fans of six faces on vertices 20 .. 33, which no other face names any more: two holes of six edges, one of
    them with a NaN vertex on its loop, so that not everything is open.  F = 2 V + 12."""
    v, f, keep, _ = _soup(V)
    if V < 257:
        return v, f, keep
    v, f = v.copy(), f.copy()
    f[np.isin(f, np.arange(20, 34))] = 0
    fans = [(c, c + 1 + i, c + 1 + (i + 1) % 6) for c in (20, 27) for i in range(6)]
    v[20:34] = np.random.default_rng(V).uniform(-3.0, 3.0, (14, 3)).astype(np.float32)
    v[23, 1] = np.nan
    return v, np.concatenate([f, np.array(fans)]), np.concatenate([keep, np.ones(12, np.uint8)])


@pytest.mark.parametrize("V", [1, 2, 63, 257, 1025, 4097])
def test_random_soups_match_the_reference_bit_for_bit(V):
    v, f, keep = _holes_soup(V)
    rng = np.random.default_rng(V)
    attributes = rng.uniform(0, 1, (V, 4)).astype(np.float32)
    attr_valid = (rng.integers(0, 2, V)).astype(np.uint8)
    for k in (None, keep):
        want, fills = _assert_everything(v, f, k, attributes=attributes, attr_valid=attr_valid)
        print(f"soup V = {V}, keep {'on' if k is not None else 'off'}: counts {want['counts']}, statuses {np.bincount(fills[None]['loop_status'], minlength=4).tolist()}")
        if V >= 63:
            assert want["counts"][0] > want["counts"][1] and want["counts"][3] > 0  # almost everything is open there
        if V >= 257:
            status = fills[None]["loop_status"]
            assert (status == ref.DEAD).sum() >= 1 and (status == ref.FILLED).sum() >= 1 and fills[3]["totals"][1] == 0
    if V >= 63:  # a foreign table: the same rows, cut at a short num_entries
        offsets, neighbors, edge_faces, entries = ref.table_of(V, f)
        short = (offsets, neighbors[:entries // 3], edge_faces[:entries // 3], entries // 3)
        want, _ = _assert_everything(v, f, None, table=short, limits=(None,))
        assert 0 < want["counts"][0] < ref.loops(V, f)["counts"][0]


def test_soup_with_holes_whose_vertices_are_dead():
    """Loops on a soup: the punched sphere with NaN and infinite vertices on some loops, an out-of-range face, a repeated one and a `keep`
    that opens one more hole."""
    v, f = _fixture("punched")
    v, f = v.copy(), f.copy()
    lp = ref.loops(len(v), f)
    tails = lp["tail"][lp["loop_half_edges"][:lp["num_members"]]]
    off = lp["loop_offsets"]
    v[tails[off[2]], 0] = np.nan
    v[tails[off[9] + 1], 2] = -np.inf
    f = np.concatenate([f, [[0, 1, len(v)], [-1, 2, 3]], f[:3]])  # two faces that do not take part; three duplicates (edges used 3 times)
    keep = np.ones(len(f), np.uint8)
    keep[1000] = 0
    want, fills = _assert_everything(v, f)
    assert (fills[None]["loop_status"] == ref.DEAD).sum() == 2 and fills[None]["totals"][0] == want["num_loops"] - 2
    kept, _ = _assert_everything(v, f, keep)
    assert kept["counts"][0] == want["counts"][0] + 3  # the dropped face's three edges are boundary now


def test_no_faces_and_no_vertices_are_no_ops():
    from diff_recon_hip import boundary_loops, fill_holes
    f0 = torch.zeros((0, 3), device=DEV, dtype=torch.int32)
    v0 = torch.zeros((0, 3), device=DEV)
    for V in (0, 5):
        loops = boundary_loops(V, f0)
        assert loops.half_edge_loop.shape == (0,) and loops.loop_offsets.tolist() == [0] and loops.loop_half_edges.shape == (0,)
        assert loops.stats == {"boundary_half_edges": 0, "loop_half_edges": 0, "loops": 0, "nonsimple_vertices": 0, "open_half_edges": 0}
    got = _gpu_loops(0, np.zeros((4, 3), np.int64))  # faces without vertices: nothing takes part, everything is still written
    _assert_loops(got, ref.loops(0, np.zeros((4, 3), np.int64)))
    v = torch.zeros((5, 3), device=DEV)
    filled = fill_holes(v, f0, vertex_attributes=torch.ones((5, 2), device=DEV))
    assert filled.vertices.shape == (5, 3) and filled.faces.shape == (0, 3) and filled.loop_status.shape == (0,) and filled.stats["filled_loops"] == 0
    assert filled.vertex_attributes.shape == (5, 2) and filled.attribute_valid.all() and not filled.new_vertex.any()
    filled = fill_holes(v0, f0)
    assert filled.vertices.shape == (0, 3) and filled.faces.shape == (0, 3) and filled.stats["loops"] == 0


# ---- determinism and purity ---------------------------------------------------------------------------------------------------------------------
def test_both_calls_are_pure_and_deterministic():
    from diff_recon_hip import mesh_holes
    v, f = ref.open_bands((257, 5, 3, 40), seed=9)
    v2, f2 = _fixture("punched")
    f = np.concatenate([f, f2 + len(v), [[0, 0, 1], [-1, 5, 6]]])
    v = np.concatenate([v, v2])
    V = len(v)
    keep = np.ones(len(f), np.uint8)
    keep[610::97] = 0  # behind the 610 faces of the bands: every face dropped from the sphere opens a hole of three
    rng = np.random.default_rng(1)
    attributes = rng.uniform(0, 1, (V, 3)).astype(np.float32)
    attr_valid = (rng.integers(0, 2, V)).astype(np.uint8)
    table = ref.table_of(V, f, keep)
    want = ref.loops(V, f, keep, table)
    n, members = want["num_loops"], want["num_members"]

    def call(pattern):  # every workspace and every output comes from torch.empty and is poisoned, with guard bytes either side
        vd, fd = _dev(v), _faces(f)
        half_edge_loop, loop_offsets, loop_half_edges, counts = _gpu_loops(V, f, keep, table)
        fill = mesh_holes._fill_arrays(vd, fd, loop_offsets[:n + 1].contiguous(), loop_half_edges[:members].contiguous(), n, members, 64,
                                       _dev(attributes), _dev(attr_valid), vd.device)  # in a fresh, poisoned workspace of its own
        names = ("loop_status", "new_vertices", "new_attributes", "new_attr_valid", "new_faces", "new_face_loop", "totals")
        return {"half_edge_loop": half_edge_loop, "loop_offsets": loop_offsets, "loop_half_edges": loop_half_edges, "counts": counts,
                **dict(zip(names, fill))}

    base = poison.assert_pure(call)
    assert base["loop_half_edges"].numpy().tobytes() == want["loop_half_edges"].tobytes()
    expect = ref.fill(v, f, want, 64, attributes, attr_valid)
    assert base["new_vertices"].numpy().tobytes() == expect["new_vertices"].tobytes()
    assert base["new_faces"].numpy().tobytes() == expect["new_faces"].tobytes()
    assert (expect["loop_status"] == ref.TOO_LONG).sum() == 2 and expect["totals"][0] > 10


# ---- the public wrappers ------------------------------------------------------------------------------------------------------------------------
def _cams():
    return [SimpleNamespace(world_view_transform=_dev(np.asarray(ref_volume.look_at_view(eye), np.float32)), tan_fovx=0.45, tan_fovy=0.45,
                            image_width=48, image_height=48, device="cuda:0") for eye in ref_volume.AXIS_EYES]


def test_fill_fused_closes_the_uncarved_fusion_of_both_kinds():
    """The six axis views of the fusion's end-to-end test, integrated WITHOUT carving: the level set ends where no view saw the volume."""
    from diff_recon_hip import MeshRenderer, fill_fused, mesh_topology
    from diff_recon_hip.color_volume import ColorTSDFVolume
    from diff_recon_hip.volume import TSDFVolume, fusion_bounds
    v, f = _latlong_sphere()
    vd, fd = _dev(v), _dev(f)
    colour = _dev(np.full((len(f), 3), 0.25, np.float32))
    plain, coloured = TSDFVolume(*fusion_bounds(vd, 24), DEV), ColorTSDFVolume(*fusion_bounds(vd, 24), DEV)
    for cam in _cams():
        out = MeshRenderer(cam).render(vertices=vd, faces=fd, faces_color=colour)
        plain.integrate(cam, out["depth"], carve_uncovered=False)
        coloured.integrate(cam, out["depth"], image=out["render"], carve_uncovered=False)
    for mesh in (plain.extract(), coloured.extract()):
        V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
        before = mesh_topology(V, mesh.faces)
        lp = ref.loops(V, mesh.faces.cpu().numpy())
        assert before["boundary"] > 0 and lp["num_loops"] > 0 and lp["counts"][0] == before["boundary"]
        limit = int(ref.loop_lengths(lp).max())
        out = fill_fused(mesh, limit)
        assert type(out) is type(mesh)
        after = mesh_topology(out.vertices.shape[0], out.faces)
        print(f"{type(mesh).__name__}: {lp['num_loops']} loops of up to {limit} edges, {lp['counts'][0] - lp['counts'][1]} open half-edges; boundary "
              f"{before['boundary']} -> {after['boundary']}, Euler {before['euler']} -> {after['euler']}")
        assert after["boundary"] == lp["counts"][0] - lp["counts"][1] and after["nonmanifold"] == before["nonmanifold"]
        s = out.stats["fill"]
        assert s["filled_loops"] == s["loops"] == lp["num_loops"] and out.stats["num_vertices"] == out.vertices.shape[0] == V + s["new_vertices"]
        assert out.stats["num_faces"] == out.faces.shape[0] == F + s["new_faces"]
        assert {k: x for k, x in out.stats.items() if k not in ("fill", "num_vertices", "num_faces")} == \
               {k: x for k, x in mesh.stats.items() if k not in ("num_vertices", "num_faces")}
        want = ref.fill(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), lp, limit)
        _same(out.vertices[V:], want["new_vertices"][:want["totals"][1]], "fill_fused vertices")
        _same(out.faces[F:], want["new_faces"][:want["totals"][2]], "fill_fused faces")
        if hasattr(mesh, "vertex_color"):
            assert out.vertex_color.shape == (out.vertices.shape[0], 3) and out.color_valid.dtype == torch.bool
            assert torch.equal(out.color_valid[:V], mesh.color_valid) and torch.equal(out.vertex_color[:V][mesh.color_valid], mesh.vertex_color[mesh.color_valid])
            assert torch.isfinite(out.vertex_color).all() and (out.vertex_color[~out.color_valid] == 0.5).all()
            lo, hi = mesh.vertex_color[mesh.color_valid].min(), mesh.vertex_color[mesh.color_valid].max()
            assert (out.vertex_color[V:][out.color_valid[V:]] >= lo).all() and (out.vertex_color[V:][out.color_valid[V:]] <= hi).all()  # a mean
        else:
            assert out.vertex_map is mesh.vertex_map and out.face_keep is mesh.face_keep and out.faces_color is None
        none = fill_fused(mesh, 2)
        assert none.faces.shape[0] == F and none.stats["fill"]["too_long"] == lp["num_loops"]


def test_smoothing_the_caps_alone_moves_only_new_vertices():
    """A cap's vertex is born at the mean of its neighbours, where a Laplacian step leaves it up to the rounding; pushed away from there, it
    comes back, and the mesh it closes stays where it is bit for bit."""
    from diff_recon_hip import fill_holes, smooth_mesh
    v, f = _fixture("punched")
    filled = fill_holes(_dev(v), _faces(f))
    V = len(v)
    assert int(filled.new_vertex.sum()) == 12
    adjacency = ref_mesh_smooth.adjacency(V + 12, filled.faces.cpu().numpy())
    pinned = ~filled.new_vertex
    for push in (0.0, 0.3):
        start = filled.vertices.clone()
        start[V:] += push
        smoothed = smooth_mesh(start, filled.faces, iterations=5, pinned=pinned)
        moved = (smoothed.vertices.view(torch.int32) != start.view(torch.int32)).any(dim=1)
        assert not moved[:V].any() and smoothed.stats["moved"] == int(moved.sum()) <= 12
        assert torch.equal(smoothed.vertices[:V].view(torch.int32), _dev(v).view(torch.int32))
        want = ref_mesh_smooth.smooth(start.cpu().numpy(), adjacency, iterations=5, pinned=pinned.cpu().numpy())
        _same(smoothed.vertices, want, ("smoothed caps", push))
        if push:
            assert moved[V:].all()
            back = (smoothed.vertices[V:] - filled.vertices[V:]).norm(dim=1)
            # its neighbours are pinned, so an iteration scales its offset from their mean by (1 - 0.5) (1 + 0.53) = 0.765: 0.765^5 = 0.26
            assert (back < 0.5 * push * 3 ** 0.5).all()


def test_example_reports_the_filled_mesh():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    res = train_synthetic.mesh_scores(m, "2D", extract=24, fill=16, smooth=3, **cfg)
    fused = res["fused"]
    lines = train_synthetic.filled_report(fused)
    print("\n".join(lines))
    s, before, after = fused["filled"], fused["topology"], fused["filled"]["topology"]
    assert len(lines) == 1 and lines[0].startswith("filled mesh, loops of up to 16 edges: ")
    assert f"{s['loops']} loops, {s['filled_loops']} filled" in lines[0] and f"{s['open_half_edges']} open half-edges" in lines[0]
    assert f"{before['boundary']} -> {after['boundary']} boundary edges" in lines[0] and f"Euler characteristic {before['euler']} -> {after['euler']}" in lines[0]
    assert s["boundary_half_edges"] == before["boundary"] and s["filled_loops"] == s["filled"] and s["loops"] == sum(s[k] for k in ref.STATUS)
    assert after["faces"] == before["faces"] + s["new_faces"] and after["boundary"] <= before["boundary"]
    assert fused["smoothed"]["topology"] == after and "topology unchanged" in train_synthetic.smoothed_report(fused)[0]  # the smoothing follows the fill
    plain = train_synthetic.mesh_scores(m, "2D", extract=24, **cfg)["fused"]
    assert "filled" not in plain and plain["topology"] == before and plain["to_soup"] == fused["to_soup"]  # the defaults stay
