"""GPU tests of the non-manifold split against tests/ref_mesh_manifold.py, everything bit for bit and to its capacity: corner_fan, vertex_fans,
counts, out_faces, new_vertex_source and new_vertex_fan with their -1 tail, and totals; the promises on the device's own output; the no-ops;
determinism and purity; the chain simplify -> split -> topology -> loops -> fill; manifold_fused on the device's own fusion; the example's line."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import poison
import ref_mesh_holes
import ref_mesh_manifold as ref
import ref_mesh_simplify as fixtures
import ref_volume
from test_mesh_smooth_gpu import _latlong_sphere, _soup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


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


def _gpu_fans(V, f, keep=None):
    from diff_recon_hip import mesh_manifold
    fd = _faces(f)
    return mesh_manifold._fans_arrays(V, fd, None if keep is None else _dev(np.asarray(keep, np.uint8)), fd.device)


def _gpu_split(V, f, corner_fan, keep=None, capacity=0):
    from diff_recon_hip import mesh_manifold
    fd = _faces(f)
    table = corner_fan if isinstance(corner_fan, torch.Tensor) else _dev(np.asarray(corner_fan, np.int32))
    return mesh_manifold._split_arrays(V, fd, None if keep is None else _dev(np.asarray(keep, np.uint8)), table, capacity, fd.device)


def _assert_split(V, f, table, keep, capacity, got_table=None):
    want = ref.split(V, f, table, keep, capacity)
    out_faces, source, label, totals = _gpu_split(V, f, table if got_table is None else got_table, keep, capacity)
    _same(out_faces, want["out_faces"], ("out_faces", capacity))
    _same(source, want["new_vertex_source"], ("new_vertex_source", capacity))  # to the capacity: -1 past the number of new vertices
    _same(label, want["new_vertex_fan"], ("new_vertex_fan", capacity))
    assert totals.tolist() == want["totals"] and totals.dtype == torch.int64
    return want, out_faces


def _assert_everything(V, f, keep=None, slack=5):
    """tsf_fans and tsf_split (on the device's own table) against the reference, every output to its capacity -- a capacity above and exactly
    at the number of new vertices -- then the promises, by calling the device a second time on its own output."""
    want = ref.fans(V, f, keep)
    corner_fan, vertex_fans, counts = _gpu_fans(V, f, keep)
    _same(corner_fan, want["corner_fan"], "corner_fan")
    _same(vertex_fans, want["vertex_fans"], "vertex_fans")
    assert counts.tolist() == want["counts"] and counts.dtype == torch.int64
    new = want["new_vertices"]
    _assert_split(V, f, want["corner_fan"], keep, new + slack, corner_fan)
    sp, out_faces = _assert_split(V, f, want["corner_fan"], keep, new, corner_fan)
    assert sp["totals"][0] == new
    # the promises on the device: who took part is told to the second pass (a row with an index in [V, V + new) would take part now)
    part = ref.participation(V, f, keep).astype(np.uint8)
    g = out_faces.cpu().numpy()
    fan2, per_vertex2, counts2 = _gpu_fans(V + new, g, part)
    assert counts2.tolist()[3:5] == [0, 0] and counts2.tolist()[:2] == want["counts"][:2] and int(per_vertex2.max().item() if V + new else 0) <= 1
    again, source2, _, totals2 = _gpu_split(V + new, g, fan2, part, slack)
    assert torch.equal(again, out_faces) and totals2.tolist() == [0, 0] and (source2 == -1).all()
    return want, sp


# ---- the CPU fixtures -------------------------------------------------------------------------------------------------------------------------
def _pinched_sphere():
    v, f = fixtures.sphere_mesh()
    fan = np.nonzero((f == 100).any(1))[0]
    pair = next((a, b) for a in fan for b in fan if a < b and len(set(f[a]) & set(f[b])) == 1)
    return v, np.delete(f, pair, axis=0)


@functools.lru_cache(maxsize=None)
def _simplified(cell):
    v, f = fixtures.sphere_mesh()
    s = fixtures.simplify(v, f, cell, v.min(0) - 0.01)
    return s["vertices"], s["faces"]


FIXTURES = {
    "sphere": lambda: (len(fixtures.sphere_mesh()[0]), fixtures.sphere_mesh()[1]),
    "pinched": lambda: (len(_pinched_sphere()[0]), _pinched_sphere()[1]),
    "kissing": lambda: (lambda v, f: (len(v), f))(*ref.kissing(*fixtures.sphere_mesh())),
    "tetrahedra": ref.two_tetrahedra,
    "cell2": lambda: (len(_simplified(2.0)[0]), _simplified(2.0)[1]),
    "cell4": lambda: (len(_simplified(4.0)[0]), _simplified(4.0)[1]),
    "cell6": lambda: (len(_simplified(6.0)[0]), _simplified(6.0)[1]),
    "cell8": lambda: (len(_simplified(8.0)[0]), _simplified(8.0)[1]),
    "soup63": lambda: (63, ref.soups()[63]),
    "soup257": lambda: (257, ref.soups()[257]),
    "soup1025": lambda: (1025, ref.soups()[1025]),
}
FIGURES = {"sphere": (0, 0, 0), "pinched": (1, 1, 0), "kissing": (1, 1, 0), "tetrahedra": (2, 2, 1), "cell2": (30, 63, 30), "cell4": (17, 35, 16),
           "cell6": (15, 63, 18), "cell8": (3, 5, 2), "soup63": (62, 240, 1), "soup257": (247, 1180, 0), "soup1025": (1007, 5044, 0)}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixtures_match_the_reference_bit_for_bit(name):
    V, f = FIXTURES[name]()
    want, sp = _assert_everything(V, f)
    assert (want["counts"][3], want["new_vertices"], want["counts"][4]) == FIGURES[name]
    if name == "sphere":
        assert np.array_equal(sp["out_faces"], np.asarray(f, np.int32))  # a manifold input comes back bit for bit


# ---- books, hubs, cones: the parent words under contention, runs and chains across blocks ---------------------------------------------------------
@pytest.mark.parametrize("k", [3, 4, 255, 256, 257, 1025])
def test_books_match_the_reference_bit_for_bit(k):
    V, f = ref.book(k)
    f = f[np.random.default_rng(k).permutation(k)]
    want, sp = _assert_everything(V, f)
    assert want["vertex_fans"][:2].tolist() == [k, k] and want["counts"] == [3 * k, 3 * k, k + 2, 2, 1, 0] and sp["totals"] == [2 * k - 2, 2 * k - 2]


@pytest.mark.parametrize("n", [2, 257, 2049])
def test_hubs_match_the_reference_bit_for_bit(n):
    V, f = ref.hub(n)
    want, sp = _assert_everything(V, f)
    assert want["vertex_fans"][0] == n and want["new_vertices"] == n - 1 and want["counts"][3] == 1
    assert (sp["new_vertex_source"] == 0).all() and sp["new_vertex_fan"].tolist() == [3 * i for i in range(1, n)]  # one keeper: corner 0


def test_cones_are_one_fan_each_whatever_the_order_of_their_faces():
    sizes = (3, 255, 256, 257, 1025, 2049)
    V, f, apexes = ref.cones(sizes, seed=11)
    want, sp = _assert_everything(V, f)
    for apex, n in apexes:
        assert want["vertex_fans"][apex] == n
    assert want["counts"][3:] == [1, 0, 0] and sp["totals"] == [1, 3]  # the two cones that share only their apex: one of them moves its 3 corners
    flat = np.asarray(f).reshape(-1)
    sizes_of = np.bincount(want["corner_fan"][want["corner_fan"] >= 0])
    big = {int(flat[c]): int(sizes_of[c]) for c in np.nonzero(sizes_of >= 255)[0]}
    assert sorted(big.values()) == sorted([n for n in sizes if n >= 255] * 2)  # thousands of scattered unions, one root each


# ---- random soups -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 2, 63, 257, 1025, 4097])
def test_random_soups_match_the_reference_bit_for_bit(V):
    """test_mesh_smooth_gpu's soup: indices -1 and V, repeated indices, duplicated, rotated and reversed triples, a hub of min(1500, V) faces."""
    _, f, keep, _ = _soup(V)
    for k in (None, keep):
        want, sp = _assert_everything(V, f, k)
        print(f"soup V = {V}, keep {'on' if k is not None else 'off'}: counts {want['counts']}, totals {sp['totals']}")
        part = ref.participation(V, f, k)
        assert np.array_equal(sp["out_faces"][~part], np.asarray(f, np.int32)[~part])  # out-of-range, negative and repeated rows, bit for bit
        if V >= 63:
            assert want["counts"][3] > 0 and want["counts"][4] > 0 and want["vertex_fans"].max() >= min(1500, V) // 4 and (~part).sum() > 0


def test_a_foreign_table_stays_in_bounds():
    V = 257
    _, f, keep, _ = _soup(V)
    want = ref.fans(V, f, keep)
    rng = np.random.default_rng(8)
    table = want["corner_fan"].copy()
    N = len(table)
    who = rng.permutation(N)
    table[who[:100]] = rng.integers(N, 2 ** 31 - 1, 100)                  # out of range
    table[who[100:200]] = -rng.integers(2, 2 ** 31 - 1, 100)              # negative
    table[who[200:400]] = rng.integers(0, N, 200)                          # mostly a corner on another vertex
    excluded = np.nonzero(np.repeat(~ref.participation(V, f, keep), 3))[0]
    table[who[400:500]] = rng.choice(excluded, 100)                        # a corner of a face that does not take part
    table[excluded[:50]] = rng.integers(0, N, 50)                          # entries AT corners that do not take part are not read at all
    flat = np.asarray(f).reshape(-1)
    part = np.repeat(ref.participation(V, f, keep), 3)
    for c in who[500:600]:                                                 # another corner of the same vertex that is no root: a label of its own
        if part[c]:
            table[c] = rng.choice(np.nonzero(part & (flat == flat[c]))[0])
    new = ref.split(V, f, table, keep)["totals"][0]
    for capacity in (new + 3, new, max(new - 5, 0), 0):
        _assert_split(V, f, table, keep, capacity)
    assert 0 < new != want["new_vertices"]


def test_no_faces_and_no_vertices_are_no_ops():
    from diff_recon_hip import split_nonmanifold, vertex_fans
    f0 = torch.zeros((0, 3), device=DEV, dtype=torch.int32)
    zero = dict.fromkeys(ref.COUNT_NAMES + ("new_vertices",), 0)
    for V in (0, 5):
        fans = vertex_fans(V, f0)
        assert fans.corner_fan.shape == (0,) and fans.vertex_fans.tolist() == [0] * V and fans.stats == zero
        out = split_nonmanifold(torch.zeros((V, 3), device=DEV), f0, vertex_attributes=torch.ones((V, 2), device=DEV))
        assert out.vertices.shape == (V, 3) and out.faces.shape == (0, 3) and out.source_vertex.tolist() == list(range(V)) and not out.new_vertex.any()
        assert out.vertex_attributes.shape == (V, 2) and out.attribute_valid.all() and out.stats["corners_rewritten"] == 0
    f = np.array([[0, 1, 2], [3, 4, 5], [-1, 7, 2 ** 31 - 1], [0, 0, 0]])  # faces without vertices: nothing takes part, everything is still written
    want, sp = _assert_everything(0, f)
    assert want["counts"] == [0] * 6 and (want["corner_fan"] == -1).all() and np.array_equal(sp["out_faces"], f.astype(np.int32))


# ---- determinism and purity ---------------------------------------------------------------------------------------------------------------------
def test_both_calls_are_pure_and_deterministic():
    V1, f1, _ = ref.cones((257, 5, 2049), seed=2)
    V2, f2 = ref.book(300)
    V3, f3 = ref.hub(600)
    v4, f4 = _simplified(2.0)
    f = np.concatenate([f1, f2 + V1, f3 + V1 + V2, f4 + V1 + V2 + V3, [[0, 0, 1], [-1, 5, 6]]])
    V = V1 + V2 + V3 + len(v4)
    keep = np.ones(len(f), np.uint8)
    keep[5::97] = 0
    want = ref.fans(V, f, keep)
    capacity = want["new_vertices"] + 7

    def call(pattern):  # every workspace and every output comes from torch.empty and is poisoned, with guard bytes either side
        corner_fan, vertex_fans, counts = _gpu_fans(V, f, keep)
        out_faces, source, label, totals = _gpu_split(V, f, corner_fan, keep, capacity)  # in a fresh, poisoned workspace of its own
        return {"corner_fan": corner_fan, "vertex_fans": vertex_fans, "counts": counts, "out_faces": out_faces, "new_vertex_source": source,
                "new_vertex_fan": label, "totals": totals}

    base = poison.assert_pure(call)  # twice on zeros first: the same call repeated gives identical bytes
    expect = ref.split(V, f, want["corner_fan"], keep, capacity)
    assert base["corner_fan"].numpy().tobytes() == want["corner_fan"].tobytes()
    assert base["out_faces"].numpy().tobytes() == expect["out_faces"].tobytes()
    assert base["new_vertex_fan"].numpy().tobytes() == expect["new_vertex_fan"].tobytes()
    assert want["new_vertices"] > 1000 and want["counts"][4] >= 2  # the copies of the book and the hub; the book's spine, the pinched cells


# ---- the public wrappers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell,new,boundary", [(2.0, 63, 89), (4.0, 35, 52)])
def test_simplified_spheres_become_manifold_and_fill_to_lone_flaps(cell, new, boundary):
    from diff_recon_hip import boundary_loops, fill_holes, mesh_topology, simplify_mesh, split_nonmanifold, vertex_fans
    from diff_recon_hip.mesh_holes import LOOP_STATUS
    v, f = fixtures.sphere_mesh()
    colour = np.random.default_rng(4).uniform(0, 1, (len(v), 3)).astype(np.float32)
    valid = np.random.default_rng(5).integers(0, 4, len(v)) != 0
    origin = tuple((v.min(0) - 0.01).tolist())
    s = simplify_mesh(_dev(v), _faces(f), cell, origin=origin, vertex_attributes=_dev(colour), attribute_valid=_dev(valid))
    V = s.vertices.shape[0]
    before = mesh_topology(V, s.faces)
    out = split_nonmanifold(s.vertices, s.faces, vertex_attributes=s.vertex_attributes, attribute_valid=s.attribute_valid)
    after = mesh_topology(out.vertices.shape[0], out.faces)
    assert before["nonmanifold"] == out.stats["nonmanifold_edges"] > 0 and before["boundary"] == 0
    assert (after["nonmanifold"], after["boundary"], out.stats["new_vertices"]) == (0, boundary, new)
    # the old vertices first, bit for bit; the copies are gathers through source_vertex, attributes and valid bytes too
    assert torch.equal(out.vertices[:V].view(torch.int32), s.vertices.view(torch.int32)) and out.vertices.shape[0] == V + new
    src = out.source_vertex.to(torch.int64)
    assert out.source_vertex.dtype == torch.int32 and torch.equal(out.source_vertex[:V], torch.arange(V, device=DEV, dtype=torch.int32))
    assert torch.equal(out.vertices.view(torch.int32), s.vertices[src].view(torch.int32))
    assert torch.equal(out.vertex_attributes.view(torch.int32), s.vertex_attributes[src].view(torch.int32))
    assert torch.equal(out.attribute_valid, s.attribute_valid[src]) and out.attribute_valid.dtype == torch.bool
    assert out.new_vertex.dtype == torch.bool and not out.new_vertex[:V].any() and out.new_vertex[V:].all()
    assert out.stats["split_vertices"] == int((out.fans.vertex_fans >= 2).sum()) and out.stats["corners_rewritten"] >= new
    want_v, want_f, _, _ = ref.split_mesh(s.vertices.cpu().numpy(), s.faces.cpu().numpy())
    _same(out.faces, want_f, "split_nonmanifold faces")
    _same(out.vertices, want_v, "split_nonmanifold vertices")
    # a second pass adds nothing; with the fans at hand the result is the same
    again = split_nonmanifold(out.vertices, out.faces)
    assert again.stats["new_vertices"] == 0 and again.stats["split_vertices"] == 0 and torch.equal(again.faces, out.faces)
    handed = split_nonmanifold(s.vertices, s.faces, fans=vertex_fans(V, s.faces))
    assert torch.equal(handed.faces, out.faces) and handed.vertex_attributes is None
    # nothing is open at a pinch any more, and the fill leaves only the lone flap faces
    loops = boundary_loops(out.vertices.shape[0], out.faces)
    assert loops.stats["nonsimple_vertices"] == 0 and loops.stats["open_half_edges"] == 0 and loops.stats["boundary_half_edges"] == boundary
    filled = fill_holes(out.vertices, out.faces, loops=loops)
    lone = filled.stats["lone_face"]
    assert filled.stats["loops"] == filled.stats["filled"] + lone and lone > 0 and filled.stats["too_long"] == filled.stats["dead"] == 0
    assert set(filled.loop_status.tolist()) == {LOOP_STATUS["filled"], LOOP_STATUS["lone_face"]}
    closed = mesh_topology(filled.vertices.shape[0], filled.faces)
    assert (closed["boundary"], closed["nonmanifold"]) == (3 * lone, 0)
    if cell == 2.0:
        assert (filled.stats["loops"], lone) == (27, 18)


def test_pinched_sphere_closes_only_after_the_split():
    from diff_recon_hip import fill_holes, mesh_topology, split_nonmanifold
    v, f = _pinched_sphere()
    vd, fd = _dev(v), _faces(f)
    alone = fill_holes(vd, fd)
    assert alone.stats["filled_loops"] == 0 and alone.stats["loops"] == 0 and alone.stats["open_half_edges"] == 6 and alone.faces.shape[0] == len(f)
    out = split_nonmanifold(vd, fd)
    assert out.stats["new_vertices"] == 1 and out.stats["split_vertices"] == 1 and out.stats["nonmanifold_edges"] == 0
    filled = fill_holes(out.vertices, out.faces)
    assert filled.stats["loops"] == 1 and filled.stats["longest_loop"] == 6 and filled.stats["filled_loops"] == 1  # ONE loop over both copies
    t = mesh_topology(filled.vertices.shape[0], filled.faces)
    assert (t["boundary"], t["nonmanifold"], t["euler"], filled.vertices.shape[0], filled.faces.shape[0]) == (0, 0, 2, 4836, 9668)


def _cams():
    return [SimpleNamespace(world_view_transform=_dev(np.asarray(ref_volume.look_at_view(eye), np.float32)), tan_fovx=0.45, tan_fovy=0.45,
                            image_width=48, image_height=48, device="cuda:0") for eye in ref_volume.AXIS_EYES]


def test_manifold_fused_splits_the_simplified_fusion_of_both_kinds():
    """The six axis views of the fusion's end-to-end test, fused, simplified in cells of 2 and 4 voxels on the device, then split."""
    from diff_recon_hip import MeshRenderer, manifold_fused, mesh_topology, simplify_fused
    from diff_recon_hip.color_volume import ColorTSDFVolume
    from diff_recon_hip.volume import TSDFVolume, fusion_bounds
    v, f = _latlong_sphere()
    vd, fd = _dev(v), _dev(f)
    colour = _dev(np.full((len(f), 3), 0.25, np.float32))
    plain, coloured = TSDFVolume(*fusion_bounds(vd, 24), DEV), ColorTSDFVolume(*fusion_bounds(vd, 24), DEV)
    for cam in _cams():
        out = MeshRenderer(cam).render(vertices=vd, faces=fd, faces_color=colour)
        plain.integrate(cam, out["depth"])
        coloured.integrate(cam, out["depth"], image=out["render"])
    split_somewhere = {"WeldedMesh": 0, "ColoredMesh": 0}
    for volume, cell in ((plain, 2.0), (plain, 4.0), (coloured, 2.0), (coloured, 4.0)):
        mesh = simplify_fused(volume.extract(), volume, cell)
        V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
        before = mesh_topology(V, mesh.faces)
        want_v, want_f, fn, sp = ref.split_mesh(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy())
        out = manifold_fused(mesh)
        assert type(out) is type(mesh)
        after = mesh_topology(out.vertices.shape[0], out.faces)
        s = out.stats["manifold"]
        split_somewhere[type(mesh).__name__] += s["new_vertices"]
        print(f"{type(mesh).__name__}, cells of {cell:g} voxels: {V} vertices, {F} faces, {s['fans']} fans, {s['split_vertices']} split, {s['new_vertices']} new; non-manifold "
              f"{before['nonmanifold']} -> {after['nonmanifold']}, boundary {before['boundary']} -> {after['boundary']}")
        assert [s[k] for k in ref.COUNT_NAMES] == fn["counts"] and s["new_vertices"] == fn["new_vertices"] and s["corners_rewritten"] == sp["totals"][1]
        assert after["nonmanifold"] == 0 and before["nonmanifold"] == s["nonmanifold_edges"]
        _same(out.faces, want_f, "manifold_fused faces")
        _same(out.vertices, want_v, "manifold_fused vertices")
        assert out.stats["num_vertices"] == out.vertices.shape[0] == V + s["new_vertices"] and out.stats["num_faces"] == out.faces.shape[0] == F
        assert {k: x for k, x in out.stats.items() if k not in ("manifold", "num_vertices", "num_faces")} == \
               {k: x for k, x in mesh.stats.items() if k not in ("num_vertices", "num_faces")}
        src = _dev(np.concatenate([np.arange(V), sp["new_vertex_source"]]).astype(np.int64))
        if hasattr(mesh, "vertex_color"):
            assert torch.equal(out.vertex_color.view(torch.int32), mesh.vertex_color[src].view(torch.int32))  # a copy has its source's colour ...
            assert torch.equal(out.color_valid, mesh.color_valid[src]) and out.color_valid.dtype == torch.bool  # ... and its valid byte
        else:
            assert out.face_keep is mesh.face_keep and out.faces_color is None and out.vertex_map.shape == mesh.vertex_map.shape
            kept = mesh.vertex_map >= 0  # every soup vertex still lands on a vertex with its position
            at, was = out.vertex_map[kept].to(torch.int64), mesh.vertex_map[kept].to(torch.int64)
            assert torch.equal(out.vertices[at].view(torch.int32), mesh.vertices[was].view(torch.int32)) and torch.equal(out.vertex_map[~kept], mesh.vertex_map[~kept])
    assert min(split_somewhere.values()) > 0, split_somewhere  # the coarse cells pinch: both kinds had copies whose attributes were compared


def test_example_reports_the_split_mesh():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    res = train_synthetic.mesh_scores(m, "2D", extract=24, simplify=3.0, fill=16, split=True, **cfg)
    fused = res["fused"]
    lines = train_synthetic.manifold_report(fused)
    print("\n".join(lines + train_synthetic.filled_report(fused)))
    s, before, after = fused["manifold"], fused["manifold"]["before"], fused["manifold"]["topology"]
    assert len(lines) == 1 and lines[0].startswith(f"manifold mesh: {s['fans']} fans, {s['split_vertices']} vertices split, {s['new_vertices']} new vertices; ")
    assert f"{before['nonmanifold']} -> {after['nonmanifold']} non-manifold edges" in lines[0] and f"{s['same_direction_edges']} same-direction edges" in lines[0]
    assert before == fused["simplified"]["topology"] and after["nonmanifold"] == 0 and before["nonmanifold"] == s["nonmanifold_edges"]
    assert after["faces"] == before["faces"] and fused["filled"]["before"] == after  # the fill follows the split, on the simplified mesh
    assert f"{after['boundary']} -> {fused['filled']['topology']['boundary']} boundary edges" in train_synthetic.filled_report(fused)[0]
    plain = train_synthetic.mesh_scores(m, "2D", extract=24, simplify=3.0, **cfg)["fused"]  # without the flag: what the split mesh was made from
    assert "manifold" not in plain and "filled" not in plain and plain["topology"] == fused["topology"] and plain["to_soup"] == fused["to_soup"]
    assert plain["simplified"]["topology"] == before and train_synthetic.simplified_report(plain["simplified"]) == train_synthetic.simplified_report(fused["simplified"])
    unsimplified = train_synthetic.mesh_scores(m, "2D", extract=24, fill=16, split=True, **cfg)["fused"]
    assert unsimplified["manifold"]["before"] == unsimplified["topology"] and unsimplified["filled"]["before"] == unsimplified["manifold"]["topology"]
