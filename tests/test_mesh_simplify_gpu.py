"""GPU tests of mesh simplification against tests/ref_mesh_simplify.py: labels, numbering, positions, attributes, faces, keep masks and both
counts bit for bit; the key's top bits; the serial one-cell case; the no-ops; purity; simplify_mesh on the device's own level set;
fuse_colored_mesh + simplify_fused(simplify_cell=...) end to end; drop_small_pieces; the example's report."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import poison
import ref_mesh_simplify as ref
import ref_mesh_weld
import ref_volume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SOUP_ORIGIN, SOUP_CELL = (-0.25, 0.5, 0.125), 0.73


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _gpu(v, f, origin, cell, mode="quadric", lam=1e-3, attrs=None, mask=None):
    """The five steps, one call each, everything with its full V / F rows."""
    from diff_recon_hip import cluster_labels, place_clusters, unique_faces
    from diff_recon_hip.mesh_weld import compact_labels, remap_faces
    vd, fd = _dev(np.asarray(v, np.float32)), _dev(np.asarray(f, np.int32).reshape(-1, 3))
    label = cluster_labels(vd, origin, cell)
    remap, _, n = compact_labels(label, vd, "first")
    placed, out_attrs, out_valid, members = place_clusters(vd, fd, remap, origin, cell, mode, lam, None if attrs is None else _dev(attrs),
                                                           None if mask is None else _dev(mask))
    new, keep_remap = remap_faces(len(v), fd, remap)
    keep, counts = unique_faces(n, new, keep_remap)
    return {"label": label, "remap": remap, "num_vertices": n, "vertices": placed, "attributes": out_attrs, "valid": out_valid,
            "member_count": members, "new_faces": new, "keep_remap": keep_remap, "keep": keep, "counts": counts}


def _assert_equals_reference(got, want, V):
    n = want["num_vertices"]
    assert got["num_vertices"] == n
    assert np.array_equal(got["label"].cpu().numpy(), want["label"]) and got["label"].dtype == torch.int32
    assert np.array_equal(got["remap"].cpu().numpy(), want["remap"])
    vert = got["vertices"].cpu().numpy()
    assert vert.shape == (V, 3)
    diff = np.nonzero((_bits(vert[:n]) != _bits(want["vertices"])).any(1))[0]
    assert len(diff) == 0, (len(diff), diff[:5], vert[diff[:5]], want["vertices"][diff[:5]])
    assert not _bits(vert[n:]).any()  # rows V' .. V - 1 are zero
    members = got["member_count"].cpu().numpy()
    assert np.array_equal(members[:n], want["member_count"]) and not members[n:].any()
    if want["attributes"] is not None:
        a, ok = got["attributes"].cpu().numpy(), got["valid"].cpu().numpy()
        assert np.array_equal(_bits(a[:n]), _bits(want["attributes"])) and not _bits(a[n:]).any()
        assert np.array_equal(ok[:n], want["valid"] != 0) and not ok[n:].any()
    assert np.array_equal(got["new_faces"].cpu().numpy(), want["new_faces"])
    assert np.array_equal(got["keep_remap"].cpu().numpy(), want["keep_remap"])
    assert np.array_equal(got["keep"].cpu().numpy(), want["keep"]) and got["keep"].dtype == torch.bool
    assert got["counts"].tolist() == [want["duplicates"], want["flaps"]]


# ---- the sphere -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sphere():
    v, f = ref.sphere_mesh()
    rng = np.random.default_rng(17)
    return v, f, rng.uniform(-1, 2, (len(v), 3)).astype(np.float32), (rng.integers(0, 3, len(v)) != 0).astype(np.uint8)


@pytest.mark.parametrize("mode", ["quadric", "mean"])
@pytest.mark.parametrize("cell", [1.7, 3.0])
def test_sphere_matches_the_reference_bit_for_bit(cell, mode):
    v, f, attrs, mask = _sphere()
    origin = (-0.3, -0.3, -0.3)
    want = ref.simplify(v, f, cell, origin, mode, 1e-3, attrs, mask)
    assert (want["num_vertices"], len(want["faces"])) == {1.7: (493, 993), 3.0: (184, 366)}[cell]
    assert 0 < int(want["valid"].sum())  # a random third of the vertices has no attribute
    _assert_equals_reference(_gpu(v, f, origin, cell, mode, 1e-3, attrs, mask), want, len(v))


# ---- random soups -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _soup(V, clean=False):
    """V vertices over about 6^3 cells of the grid (SOUP_ORIGIN, SOUP_CELL) and F = 2 V faces.  One cell holds min(1500, V // 2) members;
    unless `clean`, some vertices are NaN, +-inf, in cell -1 and in cell 2^21, some face indices are -1 and V, some faces repeat an index,
    some take two or three vertices from the crowded cell, and some are exact copies of earlier faces: in the same rotation, in another
    rotation of the same orientation, and reversed."""
    rng = np.random.default_rng(1000 + V)
    o, c = np.array(SOUP_ORIGIN), SOUP_CELL
    v = (o + c * rng.uniform(0.0, 6.0, (V, 3))).astype(np.float32)
    crowd = rng.permutation(V)[:min(1500, V // 2)]
    v[crowd] = (o + c * (np.array([2.0, 3.0, 1.0]) + rng.uniform(0.02, 0.98, (len(crowd), 3)))).astype(np.float32)
    F = 2 * V
    f = rng.integers(0, V, (F, 3)).astype(np.int64)
    if len(crowd) >= 3:
        k = F // 8
        f[:k, 0], f[:k, 1] = rng.choice(crowd, k), rng.choice(crowd, k)  # two vertices in one cluster
        f[:k // 2, 2] = rng.choice(crowd, k // 2)                         # three
    if not clean and V >= 63:
        special = rng.permutation(V)[:10]
        for i, bad in zip(special, (np.nan, np.inf, -np.inf, o[0] - 0.5 * c, o[0] + c * (2.0 ** 21 + 0.5))):
            v[i, 0] = bad
        for i, bad in zip(special[5:], (np.nan, -np.inf, o[1] - 1e-3, o[2] + c * 2.0 ** 21 * 1.001, np.inf)):
            v[i, 1 + (i % 2)] = bad
        rows = rng.permutation(F)[:F // 16]
        f[rows[0::4], 0] = -1
        f[rows[1::4], 2] = V
        f[rows[2::4], 1] = f[rows[2::4], 0]
        f[rows[3::4]] = f[rows[3::4], :1]
        m = F // 10
        src = rng.integers(0, F // 2, 3 * m)
        dst = F - 3 * m + np.arange(3 * m)
        f[dst[:m]] = f[src[:m]]                        # the same rotation
        f[dst[m:2 * m]] = f[src[m:2 * m]][:, [1, 2, 0]]  # another rotation, same orientation
        f[dst[2 * m:]] = f[src[2 * m:]][:, [0, 2, 1]]    # reversed
    attrs = rng.uniform(-2, 2, (V, 3)).astype(np.float32)
    if V >= 63:
        attrs[rng.integers(0, V)] = np.nan
    mask = (rng.integers(0, 4, V) != 0).astype(np.uint8)
    return v, f, attrs, mask


@pytest.mark.parametrize("V", [1, 63, 1025, 4097, 12289])
def test_random_soups_match_the_reference_bit_for_bit(V):
    v, f, attrs, mask = _soup(V)
    want = ref.simplify(v, f, SOUP_CELL, SOUP_ORIGIN, "quadric", 1e-3, attrs, mask)
    if V >= 63:
        assert want["member_count"].max() >= min(1500, V // 2) - 10 and want["duplicates"] > 0 and want["flaps"] > 0
        assert (want["label"] == np.arange(V)).sum() >= 10 and np.isnan(want["vertices"]).any()  # the invalid vertices are their own clusters
    _assert_equals_reference(_gpu(v, f, SOUP_ORIGIN, SOUP_CELL, "quadric", 1e-3, attrs, mask), want, V)
    want = ref.simplify(v, f, SOUP_CELL, SOUP_ORIGIN, "mean", 0.0, attrs[:, :1], None)
    _assert_equals_reference(_gpu(v, f, SOUP_ORIGIN, SOUP_CELL, "mean", 0.0, attrs[:, :1], None), want, V)


def test_eight_channels_and_no_regularisation():
    v, f, _, mask = _soup(1025)
    attrs = np.random.default_rng(5).uniform(-1, 1, (1025, 8)).astype(np.float32)
    want = ref.simplify(v, f, SOUP_CELL, SOUP_ORIGIN, "quadric", 0.0, attrs, mask)  # lambda 0: singular quadrics fall back to the mean
    _assert_equals_reference(_gpu(v, f, SOUP_ORIGIN, SOUP_CELL, "quadric", 0.0, attrs, mask), want, 1025)


def test_the_top_bits_of_the_key_keep_cells_apart():
    top = 2 ** 21 - 1
    cells = [(top, 5, 5), (top - 2 ** 20, 5, 5), (5, top, 5), (5, top - 2 ** 20, 5), (5, 0x7FF, 5), (5, 0xFFF, 5), (5, 0x800, 5), (5, 0x1000, 5),
             (5, 5, top), (5, 5, top - 2 ** 20), (5, 5, 1), (5, 5, 2 ** 10 + 1), (top, top, top), (top, top, top - 1), (0, 0, 0), (0, 0, 2 ** 20)]
    pts = [(np.array(c, np.float64) + off) for c in cells for off in (0.25, 0.5, 0.75)]
    pts += [np.array(p) for p in ((2.0 ** 21 + 0.5, 5.5, 5.5), (5.5, 2.0 ** 21 + 0.5, 5.5), (5.5, 5.5, 2.0 ** 21 + 0.5))]  # the neighbours at 2^21: invalid
    order = np.random.default_rng(2).permutation(len(pts))
    v = np.array(pts, np.float32)[order]
    assert np.array_equal(v.astype(np.float64), np.array(pts)[order])  # every coordinate is an fp32 number
    f = np.random.default_rng(3).integers(0, len(v), (40, 3))
    want = ref.simplify(v, f, 1.0, (0.0, 0.0, 0.0))
    assert want["num_vertices"] == len(cells) + 3 and sorted(want["member_count"].tolist()) == [1] * 3 + [3] * len(cells)
    _assert_equals_reference(_gpu(v, f, (0.0, 0.0, 0.0), 1.0), want, len(v))


def test_one_cell_over_the_whole_mesh_finishes():
    v, f, attrs, mask = _soup(12289, clean=True)
    want = ref.simplify(v, f, 1.0e4, (-5.0e3, -5.0e3, -5.0e3), "quadric", 1e-3, attrs, mask)
    assert want["num_vertices"] == 1 and len(want["faces"]) == 0 and want["member_count"].tolist() == [12289]
    _assert_equals_reference(_gpu(v, f, (-5.0e3, -5.0e3, -5.0e3), 1.0e4, "quadric", 1e-3, attrs, mask), want, 12289)


def test_no_vertices_and_no_faces_are_no_ops():
    from diff_recon_hip import simplify_mesh, unique_faces
    v0, f0 = torch.zeros((0, 3), device=DEV), torch.zeros((0, 3), device=DEV, dtype=torch.int32)
    s = simplify_mesh(v0, f0, 1.0)
    assert s.vertices.shape == (0, 3) and s.faces.shape == (0, 3) and s.stats["num_vertices"] == 0 and s.stats["duplicates"] == 0
    keep, counts = unique_faces(5, f0, torch.zeros((0,), device=DEV, dtype=torch.bool))
    assert keep.shape == (0,) and counts.tolist() == [0, 0]
    v, _, attrs, mask = _soup(63)
    want = ref.simplify(v, np.zeros((0, 3), np.int64), SOUP_CELL, SOUP_ORIGIN, "quadric", 1e-3, attrs, mask)  # vertices without faces: the mean
    _assert_equals_reference(_gpu(v, np.zeros((0, 3), np.int64), SOUP_ORIGIN, SOUP_CELL, "quadric", 1e-3, attrs, mask), want, 63)


# ---- purity -----------------------------------------------------------------------------------------------------------------------------------
def test_all_three_calls_are_pure():
    v, f, attrs, mask = _soup(1025)

    def call(pattern):  # every workspace and every output comes from torch.empty and is poisoned
        got = _gpu(v, f, SOUP_ORIGIN, SOUP_CELL, "quadric", 1e-3, attrs, mask)
        return {k: (x if isinstance(x, torch.Tensor) else torch.tensor(x)) for k, x in got.items()}

    base = poison.assert_pure(call)
    want = ref.simplify(v, f, SOUP_CELL, SOUP_ORIGIN, "quadric", 1e-3, attrs, mask)
    n = want["num_vertices"]
    vert = base["vertices"].numpy().view(np.float32).reshape(-1, 3)
    assert np.array_equal(_bits(vert[:n]), _bits(want["vertices"])) and not _bits(vert[n:]).any() and n < 1025


# ---- the public wrappers ------------------------------------------------------------------------------------------------------------------------
def test_simplify_mesh_on_the_devices_own_level_set_equals_the_numpy_pipeline():
    from diff_recon_hip import extract_isosurface, mesh_topology, simplify_mesh, weld_mesh
    field = _dev(ref_volume.sphere_field((28, 28, 28), (13.63, 13.29, 13.57), 9.3).reshape(28, 28, 28))
    soup_v, soup_f = extract_isosurface(field, (0.0, 0.0, 0.0), 1.0)
    welded = weld_mesh(soup_v, soup_f, eps=0.0)
    assert welded.stats["num_vertices"] == 4834 and welded.stats["num_faces"] == 9664
    v, f = welded.vertices.cpu().numpy(), welded.faces.cpu().numpy()
    colour = _dev(np.random.default_rng(9).uniform(0, 1, (len(f), 3)).astype(np.float32))
    for cell, sizes in ((1.7, (493, 993)), (2.0, (375, 746))):
        s = simplify_mesh(welded.vertices, welded.faces, cell, origin=(-0.3, -0.3, -0.3), faces_color=colour)
        want = ref.simplify(v, f, cell, (-0.3, -0.3, -0.3))
        assert (s.stats["num_vertices"], s.stats["num_faces"]) == sizes == (want["num_vertices"], len(want["faces"]))
        assert np.array_equal(_bits(s.vertices.cpu().numpy()), _bits(want["vertices"])) and np.array_equal(s.faces.cpu().numpy(), want["faces"])
        assert np.array_equal(s.vertex_map.cpu().numpy(), want["remap"]) and np.array_equal(s.face_keep.cpu().numpy(), want["keep"])
        assert torch.equal(s.faces_color, colour[s.face_keep]) and s.vertex_attributes is None and s.attribute_valid is None
        st = s.stats
        assert st["duplicates"] == want["duplicates"] == (5 if cell == 1.7 else 0) and st["flaps"] == want["flaps"]
        assert st["collapsed"] == len(f) - int(want["keep_remap"].sum()) and st["largest_cluster"] == int(want["member_count"].max())
        assert st["num_vertices_in"] == 4834 and st["num_faces_in"] == 9664 and 0 < st["max_displacement"] <= np.sqrt(3.0) * cell
        assert mesh_topology(st["num_vertices"], s.faces)["boundary"] == 0  # still closed
    s = simplify_mesh(welded.vertices, welded.faces, 2.0, placement="mean")  # origin=None: the per-axis minimum of the finite vertices
    want = ref.simplify(v, f, 2.0, tuple(v.min(0).tolist()), "mean")
    assert np.array_equal(_bits(s.vertices.cpu().numpy()), _bits(want["vertices"])) and np.array_equal(s.faces.cpu().numpy(), want["faces"])


def _latlong_sphere(radius=0.6, rings=14, segments=20):
    th = np.linspace(0, np.pi, rings + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, segments, endpoint=False)
    pts = [[0.0, 0.0, radius]] + [[radius * np.sin(t) * np.cos(p), radius * np.sin(t) * np.sin(p), radius * np.cos(t)] for t in th for p in ph]
    pts.append([0.0, 0.0, -radius])
    ring = lambda r, s: 1 + r * segments + s % segments
    faces = [(0, ring(0, s), ring(0, s + 1)) for s in range(segments)]
    for r in range(rings - 2):
        for s in range(segments):
            faces += [(ring(r, s), ring(r + 1, s), ring(r + 1, s + 1)), (ring(r, s), ring(r + 1, s + 1), ring(r, s + 1))]
    last = len(pts) - 1
    faces += [(last, ring(rings - 2, s + 1), ring(rings - 2, s)) for s in range(segments)]
    return np.array(pts, np.float32), np.array(faces, np.int32)


def test_fuse_colored_mesh_with_simplify_cell_end_to_end():
    from diff_recon_hip import fuse_colored_mesh, fuse_mesh, mesh_topology, simplify_fused
    v, f = _latlong_sphere()
    centre = v[f].astype(np.float64).mean(axis=1)
    colour = (0.5 + 0.4 * centre / np.linalg.norm(centre, axis=1, keepdims=True)).astype(np.float32)
    cams = [SimpleNamespace(world_view_transform=_dev(np.asarray(ref_volume.look_at_view(eye), np.float32)), tan_fovx=0.45, tan_fovy=0.45,
                            image_width=48, image_height=48, device="cuda:0") for eye in ref_volume.AXIS_EYES]
    vd, fd, cd = _dev(v), _dev(f), _dev(colour)
    plain, vol = fuse_colored_mesh(cams, vd, fd, cd, 20, return_volume=True)
    assert simplify_fused(plain, vol) is plain  # the defaults change nothing
    again = fuse_mesh(cams, vd, fd, 20, simplify_cell=None, min_piece_faces=0)
    assert torch.equal(again.vertices, plain.vertices) and torch.equal(again.faces, plain.faces) and again.stats == plain.stats
    mesh = simplify_fused(plain, vol, simplify_cell=2)
    assert type(mesh) is type(plain)
    want = ref.simplify(plain.vertices.cpu().numpy(), plain.faces.cpu().numpy(), 2.0 * vol.voxel_size, vol.origin, "quadric", 1e-3,
                        plain.vertex_color.cpu().numpy(), plain.color_valid.cpu().numpy().astype(np.uint8))
    assert 0 < want["num_vertices"] < plain.vertices.shape[0] // 3
    assert np.array_equal(_bits(mesh.vertices.cpu().numpy()), _bits(want["vertices"])) and np.array_equal(mesh.faces.cpu().numpy(), want["faces"])
    assert want["valid"].all() and mesh.color_valid.all()
    assert np.array_equal(_bits(mesh.vertex_color.cpu().numpy()), _bits(want["attributes"]))
    assert mesh.stats["num_vertices"] == want["num_vertices"] and mesh.stats["simplify"]["duplicates"] == want["duplicates"]
    topo = mesh_topology(mesh.stats["num_vertices"], mesh.faces)
    assert topo["boundary"] == 0 and topo["pieces"] == 1
    geometry = fuse_mesh(cams, vd, fd, 20, simplify_cell=2, min_piece_faces=4)  # one piece: the filter keeps everything
    assert torch.equal(geometry.vertices, mesh.vertices) and torch.equal(geometry.faces, mesh.faces) and geometry.stats["small_piece_faces"] == 0
    assert geometry.vertex_map.shape == (plain.vertices.shape[0],) and geometry.face_keep.shape == (plain.faces.shape[0],)
    assert int(geometry.face_keep.sum()) == geometry.faces.shape[0] and int(geometry.vertex_map.max()) == mesh.vertices.shape[0] - 1


def test_drop_small_pieces_against_the_reference_topology():
    from diff_recon_hip import drop_small_pieces
    v, f = _latlong_sphere()
    rng = np.random.default_rng(4)
    tet_v = np.array([[2, 0, 0], [3, 0, 0], [2, 1, 0], [2, 0, 1]], np.float32)
    tet_f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    strays = rng.uniform(4, 5, (9, 3)).astype(np.float32)  # three lone triangles
    unused = np.array([[9, 9, 9]], np.float32)
    verts = np.concatenate([tet_v, v, strays, unused])
    faces = np.concatenate([tet_f, f + 4, np.arange(9).reshape(3, 3) + 4 + len(v), [[0, 1, len(verts)], [-1, 2, 3]]])
    order = rng.permutation(len(faces))
    faces = faces[order]
    topo = ref_mesh_weld.topology(len(verts), faces)
    assert topo["pieces"] == 5
    valid = ((faces >= 0) & (faces < len(verts))).all(1)
    piece = topo["label"][np.clip(faces[:, 0], 0, len(verts) - 1)]
    size = np.bincount(piece[valid], minlength=len(verts))
    for min_faces, pieces in ((0, 5), (2, 2), (5, 1), (10 ** 6, 0)):
        want_keep = valid & (size[piece] >= min_faces)
        used = np.zeros(len(verts), bool)
        used[faces[want_keep].reshape(-1)] = True
        new_index = np.cumsum(used) - 1
        out_v, out_f, keep = drop_small_pieces(_dev(verts), _dev(faces.astype(np.int32)), min_faces)
        assert np.array_equal(keep.cpu().numpy(), want_keep) and keep.dtype == torch.bool
        assert np.array_equal(_bits(out_v.cpu().numpy()), _bits(verts[used])) and np.array_equal(out_f.cpu().numpy(), new_index[faces[want_keep]])
        got = ref_mesh_weld.topology(len(out_v), out_f.cpu().numpy())
        assert got["pieces"] == pieces and got["vertices_referenced"] == len(out_v)  # unreferenced vertices are compacted


def test_example_reports_the_simplified_mesh():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    res = train_synthetic.mesh_scores(m, "2D", extract=32, extract_color=True, simplify=2.0, min_piece=8, **cfg)
    simp = res["fused"]["simplified"]
    lines = train_synthetic.simplified_report(simp)
    print("\n".join(train_synthetic.fused_report(res["fused"]) + lines))
    assert len(lines) == 3 and lines[0].startswith("simplified mesh, cells of 2 voxels, pieces below 8 faces dropped: ")
    assert f"{simp['topology']['faces']} of {res['fused']['topology']['faces']} faces" in lines[0] and "duplicates removed" in lines[0]
    assert lines[1].startswith("simplified mesh against the soup: ") and lines[2].startswith("simplified mesh, colours averaged per cluster")
    assert 0 < simp["topology"]["faces"] < res["fused"]["topology"]["faces"] and simp["topology"]["pieces"] <= res["fused"]["topology"]["pieces"]
    assert np.isfinite(simp["color"]["mean_psnr"]) and simp["stats"]["simplify"]["num_faces_in"] == res["fused"]["topology"]["faces"]
    plain = train_synthetic.mesh_scores(m, "2D", extract=32, extract_color=True, **cfg)["fused"]
    assert "simplified" not in plain and plain["topology"] == res["fused"]["topology"] and plain["color"] == res["fused"]["color"]
