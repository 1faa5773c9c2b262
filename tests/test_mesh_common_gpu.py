"""GPU tests of the block-sum prefix sum the indexed-mesh units share (csrc/ts_mesh_scan.h) past 256 scan blocks, where a lane of the
one-workgroup offsets kernel owns more than one block (span > 1): more than 256 * 2048 = 524288 scanned elements.  The expected values are
closed forms of the inputs (the numpy references walk such sizes in Python loops), every comparison exact."""
import numpy as np
import pytest
import torch

import ref_mesh_manifold

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_TRI = 174764  # 3 * 174764 = 524292 corners: 257 scan blocks (span 2); 6 * 174764 = 1048584 directed records: 513 blocks (span 3)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _eq(got, want, what):
    got = got.cpu().numpy()
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
    assert len(diff) == 0, (what, len(diff), diff[:5], got.reshape(-1)[diff[:5]], want.reshape(-1)[diff[:5]])


def test_hub_of_174764_triangles_splits_past_256_scan_blocks():
    """mesh_manifold.hip's scan of the 3 F flags: the last flagged corner, 524289, lies in block 256, so its index depends on the
    second-level sums."""
    from diff_recon_hip import mesh_manifold
    n = N_TRI
    V, f = ref_mesh_manifold.hub(n)
    assert V == 2 * n + 1 and 3 * len(f) == 524292 and (3 * len(f) + 2047) // 2048 == 257
    faces = _dev(f.astype(np.int32))
    fans = mesh_manifold.vertex_fans(V, faces)
    want_fans = np.ones(V, np.int32)
    want_fans[0] = n
    _eq(fans.vertex_fans, want_fans, "vertex_fans")
    _eq(fans.corner_fan, np.arange(3 * n, dtype=np.int32), "corner_fan")  # no edge is shared: every corner is a fan of its own
    assert fans.stats["new_vertices"] == n - 1
    out_faces, source, label, totals = mesh_manifold._split_arrays(V, faces, None, fans.corner_fan, n - 1, faces.device)
    assert totals.tolist() == [n - 1, n - 1]
    _eq(source, np.zeros(n - 1, np.int32), "new_vertex_source")
    _eq(label, 3 * np.arange(1, n, dtype=np.int32), "new_vertex_fan")
    want_faces = f.astype(np.int32)
    want_faces[1:, 0] = V + np.arange(n - 1, dtype=np.int32)
    _eq(out_faces, want_faces, "out_faces")
    vertices = _dev(np.stack([np.arange(V) % 1024, np.arange(V) // 1024, np.zeros(V)], 1).astype(np.float32))
    mesh = mesh_manifold.split_nonmanifold(vertices, faces, fans=fans)
    _eq(mesh.faces, want_faces, "split_nonmanifold faces")
    _eq(mesh.source_vertex[V:], np.zeros(n - 1, np.int32), "source_vertex")
    assert mesh.vertices.shape == (V + n - 1, 3) and mesh.stats["corners_rewritten"] == n - 1


@pytest.fixture(scope="module")
def disjoint():
    """N_TRI disjoint triangles, face i = (3 i, 3 i + 1, 3 i + 2), at distinct, exactly representable positions."""
    V = 3 * N_TRI
    i = np.arange(V)
    return V, _dev(np.stack([i % 1024, i // 1024, np.zeros(V)], 1).astype(np.float32)), _dev(i.astype(np.int32).reshape(-1, 3))


def test_disjoint_triangles_weld_to_themselves_past_256_scan_blocks(disjoint):
    """mesh_weld.hip's root ranking over V = 524292 labels: 257 blocks."""
    from diff_recon_hip import weld_mesh
    V, vertices, faces = disjoint
    w = weld_mesh(vertices, faces, eps=0.0)
    assert w.stats["num_vertices"] == V and w.stats["num_faces"] == N_TRI and w.stats["largest_cluster"] == 1
    _eq(w.vertex_map, np.arange(V, dtype=np.int32), "vertex_map")
    assert torch.equal(w.vertices, vertices) and torch.equal(w.faces.to(torch.int32), faces) and bool(w.face_keep.all())


def test_disjoint_triangles_adjacency_and_loops_past_256_scan_blocks(disjoint):
    """mesh_smooth.hip's head ranking over 6 F = 1048584 records (513 blocks, span 3) and mesh_holes.hip's two-column scan over 3 F = 524292
    half-edges (257 blocks)."""
    from diff_recon_hip import mesh_holes, mesh_smooth
    V, _, faces = disjoint
    adj = mesh_smooth.vertex_adjacency(V, faces)
    assert adj.stats == {"entries": 2 * V, "boundary": 2 * V, "manifold": 0, "nonmanifold": 0}
    _eq(adj.offsets, 2 * np.arange(V + 1, dtype=np.int32), "offsets")
    v = np.arange(V, dtype=np.int32)
    base, k = v - v % 3, v % 3
    others = np.stack([base + np.where(k == 0, 1, 0), base + np.where(k == 2, 1, 2)], 1)  # the two other vertices of the face, ascending
    _eq(adj.neighbors, others.reshape(-1), "neighbors")
    _eq(adj.edge_faces, np.ones(2 * V, np.int32), "edge_faces")
    loops = mesh_holes.boundary_loops(V, faces, adjacency=adj)
    assert loops.stats["loops"] == N_TRI and loops.stats["loop_half_edges"] == V and loops.stats["boundary_half_edges"] == V
    _eq(loops.half_edge_loop, v // 3, "half_edge_loop")
    _eq(loops.loop_offsets, 3 * np.arange(N_TRI + 1, dtype=np.int32), "loop_offsets")
    _eq(loops.loop_half_edges, v, "loop_half_edges")  # every loop from its smallest half-edge along the boundary
