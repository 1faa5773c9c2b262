"""GPU tests of vertex welding and edge topology (diff_recon_hip.mesh_weld over include/ts_weld.h, csrc/mesh_weld.hip) against the numpy
reference tests/ref_mesh_weld.py.  Every comparison is exact -- integers, or floats bit for bit -- except the render of the welded mesh,
which is held to the criterion of tests/test_mesh_gpu.py against the float64 checker."""
import os
import sys

import numpy as np
import pytest
import torch

import ref_mesh_f64
import ref_mesh_weld as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = ref.GRID_EPS


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def gpu_labels(v, eps):
    from diff_recon_hip import mesh_weld
    out = mesh_weld.weld_labels(_t(np.asarray(v, np.float32)), eps)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def gpu_weld(v, f, eps, position="first", colors=None):
    from diff_recon_hip import weld_mesh
    w = weld_mesh(_t(np.asarray(v, np.float32)), _t(np.asarray(f, np.int64)), None if colors is None else _t(colors), eps=eps, position=position)
    torch.cuda.synchronize()
    return w


def check_weld(name, v, f, eps, position="first"):
    """The whole weld against the reference; returns (device result, reference)."""
    want = ref.weld(v, f, eps, position)
    got = gpu_weld(v, f, eps, position)
    V = len(v)
    remap = got.vertex_map.cpu().numpy().astype(np.int64)
    keep = got.face_keep.cpu().numpy()
    print(f"{name} ({position}): V {V} -> {got.stats['num_vertices']} (reference {want['num_vertices']}), faces kept {int(keep.sum())} of {len(keep)}, "
          f"largest cluster {got.stats['largest_cluster']}")
    assert got.stats["num_vertices"] == want["num_vertices"] and got.stats["num_vertices_in"] == V and got.stats["num_faces_in"] == len(keep)
    assert np.array_equal(remap, want["remap"]), name
    assert np.array_equal(keep, want["keep"]) and got.stats["num_faces"] == int(want["keep"].sum())
    assert np.array_equal(got.faces.cpu().numpy().astype(np.int64), want["faces"][want["keep"]])
    gv = got.vertices.cpu().numpy()
    assert gv.shape == want["vertices"].shape and gv.dtype == np.float32
    same = (_bits(gv) == _bits(want["vertices"])) | (np.isnan(gv) & np.isnan(want["vertices"]))
    assert same.all(), (name, position, int((~same).any(1).sum()))
    assert got.stats["largest_cluster"] == want["largest_cluster"]
    return got, want


def check_topology(name, V, faces, keep=None):
    from diff_recon_hip import mesh_topology
    want = ref.topology(V, faces, keep)
    got = mesh_topology(V, _t(np.asarray(faces, np.int64)), None if keep is None else _t(np.asarray(keep, bool)))
    print(f"{name}: {got}")
    for k in ("edges", "boundary", "manifold", "nonmanifold", "pieces", "vertices_referenced", "faces", "euler"):
        assert got[k] == want[k] and isinstance(got[k], int), (name, k, got[k], want[k])
    return got


# ---- 1. threshold -----------------------------------------------------------------------------------------------------------------------------
def test_threshold_is_inclusive_and_one_ulp_outside_is_not():
    eps = 0.25
    for axis in range(3):
        a, b = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32)
        a[0, axis], a[1, axis] = 1.0, 1.25  # exactly eps apart: d2 == eps * eps
        b[0, axis], b[1, axis] = 1.0, np.nextafter(np.float32(1.25), np.float32(2))
        assert np.float32(a[1, axis] - a[0, axis]) ** 2 == np.float32(eps) ** 2
        assert ref.labels(a, eps).tolist() == [0, 0] and ref.labels(b, eps).tolist() == [0, 1]
        assert gpu_labels(a, eps).tolist() == [0, 0], axis
        assert gpu_labels(b, eps).tolist() == [0, 1], axis
        assert gpu_labels(a[::-1], eps).tolist() == [0, 0] and gpu_labels(b[::-1], eps).tolist() == [0, 1]
    assert gpu_labels(np.array([[3.0, -2.0, 7.0]], np.float32), eps).tolist() == [0]  # V = 1
    got, _ = check_weld("one vertex", np.array([[3.0, -2.0, 7.0]], np.float32), np.zeros((0, 3), np.int64), eps)
    assert got.vertices.cpu().tolist() == [[3.0, -2.0, 7.0]] and got.faces.shape == (0, 3)
    from diff_recon_hip import weld_mesh
    empty = weld_mesh(torch.zeros((0, 3), device=DEV), torch.zeros((0, 3), device=DEV, dtype=torch.int32), eps=eps)
    assert empty.vertices.shape == (0, 3) and empty.stats["num_vertices"] == 0 and empty.stats["largest_cluster"] == 0


# ---- 2. a chain across boxes ---------------------------------------------------------------------------------------------------------------------
def test_chain_across_three_boxes_is_one_cluster():
    V, eps = 2500, 0.01  # three boxes of 1024 sorted points, the last partial
    direction = np.array([-0.6, 0.64, 0.48])  # unit length; x falls while y and z rise: the Morton order is not the order along the line
    line = (np.arange(V)[:, None] * (0.75 * eps)) * direction + np.array([9.0, -3.0, 0.5])
    perm = np.random.default_rng(7).permutation(V)
    v = line[perm].astype(np.float32)
    step = np.linalg.norm(np.diff(line.astype(np.float32).astype(np.float64), axis=0), axis=1)
    assert step.max() < 0.8 * eps and np.linalg.norm((line[2:] - line[:-2]).astype(np.float32), axis=1).min() > 1.4 * eps
    got = gpu_labels(v, eps)
    print(f"chain: {len(np.unique(got))} cluster(s)")
    assert not got.any()  # one cluster: every label is 0
    assert len(np.unique(gpu_labels(v, 0.7 * eps))) == V  # and below the step nothing merges
    cut = np.delete(line, 1250, axis=0)[np.random.default_rng(8).permutation(V - 1)].astype(np.float32)  # a gap of 1.5 eps: two clusters
    assert np.array_equal(gpu_labels(cut, eps), ref.labels(cut, eps)) and len(np.unique(gpu_labels(cut, eps))) == 2


# ---- 3. the jittered grid ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    v, f, grid_id = ref.posed_grid()
    return v, f, grid_id, ref.weld(v, f, EPS)


def test_jittered_grid_welds_into_the_grid(grid):
    v, f, grid_id, _ = grid
    assert v.shape == (2166, 3) and f.shape == (722, 3)
    got, want = check_weld("grid", v, f, EPS)
    assert got.stats["num_vertices"] == 400 and got.stats["num_faces"] == 722 and got.stats["largest_cluster"] == 6  # six triangles meet at an interior vertex
    assert ref.same_partition(got.vertex_map.cpu().numpy(), grid_id)  # every cluster is exactly one grid vertex
    assert 0.0 < got.stats["max_displacement"] < EPS
    t = check_topology("grid", 400, got.faces.cpu().numpy())
    assert (t["edges"], t["boundary"], t["manifold"], t["nonmanifold"], t["pieces"], t["euler"]) == (1121, 76, 1045, 0, 1, 1)
    soup = check_topology("soup", len(v), f)  # before the weld: 722 separate triangles
    assert (soup["edges"], soup["boundary"], soup["pieces"], soup["euler"]) == (2166, 2166, 722, 722)


def _planted(grid):
    """The grid plus: a sliver (two of its vertices fall into one cluster), a third face on an interior edge, a second grid far away, and four
    faces that name no vertex."""
    v, f, grid_id, _ = grid
    rng = np.random.default_rng(21)
    first = {g: int(np.nonzero(grid_id == g)[0][0]) for g in (0, 1, 210, 211)}

    def near(g):
        return v[first[g]] + ((rng.random(3) * 2 - 1) * EPS * 0.2).astype(np.float32)
    apex = v[first[210]] + np.array([0.0, 0.0, 40.0 * EPS], np.float32)  # its own cluster, off the surface
    extra_v = np.stack([near(0), near(0), near(1), near(210), near(211), apex])
    V0 = len(v)
    far, far_f, _ = ref.grid_soup(5, EPS, seed=4, origin=(5000.0, -3000.0, 800.0))
    v2 = np.concatenate([v, extra_v, far]).astype(np.float32)
    V = len(v2)
    faces = np.concatenate([f, [[V0, V0 + 1, V0 + 2], [V0 + 3, V0 + 4, V0 + 5]], far_f + V0 + 6, [[0, 1, V], [-1, 3, 4], [5, 2 ** 31 - 1, 6], [-2 ** 31, 7, 8]]])
    return v2, faces.astype(np.int64), V0


def test_planted_sliver_nonmanifold_edge_second_piece_and_bad_indices(grid):
    v, faces, V0 = _planted(grid)
    for position in ("first", "mean"):
        got, want = check_weld("planted", v, faces, EPS, position)
    keep = got.face_keep.cpu().numpy()
    assert not keep[722] and keep[723] and not keep[-4:].any() and keep[:722].all()  # the sliver and the four bad faces are dropped
    assert got.stats["num_vertices"] == 400 + 1 + 25 and got.stats["num_faces"] == 722 + 1 + 32
    t = check_topology("planted, welded", got.stats["num_vertices"], got.faces.cpu().numpy())
    assert t["nonmanifold"] == 1 and t["pieces"] == 2 and t["edges"] == 1121 + 2 + 56
    # the same through the keep mask on the un-compacted remapped faces, the bad rows (-1 -1 -1) included
    from diff_recon_hip import mesh_weld
    new, keep_t = mesh_weld.remap_faces(len(v), _t(faces), got.vertex_map)
    assert np.array_equal(new.cpu().numpy().astype(np.int64), want["faces"]) and np.array_equal(keep_t.cpu().numpy(), want["keep"])
    check_topology("planted, keep mask", got.stats["num_vertices"], want["faces"], want["keep"])
    check_topology("planted, no mask", got.stats["num_vertices"], want["faces"])  # the sliver's edges count when it is not masked out
    check_topology("planted, soup with bad indices", len(v), faces)
    check_topology("no vertices", 0, faces[:5])
    check_topology("no faces", 7, np.zeros((0, 3), np.int64))


# ---- 4. degenerate inputs -----------------------------------------------------------------------------------------------------------------------
def test_coincident_points_are_one_cluster():
    v = np.tile(np.array([[0.3, -1.7, 2.9]], np.float32), (1500, 1))  # more than one box
    f = np.arange(1500, dtype=np.int64).reshape(-1, 3)
    for eps in (0.0, 0.5):
        got, _ = check_weld(f"coincident, eps {eps}", v, f, eps, "mean")
        assert got.stats["num_vertices"] == 1 and got.stats["largest_cluster"] == 1500 and got.stats["num_faces"] == 0
        assert _bits(got.vertices.cpu().numpy()).tolist() == _bits(v[:1]).tolist()


def test_signed_zeros_are_equal_at_eps_zero():
    v = np.array([[0.0, 1.0, -0.0], [-0.0, 1.0, 0.0], [0.0, 1.0, 1e-6], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [2.0, 2.0, 2.0], [2.0, 2.0, 2.0]], np.float32)
    assert gpu_labels(v, 0.0).tolist() == [0, 0, 2, 3, 3, 5, 5]
    for position in ("first", "mean"):
        check_weld("signed zeros", v, [[0, 2, 3], [0, 1, 5]], 0.0, position)


def test_non_finite_vertices_are_singletons_and_disturb_nothing():
    rng = np.random.default_rng(5)
    base = rng.random((600, 3), dtype=np.float32)
    v = np.concatenate([base, base + np.float32(1e-4)])  # 600 pairs
    clean = ref.labels(v, 1e-3)
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, np.inf, np.inf], [-np.inf, 0.1, np.nan]], np.float32)
    where = np.array([0, 1, 2, 599, 600, 1199])
    planted = v.copy()
    planted[where] = bad  # each takes one member out of a pair; a copy of a finite neighbour's other coordinates stays within eps
    planted[where[:3], 1:] = np.where(np.isfinite(bad[:3, 1:]), v[where[:3], 1:], bad[:3, 1:])
    for eps in (1e-3, 3e38):  # 3e38 * 3e38 overflows to inf in fp32: every finite pair passes, no other
        got = gpu_labels(planted, eps)
        want = ref.labels(planted, eps)
        assert np.array_equal(got, want), eps
        assert (got[where] == where).all() and not np.isin(got, where)[np.setdiff1d(np.arange(len(v)), where)].any()
    rest = np.setdiff1d(np.arange(len(v)), np.concatenate([where, (where + 600) % 1200]))
    assert np.array_equal(gpu_labels(planted, 1e-3)[rest], clean[rest])  # the others are unaffected
    f = rng.integers(0, len(v), size=(300, 3))
    for position in ("first", "mean"):
        check_weld("non-finite", planted, f, 1e-3, position)
    allbad = np.full((1100, 3), np.nan, np.float32)  # nothing finite: an empty bounding box
    assert np.array_equal(gpu_labels(allbad, 1.0), np.arange(1100))


def test_eps_beyond_the_bounding_box_gives_one_cluster():
    v = np.random.default_rng(6).random((2100, 3), dtype=np.float32) * 4 - 2
    got = gpu_labels(v, 10.0)
    assert not got.any()
    v[[5, 1999]] = np.nan
    got = gpu_labels(v, 10.0)
    assert np.array_equal(got, ref.labels(v, 10.0)) and got[5] == 5 and got[1999] == 1999 and np.count_nonzero(got) == 2


# ---- 5. compaction ------------------------------------------------------------------------------------------------------------------------------
def test_compaction_numbers_by_ascending_label_and_places_both_position_modes(grid):
    v, f, grid_id, want = grid
    from diff_recon_hip import mesh_weld
    label = mesh_weld.weld_labels(_t(v), EPS)
    assert np.array_equal(label.cpu().numpy(), want["label"])
    remap, first, n = mesh_weld.compact_labels(label, _t(v), "first")
    assert n == 400 and np.array_equal(remap.cpu().numpy(), want["remap"])
    roots = np.unique(want["label"])
    assert np.array_equal(_bits(first.cpu().numpy()), _bits(v[roots]))  # the inputs' own bits
    remap2, mean, n2 = mesh_weld.compact_labels(label, _t(v), "mean")
    assert n2 == 400 and torch.equal(remap, remap2)
    assert np.array_equal(_bits(mean.cpu().numpy()), _bits(ref.compact(want["label"], v, "mean")[1]))
    assert not np.array_equal(_bits(mean.cpu().numpy()), _bits(first.cpu().numpy()))
    # labels need not come from the search: every vertex alone, and 3000 vertices (two scan tiles) in clusters of three
    alone = torch.arange(len(v), device=DEV, dtype=torch.int32)
    remap, out, n = mesh_weld.compact_labels(alone, _t(v), "mean")
    assert n == len(v) and torch.equal(remap, alone) and np.array_equal(_bits(out.cpu().numpy()), _bits(v))
    big = np.random.default_rng(9).standard_normal((3000, 3)).astype(np.float32)
    lab3 = (np.arange(3000) % 1000).astype(np.int32)
    for position in ("first", "mean"):
        remap, out, n = mesh_weld.compact_labels(_t(lab3), _t(big), position)
        wr, wo, wn = ref.compact(lab3.astype(np.int64), big, position)
        assert n == wn == 1000 and np.array_equal(remap.cpu().numpy(), wr) and np.array_equal(_bits(out.cpu().numpy()), _bits(wo)), position


# ---- 6. purity --------------------------------------------------------------------------------------------------------------------------------
def test_runs_repeat_bit_for_bit_and_vertex_order_only_permutes_the_partition(grid):
    v, faces, _ = _planted(grid)
    a = gpu_weld(v, faces, EPS, "mean")
    b = gpu_weld(v, faces, EPS, "mean")
    for x, y in ((a.vertices, b.vertices), (a.faces, b.faces), (a.vertex_map, b.vertex_map), (a.face_keep, b.face_keep)):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    assert a.stats == b.stats
    perm = np.random.default_rng(12).permutation(len(v))  # vertex k of the permuted mesh is vertex perm[k]
    inverse = np.argsort(perm)
    ok = ((faces >= 0) & (faces < len(v)))
    faces_p = np.where(ok, inverse[np.where(ok, faces, 0)], faces)
    c = gpu_weld(v[perm], faces_p, EPS, "first")
    la, lc = a.vertex_map.cpu().numpy(), c.vertex_map.cpu().numpy()
    assert c.stats["num_vertices"] == a.stats["num_vertices"] and ref.same_partition(lc, la[perm])
    assert np.array_equal(c.face_keep.cpu().numpy(), a.face_keep.cpu().numpy())
    assert c.stats["largest_cluster"] == a.stats["largest_cluster"]
    from diff_recon_hip import mesh_topology
    assert mesh_topology(c.stats["num_vertices"], c.faces) == mesh_topology(a.stats["num_vertices"], a.faces)
    assert np.array_equal(gpu_labels(v[perm], EPS), ref.labels(v[perm], EPS))


# ---- 7. guards --------------------------------------------------------------------------------------------------------------------------------
GUARD = 8


class Guarded:
    """`rows` rows of `width` elements between sentinel rows of one allocation."""

    def __init__(self, rows, width, dtype, sentinel):
        self.sentinel = sentinel
        self.block = torch.full((rows + 2 * GUARD, width), sentinel, device=DEV, dtype=dtype)
        self.view = self.block[GUARD:GUARD + rows]
        self.rows = rows
        assert self.view.is_contiguous()

    def untouched(self):
        s = torch.tensor(self.sentinel, dtype=self.block.dtype, device=DEV)
        lo, hi = self.block[:GUARD], self.block[GUARD + self.rows:]
        if self.block.dtype == torch.float32:
            lo, hi, s = lo.view(torch.int32), hi.view(torch.int32), s.view(torch.int32)
        return bool((lo == s).all()) and bool((hi == s).all())


def test_outputs_stay_between_their_guards(grid):
    from diff_recon_hip import mesh_weld
    from diff_triangle_rasterization_2D import _C as native
    lib = mesh_weld._lib
    v_np, faces_np, _ = _planted(grid)
    want = ref.weld(v_np, faces_np, EPS, "mean")
    V, F = len(v_np), len(faces_np)
    v, faces = _t(v_np), _t(faces_np.clip(-2 ** 31, 2 ** 31 - 1), torch.int32)
    label = Guarded(V, 1, torch.int32, -0x1234567)
    remap = Guarded(V, 1, torch.int32, -0x1234567)
    out_v = Guarded(V, 3, torch.float32, -7.25)
    count = Guarded(1, 1, torch.int32, -0x1234567)
    out_f = Guarded(F, 3, torch.int32, -0x1234567)
    keep = Guarded(F, 1, torch.uint8, 0xA5)
    counts = Guarded(1, 4, torch.int64, -0x0123456789ABCDEF)
    comp = Guarded(V, 1, torch.int32, -0x1234567)
    nbytes = lib.ts2d_weld_workspace_bytes(V, F)
    ws = Guarded(1, nbytes, torch.uint8, 0x5A)  # the workspace too: one row of exactly the bytes the size query asks for
    stream = torch.cuda.current_stream().cuda_stream
    everything = (label, remap, out_v, count, out_f, keep, counts, comp, ws)
    for mode in (0, 1):
        native._check(lib.ts2d_weld_labels(V, v.data_ptr(), EPS, label.view.data_ptr(), ws.view.data_ptr(), nbytes, stream), "labels")
        native._check(lib.ts2d_weld_compact(V, label.view.data_ptr(), v.data_ptr(), mode, remap.view.data_ptr(), out_v.view.data_ptr(),
                                            count.view.data_ptr(), ws.view.data_ptr(), nbytes, stream), "compact")
        native._check(lib.ts2d_weld_remap_faces(V, F, faces.data_ptr(), remap.view.data_ptr(), out_f.view.data_ptr(), keep.view.data_ptr(), stream), "remap")
        native._check(lib.ts2d_weld_edge_census(V, F, out_f.view.data_ptr(), keep.view.data_ptr(), counts.view.data_ptr(), ws.view.data_ptr(), nbytes,
                                                stream), "census")
        native._check(lib.ts2d_weld_face_components(V, F, out_f.view.data_ptr(), keep.view.data_ptr(), comp.view.data_ptr(), None, 0, stream), "components")
        torch.cuda.synchronize()
        assert all(g.untouched() for g in everything), [g.untouched() for g in everything]
        n = int(count.view.item())
        assert n == want["num_vertices"]
        assert np.array_equal(label.view[:, 0].cpu().numpy(), want["label"]) and np.array_equal(remap.view[:, 0].cpu().numpy(), want["remap"])
        assert np.array_equal(out_f.view.cpu().numpy(), want["faces"]) and np.array_equal(keep.view[:, 0].cpu().numpy(), want["keep"].astype(np.uint8))
        expect = want["vertices"] if mode == 1 else ref.compact(want["label"], v_np, "first")[1]
        assert np.array_equal(_bits(out_v.view[:n].cpu().numpy()), _bits(expect)) and not out_v.view[n:].any()  # the rows past V' are zero
        topo = ref.topology(V, want["faces"], want["keep"])
        assert counts.view[0].tolist() == [topo[k] for k in ("edges", "boundary", "manifold", "nonmanifold")]
        assert np.array_equal(comp.view[:, 0].cpu().numpy(), topo["label"])


def weld_call(inputs, eps=EPS):
    """The calls of include/ts_weld.h in a row on the current stream, each reading the device outputs of the ones before it; every documented
    output to its capacity (tests/replay.py; also tests/test_graph_replay_gpu.py at the smallest size)."""
    from diff_recon_hip import mesh_weld
    from diff_triangle_rasterization_2D import _C as native
    lib = mesh_weld._lib
    v, faces = inputs["v"], inputs["f"]
    V, F = v.shape[0], faces.shape[0]
    label, counted, remap = (torch.empty(V, device=DEV, dtype=torch.int32) for _ in range(3))
    visits = torch.zeros(1, device=DEV, dtype=torch.int64)  # "that the caller cleared"
    out_v, count = torch.empty((V, 3), device=DEV), torch.empty(1, device=DEV, dtype=torch.int32)
    mean_remap, mean_v, mean_count = torch.empty(V, device=DEV, dtype=torch.int32), torch.empty((V, 3), device=DEV), torch.empty(1, device=DEV, dtype=torch.int32)
    out_f, keep = torch.empty((F, 3), device=DEV, dtype=torch.int32), torch.empty(F, device=DEV, dtype=torch.uint8)
    counts, pieces = torch.empty(4, device=DEV, dtype=torch.int64), torch.empty(V, device=DEV, dtype=torch.int32)
    nbytes = lib.ts2d_weld_workspace_bytes(V, F)
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    s = torch.cuda.current_stream().cuda_stream
    native._check(lib.ts2d_weld_labels(V, v.data_ptr(), eps, label.data_ptr(), ws.data_ptr(), nbytes, s), "labels")
    native._check(lib.ts2d_weld_labels_counted(V, v.data_ptr(), eps, counted.data_ptr(), visits.data_ptr(), ws.data_ptr(), nbytes, s), "labels_counted")
    native._check(lib.ts2d_weld_compact(V, label.data_ptr(), v.data_ptr(), 1, mean_remap.data_ptr(), mean_v.data_ptr(), mean_count.data_ptr(),
                                        ws.data_ptr(), nbytes, s), "compact")
    native._check(lib.ts2d_weld_compact(V, counted.data_ptr(), v.data_ptr(), 0, remap.data_ptr(), out_v.data_ptr(), count.data_ptr(), ws.data_ptr(),
                                        nbytes, s), "compact")
    native._check(lib.ts2d_weld_remap_faces(V, F, faces.data_ptr(), remap.data_ptr(), out_f.data_ptr(), keep.data_ptr(), s), "remap")
    native._check(lib.ts2d_weld_edge_census(V, F, out_f.data_ptr(), keep.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes, s), "census")
    native._check(lib.ts2d_weld_face_components(V, F, out_f.data_ptr(), keep.data_ptr(), pieces.data_ptr(), ws.data_ptr(), nbytes, s), "components")
    return {"label": label, "label_counted": counted, "box_visits": visits, "remap": remap, "vertices": out_v, "count": count,
            "remap_mean": mean_remap, "vertices_mean": mean_v, "count_mean": mean_count, "faces": out_f, "keep": keep, "counts": counts,
            "pieces": pieces}


def test_the_calls_can_be_captured_in_a_graph(grid):
    """No allocation and no host synchronisation inside: a weld is captured once and replayed on other data of the same size.  Then the
    same through tests/replay.py: all the calls of the header in one graph, captured on the coincident vertices and replayed on the grid
    and on them in turn, every output compared with the eager run byte for byte."""
    from diff_recon_hip import mesh_weld
    from diff_triangle_rasterization_2D import _C as native
    lib = mesh_weld._lib
    v_np, f_np, _, want = grid
    V, F = len(v_np), len(f_np)
    v, faces = torch.zeros((V, 3), device=DEV), _t(f_np, torch.int32)
    label, remap = torch.empty(V, device=DEV, dtype=torch.int32), torch.empty(V, device=DEV, dtype=torch.int32)
    out_v, count = torch.empty((V, 3), device=DEV), torch.zeros(1, device=DEV, dtype=torch.int32)
    out_f, keep = torch.empty((F, 3), device=DEV, dtype=torch.int32), torch.empty(F, device=DEV, dtype=torch.uint8)
    counts = torch.zeros(4, device=DEV, dtype=torch.int64)
    nbytes = lib.ts2d_weld_workspace_bytes(V, F)
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            s = torch.cuda.current_stream().cuda_stream
            native._check(lib.ts2d_weld_labels(V, v.data_ptr(), EPS, label.data_ptr(), ws.data_ptr(), nbytes, s), "labels")
            native._check(lib.ts2d_weld_compact(V, label.data_ptr(), v.data_ptr(), 1, remap.data_ptr(), out_v.data_ptr(), count.data_ptr(), ws.data_ptr(),
                                                nbytes, s), "compact")
            native._check(lib.ts2d_weld_remap_faces(V, F, faces.data_ptr(), remap.data_ptr(), out_f.data_ptr(), keep.data_ptr(), s), "remap")
            native._check(lib.ts2d_weld_edge_census(V, F, out_f.data_ptr(), keep.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes, s), "census")
    torch.cuda.current_stream().wait_stream(side)
    v.copy_(_t(v_np))
    graph.replay()
    torch.cuda.synchronize()
    assert int(count.item()) == 400 and np.array_equal(remap.cpu().numpy(), want["remap"]) and bool(keep.all())
    assert counts.tolist() == [1121, 76, 1045, 0]
    v.zero_()  # all coincident: one cluster, every face collapses
    graph.replay()
    torch.cuda.synchronize()
    assert int(count.item()) == 1 and not bool(keep.any()) and counts.tolist() == [0, 0, 0, 0]
    del graph
    import replay
    case_a = {"v": _t(v_np), "f": _t(f_np, torch.int32)}
    case_b = {"v": torch.zeros((V, 3), device=DEV), "f": _t(f_np, torch.int32)}
    base_a, base_b, replays = replay.assert_replays(weld_call, case_a, case_b, differ=("count", "counts", "keep", "box_visits"))
    assert replays == 8
    i32, i64 = (lambda b, k: b[k].view(torch.int32).numpy()), (lambda b, k: b[k].view(torch.int64).tolist())
    assert i32(base_a, "count").tolist() == [400] and np.array_equal(i32(base_a, "remap"), want["remap"]) and bool(base_a["keep"].all())
    assert i64(base_a, "counts") == [1121, 76, 1045, 0] and np.array_equal(i32(base_a, "label"), i32(base_a, "label_counted"))
    assert i32(base_b, "count").tolist() == [1] and not bool(base_b["keep"].any()) and i64(base_b, "counts") == [0, 0, 0, 0]
    assert i32(base_a, "count_mean").tolist() == [400] and not i32(base_a, "pieces")[:400].any()  # the welded grid is one piece


# ---- 8. render --------------------------------------------------------------------------------------------------------------------------------
class Cam:  # the camera pattern of tests/test_mesh_gpu.py
    def __init__(self, s):
        self.device = DEV
        self.image_width, self.image_height = s["image_width"], s["image_height"]
        self.tan_fovx, self.tan_fovy = s["tanfovx"], s["tanfovy"]
        self.world_view_transform = torch.from_numpy(np.ascontiguousarray(s["viewmatrix"])).to(DEV)


def _render(cam, vertices, faces, colors):
    from diff_recon_hip import MeshRenderer
    out = MeshRenderer(Cam(cam)).render(vertices, faces, colors)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.fixture(scope="module")
def welded_render(grid):
    import synthetic
    v, f, _, _ = grid
    colors = ref.face_colors(len(f))
    w = gpu_weld(v, f, EPS, "first", colors)
    cam = synthetic.camera(ref.RENDER_W, ref.RENDER_H)
    return cam, w, _render(cam, w.vertices, w.faces, w.faces_color)


def test_welded_grid_renders_like_the_float64_checker(welded_render):
    cam, w, got = welded_render
    vertices, faces, colors = w.vertices.cpu().numpy(), w.faces.cpu().numpy().astype(np.int64), w.faces_color.cpu().numpy()
    want = ref_mesh_f64.render(vertices, faces, colors, ref.RENDER_W, ref.RENDER_H, cam["tanfovx"], cam["tanfovy"], cam["viewmatrix"])
    amb = want["ambiguous"]
    share = amb.mean()
    print(f"welded grid: ambiguous share {share:.4f}")
    assert share <= ref_mesh_f64.MAX_AMBIGUOUS_SHARE  # on the reference alone, before anything is compared
    fi, mask = got["face_idx"].astype(np.int64), got["mask"][0] > 0.5
    assert np.array_equal(mask, fi >= 0) and set(np.unique(got["mask"])) <= {0.0, 1.0}
    clear = ~amb
    wrong_face = int((fi != want["face_idx"])[clear].sum())
    wrong_mask = int((mask != want["mask"])[clear].sum())
    expect_rgb = np.where(mask[None], colors[np.maximum(fi, 0)].transpose(2, 0, 1), np.zeros(3, np.float32)[:, None, None])
    wrong_rgb = int((got["render"] != expect_rgb).any(0).sum())  # a copy of the face's colour: bit for bit, on every pixel
    both = clear & mask & want["mask"]
    rel = np.abs(got["depth"].astype(np.float64) - want["depth"])[both] / want["depth"][both]
    tol = 2 * want["eps"][want["face_idx"][both]]
    wrong_depth = int((rel > tol).sum())
    outside = sum(int(fi[y, x]) not in cand for (y, x), cand in want["candidates"].items())
    print(f"welded grid: non-ambiguous pixels {int(clear.sum())}, covered {int(both.sum())}: wrong face {wrong_face} mask {wrong_mask} depth {wrong_depth} "
          f"(max rel err / tol {float((rel / tol).max()):.3g}); wrong colour {wrong_rgb}; ambiguous pixels outside the candidates {outside}")
    assert both.sum() > 1000 and len(np.unique(fi[both])) > 300
    assert wrong_face == 0 and wrong_mask == 0 and wrong_rgb == 0 and wrong_depth == 0 and outside == 0
    assert np.all(got["depth"][~mask] == 0)


# ---- 9. file ----------------------------------------------------------------------------------------------------------------------------------
def test_welded_glb_holds_the_indexed_mesh_and_renders_the_same(tmp_path, grid, welded_render):
    from diff_recon_hip import RawTriangle
    from diff_recon_hip.mesh_renderer import load_glb_mesh
    from diff_recon_hip.raw_triangle import read_glb
    v, f, _, _ = grid
    cam, w, got = welded_render
    rng = np.random.default_rng(17)
    P = len(f)
    model = RawTriangle(v.reshape(P, 3, 3).copy(), rng.normal(size=(P, 1)).astype(np.float32), (0.5 * rng.normal(size=(P, 3))).astype(np.float32))
    kept = w.faces.cpu().numpy().astype(np.int64)
    for back in (True, False):
        path = str(tmp_path / f"welded_{back}.glb")
        model.saveGLB(path, save_back=back, process=True, weld_eps=EPS)
        doc, _ = read_glb(path)
        prim = doc["meshes"][0]["primitives"][0]
        assert doc["accessors"][prim["attributes"]["POSITION"]]["count"] == 400 and doc["accessors"][prim["attributes"]["COLOR_0"]]["count"] == 400
        assert doc["accessors"][prim["indices"]]["count"] == 3 * 722 * (2 if back else 1)
        vertices, faces, colors = load_glb_mesh(path, DEV)
        assert np.array_equal(_bits(vertices.cpu().numpy()), _bits(w.vertices.cpu().numpy()))  # the V' welded positions
        assert np.array_equal(faces.cpu().numpy().astype(np.int64), np.concatenate([kept, kept[:, ::-1]]) if back else kept)
        again = _render(cam, vertices, faces, colors)
        assert np.array_equal(again["mask"], got["mask"]) and np.array_equal(_bits(again["depth"]), _bits(got["depth"]))
        assert np.array_equal(again["face_idx"], got["face_idx"])  # a reversed twin never wins a pixel
    # COLOR_0: the mean RGBA of the incident kept front faces, summed in float64 in face order
    from diff_recon_hip.raw_triangle import SH2RGB, _accessor
    doc, binary = read_glb(str(tmp_path / "welded_True.glb"))
    col = _accessor(doc, binary, doc["meshes"][0]["primitives"][0]["attributes"]["COLOR_0"])
    rgba = np.concatenate([np.clip(SH2RGB(model.shs[:, :3]), 0, 1), 1 / (1 + np.exp(-model.opacity.reshape(-1, 1)))], axis=1).astype(np.float64)
    sums, count = np.zeros((400, 4)), np.zeros((400, 1))
    for face, c in zip(kept, rgba):
        for k in face:
            sums[k] += c
            count[k] += 1
    assert np.array_equal(col, np.round(sums / count * 255).astype(np.uint8))
    unwelded = str(tmp_path / "soup.glb")
    model.saveGLB(unwelded)  # process=False next to it: the soup, as before
    assert read_glb(unwelded)[0]["accessors"][0]["count"] == 3 * P


# ---- 10. example ------------------------------------------------------------------------------------------------------------------------------
def test_example_weld_mesh_reports_and_eps_zero_keeps_every_vertex():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic
    cfg = dict(iters=60, triangles=4000, width=160, height=112, views=3)  # the size tests/test_mesh_census_gpu.py uses for --refine-mesh
    _, m, _ = train_synthetic.train("2D", views_per_step=2, log=None, **cfg)
    P = m._vertex.shape[0]
    plain = train_synthetic.mesh_scores(m, "2D", **cfg)
    assert "welded" not in plain
    res = train_synthetic.mesh_scores(m, "2D", weld=0.0, **cfg)
    w = res["welded"]
    lines = train_synthetic.weld_report(w)
    print("\n".join(lines))
    assert res["psnr"] == plain["psnr"] and res["ssim"] == plain["ssim"]  # the unwelded figures are what they were
    assert w["stats"]["num_vertices_in"] == 3 * P and w["stats"]["num_vertices"] == 3 * P  # EPS = 0: V' == V
    assert w["stats"]["num_faces"] == P and w["stats"]["largest_cluster"] == 1 and w["stats"]["max_displacement"] == 0.0
    assert w["topology"]["pieces"] == P and w["topology"]["boundary"] == 3 * P and w["topology"]["euler"] == P
    assert w["psnr"] == plain["psnr"] and w["ssim"] == plain["ssim"]  # nothing moved: the front faces draw what the soup draws
    assert len(lines) == 4 and f"vertices {3 * P} -> {3 * P}, 0 of {P} faces dropped" in lines[0]
    assert "edges" in lines[1] and "pieces" in lines[1] and "largest cluster: 1 vertices" in lines[2] and "PSNR" in lines[3] and "the soup" in lines[3]
    res = train_synthetic.mesh_scores(m, "2D", refine=True, weld=2.0, **cfg)  # after --refine-mesh: the refined mesh is the one welded
    w, r = res["welded"], res["refined"]
    print("\n".join(train_synthetic.weld_report(w)))
    assert w["stats"]["num_vertices_in"] == 3 * r["kept"] and w["stats"]["num_vertices"] <= w["stats"]["num_vertices_in"]
    assert w["soup"]["mean_psnr"] == r["mean_psnr"] and len(w["psnr"]) == 3
