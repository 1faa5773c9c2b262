"""GPU tests of the mesh-distance feature against tests/ref_mesh_distance.py: the cross-set nearest search (indices equal, squared distances
bit-equal), the surface sampler (faces equal, points bit-equal), the scores, RawTriangle's set difference and the example's report."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

import ref_mesh_distance as ref
from test_knn_gpu import _pts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _search(q, r):
    from diff_recon_hip.mesh_distance import nearest_points
    visits = torch.zeros(1, device="cuda", dtype=torch.int64)
    idx, d2 = nearest_points(_dev(q), _dev(r), visits)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (len(q),)
    return idx.cpu().numpy(), d2.cpu().numpy(), int(visits.item())


def _check_search(q, r):
    idx, d2, visits = _search(q, r)
    want_idx, want_d2 = ref.nearest(q, r)
    assert np.array_equal(idx, want_idx), np.nonzero(idx != want_idx)[0][:10]
    assert np.array_equal(_bits(d2), _bits(want_d2))
    return idx, d2, visits


# ---- nearest search ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,R,kind", [(1, 1, "uniform"), (9, 5, "uniform"), (1000, 1025, "uniform"), (1025, 1000, "uniform"),
                                      (8192, 8192, "uniform"), (3000, 5000, "clustered")])
def test_nearest_matches_brute_force(Q, R, kind):
    _check_search(_pts(Q, 1, kind), _pts(R, 2, kind))


def test_query_cluster_far_from_all_refs_sweeps_every_box():
    refs = _pts(4096, 3)
    extent = float(np.ptp(refs, axis=0).max())
    rng = np.random.default_rng(4)
    queries = (np.array([50 * extent, -50 * extent, 50 * extent], np.float32) + rng.normal(size=(20000, 3)) * 0.01 * extent).astype(np.float32)
    _, _, visits = _check_search(queries, refs)
    assert 20 <= visits <= 20 * 4  # 20 workgroups, 4 ref boxes: the seed box always, the others while their bound is within the radius


def test_duplicate_refs_the_smallest_index_wins():
    rng = np.random.default_rng(5)
    distinct = rng.random((64, 3), dtype=np.float32) * 10
    which = rng.permutation(np.repeat(np.arange(64), 40))
    refs = distinct[which]
    idx, d2, _ = _check_search(distinct, refs)
    first = np.array([np.nonzero(which == k)[0][0] for k in range(64)])
    assert np.array_equal(idx, first) and (d2 == 0).all()


def test_eight_exact_ties_across_boxes():
    g = np.arange(12, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)  # 1728 refs: two boxes
    refs = lattice[np.random.default_rng(6).permutation(len(lattice))]
    c = np.arange(11, dtype=np.float32) + np.float32(0.5)
    queries = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
    idx, d2, _ = _check_search(queries, refs)
    assert (d2 == 0.75).all()
    corner = np.abs(refs[None, :, :] - queries[:, None, :]).max(axis=2) == 0.5
    assert (corner.sum(axis=1) == 8).all() and np.array_equal(idx, corner.argmax(axis=1))


def test_non_finite_refs_and_queries():
    refs, queries = _pts(3000, 7), _pts(1500, 8)
    rng = np.random.default_rng(9)
    for row, col, val in zip(rng.choice(3000, 600, replace=False), rng.integers(0, 3, 600), rng.choice([NAN, INF, -INF], 600)):
        refs[row, col] = val
    for row, col, val in zip(rng.choice(1500, 100, replace=False), rng.integers(0, 3, 100), rng.choice([NAN, INF, -INF], 100)):
        queries[row, col] = val
    queries[1024:1500] = NAN  # a workgroup without a single finite query
    idx, d2, _ = _check_search(queries, refs)
    bad = ~np.isfinite(queries).all(axis=1)
    assert (idx[bad] == -1).all() and np.isnan(d2[bad]).all() and (idx[~bad] >= 0).all()
    assert np.isfinite(refs[idx[~bad]]).all()
    idx, d2, _ = _check_search(queries, np.where(np.arange(3000)[:, None] % 2 == 0, NAN, INF).astype(np.float32) * np.ones((1, 3), np.float32))
    assert (idx == -1).all() and np.isinf(d2[~bad]).all() and np.isnan(d2[bad]).all()


def test_overflowing_distances_still_name_the_smallest_index():
    rng = np.random.default_rng(10)
    refs = rng.choice(np.array([-3e38, 3e38], np.float32), (2000, 3))  # a query coordinate of 1 is 3e38 from every ref: d = +inf
    queries = rng.choice(np.array([-3e38, 1.0, 3e38], np.float32), (300, 3))
    idx, d2, _ = _check_search(queries, refs)
    assert np.isinf(d2).any() and (d2 == 0).any() and (idx >= 0).all() and (idx[np.isinf(d2)] == 0).all()
    idx, d2, _ = _check_search(np.array([[-3e38, -3e38, -3e38]], np.float32), np.array([[3e38, 3e38, 3e38], [-3e38, 3e38, 0]], np.float32))
    assert idx[0] == 0 and np.isinf(d2[0])


def test_empty_sets():
    queries = _pts(10, 11)
    queries[3, 1] = NAN
    idx, d2, visits = _check_search(queries, np.zeros((0, 3), np.float32))
    assert (idx == -1).all() and np.isnan(d2[3]) and np.isinf(np.delete(d2, 3)).all() and visits == 0
    idx, d2, _ = _search(np.zeros((0, 3), np.float32), _pts(10, 12))
    assert idx.shape == (0,) and d2.shape == (0,)


# ---- sampler ------------------------------------------------------------------------------------------------------------------------------------
def _sample(v, f, n, seed=0, keep=None):
    from diff_recon_hip.mesh_distance import face_areas, sample_mesh_surface
    keep_t = None if keep is None else _dev(keep)
    area = face_areas(_dev(v), _dev(f), keep_t).cpu().numpy()
    s = sample_mesh_surface(_dev(v), _dev(f), n, seed, keep_t)
    assert s.points.dtype == torch.float32 and s.face.dtype == torch.int32 and s.points.shape == (n, 3) and s.face.shape == (n,)
    return s.points.cpu().numpy(), s.face.cpu().numpy(), s.area, area


def _check_sample(v, f, n, seed=0, keep=None):
    points, face, total, area = _sample(v, f, n, seed, keep)
    want_area = ref.face_areas(v, f, keep)
    assert np.array_equal(_bits(area), _bits(want_area))
    want_points, want_face = ref.sample(v, f, want_area, n, seed)
    assert np.array_equal(face, want_face)
    assert np.array_equal(_bits(points), _bits(want_points))
    assert total == pytest.approx(float(want_area.sum()), rel=1e-12)
    assert ref.barycentric_excess(v, f, points, face) < 1e-5  # every point lies in its face
    return points, face, area


@functools.lru_cache(maxsize=None)
def _soup():
    return ref.heavy_tailed_soup(5000, seed=3)


def test_sampler_one_triangle_and_one_sample():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 1]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    _, face, area = _check_sample(v, f, 777, seed=1)
    assert (face == 0).all() and area[0] == 0.5 * np.sqrt(36.0 + 4.0)
    _check_sample(v, f, 1, seed=2)
    _check_sample(*_soup(), 1, seed=2)


def test_sampler_never_draws_a_face_below_the_weight_resolution():
    s = np.float32(2.0 ** -17)  # the middle face: 0.5 * s * 4 s = 2^-33 exactly, weight floor(2^-33 * 2^32) = 0
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 5], [s, 0, 5], [0, 4 * s, 5], [9, 0, 0], [10, 0, 0], [9, 2, 0]], np.float32)
    f = np.arange(9, dtype=np.int32).reshape(3, 3)
    _, face, area = _check_sample(v, f, 4001, seed=3)
    assert area[0] == area[2] == 1.0 and area[1] == 2.0 ** -33
    count = np.bincount(face, minlength=3)
    assert count[1] == 0 and abs(int(count[0]) - int(count[2])) <= 1


def test_sampler_heavy_tailed_soup():
    v, f = _soup()
    _, face, area = _check_sample(v, f, 20000, seed=11)
    assert (np.diff(face) >= 0).all()
    w, C = ref.weights(area)
    assert np.abs(np.bincount(face, minlength=5000) - 20000 * w.astype(np.float64) / float(C[-1])).max() < 2


def test_sampler_skips_invalid_faces():
    v, f = (a.copy() for a in _soup())
    rng = np.random.default_rng(12)
    keep = rng.random(5000) < 0.6
    f[rng.choice(5000, 200, replace=False), rng.integers(0, 3, 200)] = rng.choice([-1, 15000, 2 ** 31 - 1, -2 ** 31], 200)  # out of range
    v[rng.choice(15000, 150, replace=False), rng.integers(0, 3, 150)] = rng.choice([NAN, INF, -INF], 150)
    flat = rng.choice(5000, 100, replace=False)
    v[f[flat, 2].clip(0, 14999)] = v[f[flat, 1].clip(0, 14999)]  # zero-area faces
    for k in (None, keep):
        _, face, area = _check_sample(v, f, 6000, seed=13, keep=k)
        assert (area[face] > 0).all()
        invalid = ((f < 0) | (f >= 15000)).any(axis=1)
        assert (area[invalid] == 0).all() and (k is None or (area[~k] == 0).all())
        assert np.isfinite(area).all()


def test_sampler_without_area_raises():
    from diff_recon_hip.mesh_distance import sample_mesh_surface
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 0, 0], [0, 1, 7]], np.int32)
    with pytest.raises(ValueError, match="no surface"):
        sample_mesh_surface(_dev(v), _dev(f), 10)
    with pytest.raises(ValueError, match="no surface"):
        sample_mesh_surface(_dev(v), _dev(np.zeros((0, 3), np.int32)), 10)
    with pytest.raises(ValueError, match="no surface"):
        sample_mesh_surface(*map(_dev, _soup()), 10, keep=torch.zeros(5000, dtype=torch.bool, device="cuda"))


def test_sampler_is_a_function_of_the_seed():
    v, f = _soup()
    a, fa, _, _ = _sample(v, f, 5000, seed=21)
    b, fb, _, _ = _sample(v, f, 5000, seed=21)
    c, fc, _, _ = _sample(v, f, 5000, seed=22)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(fa, fb)
    assert not np.array_equal(_bits(a), _bits(c))
    d, fd, _, _ = _sample(v, f, 5000, seed=21 + 2 ** 64)  # the seed is taken mod 2^64
    assert np.array_equal(_bits(a), _bits(d)) and np.array_equal(fa, fd)


# ---- scores -------------------------------------------------------------------------------------------------------------------------------------
def _same_scores(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        if k in ("a_count", "b_count", "a_dropped", "b_dropped", "a_within", "b_within"):
            assert got[k] == w and all(isinstance(x, int) for x in (got[k] if isinstance(got[k], list) else [got[k]])), k
        else:
            assert np.allclose(got[k], w, rtol=1e-9, atol=0, equal_nan=True), (k, got[k], w)


def test_scores_match_the_float64_reference():
    from diff_recon_hip.mesh_distance import point_cloud_distance
    a, b = _pts(3000, 31), _pts(2500, 32) + np.float32(0.05)
    a[7, 0], b[9, 2], b[11, 1] = NAN, INF, NAN
    thresholds = [0.05, 0.2, 0.5, 100.0]
    got = point_cloud_distance(_dev(a), _dev(b), thresholds)
    want = ref.point_cloud_distance(a, b, thresholds)
    _same_scores(got, want)
    assert got["a_dropped"] == 1 and got["b_dropped"] == 2 and got["precision"][-1] == 1.0 and got["fscore"][-1] == 1.0
    far = point_cloud_distance(_dev(a), _dev(b + np.float32(1000)), [1.0])
    assert far["precision"] == [0.0] and far["recall"] == [0.0] and far["fscore"] == [0.0]


def test_known_answer_two_parallel_squares():
    from diff_recon_hip.mesh_distance import mesh_distance
    h = 0.5
    a, b = ref.two_squares(h)
    res = mesh_distance(tuple(map(_dev, a)), tuple(map(_dev, b)), 2000, seed=0, thresholds=[h / 2, 2 * h])
    print(res["accuracy"] / h - 1, res["completeness"] / h - 1)
    assert h <= res["accuracy"] <= h * (1 + 1e-3) and h <= res["completeness"] <= h * (1 + 1e-3)
    assert res["precision"] == [0.0, 1.0] and res["recall"] == [0.0, 1.0]
    assert res["area_a"] == 1.0 and res["area_b"] == 1.0
    _same_scores(res, ref.mesh_distance(a, b, 2000, seed=0, thresholds=[h / 2, 2 * h]))


# ---- RawTriangle ----------------------------------------------------------------------------------------------------------------------------------
def test_raw_triangle_difference_follows_the_kd_tree_rule():
    from scipy.spatial import cKDTree
    from diff_recon_hip import RawTriangle
    rng = np.random.default_rng(41)
    P = 3000
    a = RawTriangle(rng.random((P, 3, 3), dtype=np.float32) * 10, rng.random((P, 1), dtype=np.float32), rng.random((P, 12), dtype=np.float32))
    copies = rng.choice(P, 1100, replace=False)
    far = rng.random((900, 3, 3), dtype=np.float32) * 10 + np.float32(100)
    b = RawTriangle(np.concatenate([a.vertex[copies], far])[rng.permutation(2000)], np.zeros((2000, 1), np.float32), np.zeros((2000, 12), np.float32))
    distance, _ = cKDTree(b.center.astype(np.float64)).query(a.center.astype(np.float64))
    assert not ((distance > 1e-6) & (distance < 1e-4)).any()  # no centre distance near the threshold: the fp32 search cannot disagree
    keep = distance > 1e-5
    assert keep.sum() == P - 1100
    before = copy.deepcopy(a)
    diff = a - b
    assert diff is not a and len(a) == P
    for name in ("vertex", "opacity", "shs", "contained_idx"):
        assert np.array_equal(getattr(a, name), getattr(before, name)), name  # a itself is unchanged
        assert np.array_equal(getattr(diff, name), getattr(before, name)[keep] if name != "contained_idx" else np.ones(keep.sum(), bool)), name
    a -= b
    assert np.array_equal(a.vertex, diff.vertex) and len(a) == P - 1100


# ---- example --------------------------------------------------------------------------------------------------------------------------------------
def test_example_reports_geometry():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic
    cfg = dict(iters=30, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    res = train_synthetic.mesh_scores(m, "2D", geometry=2000, **cfg)
    g = res["geometry"]
    lines = train_synthetic.geometry_report(g)
    print("\n".join(lines))
    assert "geometry" not in train_synthetic.mesh_scores(m, "2D", **cfg)
    for k in ("accuracy", "completeness", "chamfer", "chamfer_sq", "hausdorff", "area_a", "area_b", "median_edge"):
        assert np.isfinite(g[k]) and g[k] > 0, k
    assert len(g["fscore"]) == 3 and all(0.0 <= x <= 1.0 for x in g["fscore"] + g["precision"] + g["recall"])
    assert g["thresholds"] == pytest.approx([0.5 * g["median_edge"], g["median_edge"], 2 * g["median_edge"]])
    assert g["a_within"] == sorted(g["a_within"]) and g["a_count"] == g["b_count"] == 2000
    assert len(lines) == 3 and all(line.startswith("mesh geometry") for line in lines) and "F-score" in lines[1]
