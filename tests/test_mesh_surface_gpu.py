"""GPU tests of the point-to-surface feature against tests/ref_mesh_surface.py: MeshBVH.closest returns the brute-force face, and the squared
distance and the closest point bit for bit, on every boundary of the structure (leaves of 8 faces, fan-out 8: 8 / 64 / 512 / 4096 faces; waves
of 64 queries, workgroups of 256); the scores on known answers; purity; pruning; the example's report."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import poison
import ref_mesh_distance as refd
import ref_mesh_surface as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = np.float32(np.nan), np.float32(np.inf)
LEAF = 8  # faces per leaf (csrc/mesh_bvh.hip)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _closest(q, v, f, keep=None):
    from diff_recon_hip import MeshBVH
    visits = torch.zeros(1, device="cuda", dtype=torch.int64)
    face, d2, point = MeshBVH(_dev(v), _dev(f), None if keep is None else _dev(keep)).closest(_dev(q), visits)
    assert face.dtype == torch.int32 and d2.dtype == torch.float64 and point.dtype == torch.float32
    assert face.shape == d2.shape == (len(q),) and point.shape == (len(q), 3)
    return face.cpu().numpy(), d2.cpu().numpy(), point.cpu().numpy(), int(visits.item())


def _check(q, v, f, keep=None):
    face, d2, point, visits = _closest(q, v, f, keep)
    want_face, want_d2, want_point = ref.closest(q, v, f, keep)
    assert np.array_equal(face, want_face), (np.nonzero(face != want_face)[0][:10], face[face != want_face][:10], want_face[face != want_face][:10])
    assert np.array_equal(d2.view(np.uint64), want_d2.view(np.uint64)), np.nonzero(d2.view(np.uint64) != want_d2.view(np.uint64))[0][:10]
    assert np.array_equal(point.view(np.uint32), want_point.view(np.uint32)), np.nonzero((point.view(np.uint32) != want_point.view(np.uint32)).any(axis=1))[0][:10]
    return face, d2, point, visits


def _queries(Q, v, seed):
    """Q queries around the finite vertices `v`: uniform in their box grown by a quarter, and every fourth one ON a vertex."""
    rng = np.random.default_rng(seed)
    fin = v[np.isfinite(v).all(axis=1)]
    lo, hi = fin.min(axis=0).astype(np.float64), fin.max(axis=0).astype(np.float64)
    q = (lo - 0.25 * (hi - lo) + rng.random((Q, 3)) * 1.5 * (hi - lo)).astype(np.float32)
    q[::4] = fin[rng.integers(0, len(fin), len(q[::4]))]
    return q


@functools.lru_cache(maxsize=None)
def _soup(F):
    return refd.heavy_tailed_soup(F, seed=F)


@functools.lru_cache(maxsize=None)
def _grid(F):
    v, f = ref.grid_mesh(max(1, int(np.ceil(np.sqrt(F / 2)))), seed=F)
    return v, f[:F]


# ---- parity ------------------------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (9, 2), (65, 63), (130, 65), (700, 1025), (1500, 4097),            # the issue's
         (64, 8), (257, 9), (64, 64), (256, 512), (100, 513), (100, 4096), (3, 7)]  # this structure's: one leaf / two, one level / two / three / four / five


@pytest.mark.parametrize("kind", ["soup", "grid"])
@pytest.mark.parametrize("Q,F", SIZES)
def test_closest_matches_brute_force(Q, F, kind):
    v, f = (_soup if kind == "soup" else _grid)(F)
    assert len(f) == F
    face, d2, _, _ = _check(_queries(Q, v, Q + F), v, f)
    assert (face >= 0).all() and np.isfinite(d2).all()


def test_grid_mesh_queries_on_shared_edges_and_vertices_tie_to_the_smallest_index():
    v, f = _grid(800)
    rng = np.random.default_rng(1)
    tri = v[f[rng.integers(0, len(f), 600)]]
    on_edge = (0.5 * tri[:, 0] + 0.5 * tri[:, 1]).astype(np.float32)  # fp32 midpoints: on the edge or within a rounding of it
    face, d2, _, _ = _check(np.concatenate([v, on_edge]), v, f)
    at_vertex = face[:len(v)]
    uses = [np.nonzero((f == k).any(axis=1))[0] for k in range(len(v))]
    assert all(at_vertex[k] == u.min() for k, u in enumerate(uses) if len(u)) and (d2[:len(v)][[len(u) > 0 for u in uses]] == 0).all()


def test_every_face_repeated_and_shuffled_the_smallest_index_wins():
    v, f = _soup(64)
    which = np.random.default_rng(2).permutation(np.repeat(np.arange(64), 40))
    q = np.concatenate([v, _queries(300, v, 3)])
    face, d2, _, _ = _check(q, v, f[which])
    first = np.array([np.nonzero(which == k)[0][0] for k in range(64)])
    assert np.isin(face, first).all()
    assert (d2[:len(v)] == 0).all()  # the queries at the vertices


def _spoiled(F, seed):
    v, f = (a.copy() for a in _soup(F))
    rng = np.random.default_rng(seed)
    keep = (rng.random(F) < 0.93).astype(np.uint8)
    n = max(1, F // 15)
    f[rng.choice(F, n, replace=False), rng.integers(0, 3, n)] = rng.choice([-1, 3 * F, 2 ** 31 - 1, -2 ** 31], n)
    v[rng.choice(3 * F, n, replace=False), rng.integers(0, 3, n)] = rng.choice([NAN, INF, -INF], n)
    return v, f, keep


def test_ineligible_faces_are_never_returned():
    v, f, keep = _spoiled(2000, 4)
    eligible = ref.eligible_faces(v, f, keep)
    assert 0.7 * 2000 < len(eligible) < 0.9 * 2000  # about 20 % are ineligible, for every one of the three reasons
    q = _queries(700, v, 5)
    face, _, _, _ = _check(q, v, f, keep)
    assert np.isin(face, eligible).all()
    face, _, _, _ = _check(q, v, f, keep.astype(bool))  # a bool mask
    face, _, _, _ = _check(q, v, f)                     # no mask: more faces are eligible
    assert not np.isin(face, eligible).all()
    from diff_recon_hip import MeshBVH
    wide = MeshBVH(_dev(v.astype(np.float64)), _dev(f.astype(np.int64)), _dev(keep)).closest(_dev(q))  # float64 vertices, int64 faces
    assert np.array_equal(wide[0].cpu().numpy(), ref.closest(q, v, f, keep)[0])


def test_zero_area_faces_are_eligible():
    v, f = (a.copy() for a in _soup(300))
    rng = np.random.default_rng(6)
    seg, pt = rng.choice(300, 60, replace=False), rng.choice(300, 30, replace=False)
    v[f[seg, 1]] = v[f[seg, 0]]                     # a == b: a segment
    v[f[pt, 1]] = v[f[pt, 2]] = v[f[pt, 0]]         # a == b == c: a point
    q = np.concatenate([_queries(400, v, 7), v[f[pt, 0]], (v[f[seg, 0]] * 0.25 + v[f[seg, 2]] * 0.75).astype(np.float32)])
    face, d2, _, _ = _check(q, v, f)
    assert np.isin(pt, face).any() and np.isin(seg, face).any() and np.isfinite(d2).all()


def test_no_eligible_face_and_no_face():
    v, f = _soup(100)
    q = _queries(70, v, 8)
    q[5, 1], q[69, 0] = NAN, INF
    for vv, ff, keep in ((v, f, np.zeros(100, np.uint8)), (np.full_like(v, NAN), f, None), (v, np.zeros((0, 3), np.int32), None),
                         (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None)):
        face, d2, point, visits = _check(q, vv, ff, keep)
        bad = np.arange(70) % 64 == 5
        assert (face == -1).all() and np.isnan(d2[bad]).all() and np.isposinf(d2[~bad]).all() and np.isnan(point).all()
        assert visits == 0 if len(ff) == 0 else visits <= 2  # two waves: at most their seed leaves, every node above is empty
    from diff_recon_hip import point_to_mesh_distance
    face, d2, point = point_to_mesh_distance(_dev(np.zeros((0, 3), np.float32)), (_dev(v), _dev(f)))
    assert face.shape == (0,) and d2.shape == (0,) and point.shape == (0, 3)


def test_non_finite_queries():
    v, f = _soup(1025)
    q = _queries(1500, v, 9)
    rng = np.random.default_rng(10)
    for row, col, val in zip(rng.choice(1500, 100, replace=False), rng.integers(0, 3, 100), rng.choice([NAN, INF, -INF], 100)):
        q[row, col] = val
    q[1300:1500] = NAN  # 200 in a row, and in a row after the stable sort too (one Morton code): whole waves without a live lane
    face, d2, point, _ = _check(q, v, f)
    bad = ~np.isfinite(q).all(axis=1)
    assert bad.sum() >= 290 and (face[bad] == -1).all() and np.isnan(d2[bad]).all() and np.isnan(point[bad]).all() and (face[~bad] >= 0).all()
    _check(np.full((64, 3), INF, np.float32), v, f)  # one wave, nobody alive


def test_query_cluster_far_from_the_mesh():
    v, f = _soup(4097)
    extent = float(np.ptp(v, axis=0).max())
    rng = np.random.default_rng(11)
    q = (np.array([50 * extent, -50 * extent, 50 * extent]) + rng.normal(size=(2000, 3)) * 0.01 * extent).astype(np.float32)
    _, _, _, visits = _check(q, v, f)
    waves, leaves = -(-2000 // 64), -(-4097 // LEAF)
    print(f"far cluster: {visits} leaf visits, {visits / waves:.1f} per wave of {leaves} leaves")
    assert waves <= visits <= waves * leaves


def test_coordinates_at_the_fp32_range():
    rng = np.random.default_rng(12)
    v = (rng.uniform(-1, 1, (600, 3)) * 3e38).astype(np.float32)
    f = rng.integers(0, 600, (900, 3)).astype(np.int32)
    q = (rng.uniform(-1, 1, (500, 3)) * 3e38).astype(np.float32)
    q[::5] = v[rng.integers(0, 600, 100)]
    face, d2, point, _ = _check(q, v, f)
    assert (face >= 0).all() and np.isfinite(d2).all() and np.isfinite(point).all()
    assert d2.max() > float(np.finfo(np.float32).max)  # squared distances that fp32 could not hold


# ---- known answers and scores ----------------------------------------------------------------------------------------------------------------------
def test_known_answer_two_parallel_squares():
    from diff_recon_hip import mesh_distance, mesh_surface_distance, point_to_mesh_distance, sample_mesh_surface
    a, b = refd.two_squares(0.5)
    ga, gb = tuple(map(_dev, a)), tuple(map(_dev, b))
    pa = sample_mesh_surface(*ga, 2000, seed=0).points
    face, d2, point = point_to_mesh_distance(pa, gb)
    assert (d2 == 0.25).all() and (point[:, 2] == 0.5).all() and torch.equal(point[:, :2], pa[:, :2]) and (face >= 0).all()
    res = mesh_surface_distance(ga, gb, 2000, seed=0, thresholds=[0.25, 0.5, 1.0])
    assert res["accuracy"] == 0.5 and res["completeness"] == 0.5 and res["chamfer"] == 0.5 and res["chamfer_sq"] == 0.5 and res["hausdorff"] == 0.5
    assert res["precision"] == [0.0, 1.0, 1.0] and res["recall"] == [0.0, 1.0, 1.0] and res["fscore"] == [0.0, 1.0, 1.0]
    assert res["a_within"] == [0, 2000, 2000] and res["a_count"] == res["b_count"] == 2000 and res["a_dropped"] == res["b_dropped"] == 0
    assert res["area_a"] == 1.0 and res["area_b"] == 1.0
    assert set(res) == set(mesh_distance(ga, gb, 100)) and set(res) == set(refd.mesh_distance(a, b, 100))


def test_scores_match_the_float64_reference_and_a_mesh_scores_zero_against_itself():
    from diff_recon_hip import mesh_distance, mesh_surface_distance
    va, fa = _grid(800)
    vb, fb = ref.grid_mesh(17, seed=99)
    vb = vb + np.float32(0.01)
    thresholds = [0.005, 0.02, 0.1]
    got = mesh_surface_distance((_dev(va), _dev(fa)), (_dev(vb), _dev(fb)), 3000, seed=5, thresholds=thresholds)
    pa, _ = refd.sample(va, fa, refd.face_areas(va, fa), 3000, 5)
    pb, _ = refd.sample(vb, fb, refd.face_areas(vb, fb), 3000, 6)
    face_ab, d2_ab, _ = ref.closest(pa, vb, fb)
    face_ba, d2_ba, _ = ref.closest(pb, va, fa)
    want = ref.scores(face_ab, d2_ab, face_ba, d2_ba, thresholds)
    for k, w in want.items():
        if k in ("a_count", "b_count", "a_dropped", "b_dropped", "a_within", "b_within"):
            assert got[k] == w, k
        else:
            assert np.allclose(got[k], w, rtol=1e-12, atol=0), (k, got[k], w)  # bit-equal distances; the sums may associate differently
    mesh = (_dev(va), _dev(fa))
    same = mesh_surface_distance(mesh, mesh, 3000, seed=5, thresholds=[1e-6])
    bar = 8 * 2.0 ** -24 * float(np.abs(va).max())  # the fp32 rounding of the sampler's point: three rounded operations per coordinate
    p2p = mesh_distance(mesh, mesh, 3000, seed=5)
    print(f"a mesh against itself: to the surface {same['accuracy']:.3g} / {same['completeness']:.3g} (bar {bar:.3g}), point to point {p2p['accuracy']:.3g} / {p2p['completeness']:.3g}")
    assert same["accuracy"] <= bar and same["completeness"] <= bar and same["precision"] == [1.0] and same["recall"] == [1.0]
    assert p2p["accuracy"] > 100 * bar


# ---- purity, determinism ------------------------------------------------------------------------------------------------------------------------------
def test_build_and_closest_are_pure_and_permuting_the_queries_permutes_the_results():
    from diff_recon_hip import MeshBVH
    v, f, keep = _spoiled(1025, 13)
    q = _queries(700, v, 14)
    q[3, 2] = NAN
    gv, gf, gk, gq = _dev(v), _dev(f), _dev(keep), _dev(q)

    def call(pattern):  # the index, both workspaces and the three outputs come from torch.empty: all poisoned
        visits = torch.zeros(1, device="cuda", dtype=torch.int64)
        bvh = MeshBVH(gv, gf, gk)
        face, d2, point = bvh.closest(gq, visits)
        return {"face": face, "dist2": d2, "point": point, "visits": int(visits.item())}

    base = poison.assert_pure(call)
    want_face, want_d2, want_point = ref.closest(q, v, f, keep)
    assert np.array_equal(base["face"].numpy().view(np.int32), want_face) and np.array_equal(base["dist2"].numpy().view(np.uint64), want_d2.view(np.uint64))
    assert np.array_equal(base["point"].numpy().view(np.uint32).reshape(-1, 3), want_point.view(np.uint32))
    perm = np.random.default_rng(15).permutation(700)
    face, d2, point, _ = _closest(q[perm], v, f, keep)
    assert np.array_equal(face, want_face[perm]) and np.array_equal(d2.view(np.uint64), want_d2[perm].view(np.uint64))
    assert np.array_equal(point.view(np.uint32), want_point[perm].view(np.uint32))


# ---- pruning ------------------------------------------------------------------------------------------------------------------------------------------
LEAF_VISITS_CAP = 2 * 5882  # 2 x the figure measured on the MI355X; the count is a function of the input, not of the run


def test_the_hierarchy_prunes():
    from diff_recon_hip import MeshBVH, sample_mesh_surface
    v, f = ref.small_triangle_soup(16384, seed=16)
    gv, gf = _dev(v), _dev(f)
    samples = sample_mesh_surface(gv, gf, 8192, seed=17)
    visits = torch.zeros(1, device="cuda", dtype=torch.int64)
    face, d2, _ = MeshBVH(gv, gf).closest(samples.points, visits)
    waves, leaves = 8192 // 64, 16384 // LEAF
    n = int(visits.item())
    print(f"8192 samples on 16384 small triangles: {n} leaf visits = {n / waves:.1f} per wave, brute force {waves * leaves}")
    bar = 8 * 2.0 ** -24 * float(np.abs(v).max())
    assert float(d2.max().sqrt()) <= bar  # every sample lies on the soup
    assert n < waves * leaves // 2
    assert n <= LEAF_VISITS_CAP
    sub = np.arange(0, 8192, 16)
    want_face, want_d2, _ = ref.closest(samples.points.cpu().numpy()[sub], v, f)
    assert np.array_equal(face.cpu().numpy()[sub], want_face) and np.array_equal(d2.cpu().numpy()[sub].view(np.uint64), want_d2.view(np.uint64))


# ---- example ------------------------------------------------------------------------------------------------------------------------------------------
def test_example_reports_surface_scores():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    res = train_synthetic.mesh_scores(m, "2D", geometry=2000, surface=2000, **cfg)
    s, g = res["surface"], res["geometry"]
    lines = train_synthetic.geometry_report(s, title="mesh surface")
    print("\n".join(lines))
    assert "surface" not in train_synthetic.mesh_scores(m, "2D", **cfg)
    for k in ("accuracy", "completeness", "chamfer", "chamfer_sq", "hausdorff", "area_a", "area_b", "median_edge"):
        assert np.isfinite(s[k]) and s[k] > 0, k
    assert s["accuracy"] < g["accuracy"] and s["completeness"] < g["completeness"]  # the same samples: a surface is never farther than its samples
    assert len(s["fscore"]) == 3 and all(0.0 <= x <= 1.0 for x in s["fscore"] + s["precision"] + s["recall"])
    assert s["thresholds"] == g["thresholds"] and s["a_count"] == s["b_count"] == 2000 and s["area_a"] == g["area_a"]
    assert len(lines) == 3 and all(line.startswith("mesh surface") for line in lines) and "F-score" in lines[1]
