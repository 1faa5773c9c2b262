"""GPU tests of the ray-casting feature against tests/ref_mesh_ray.py: ray_cast returns the brute-force first hit -- face, t, barycentric
weights and side bit for bit -- on every boundary of the structure (leaves of 8 faces, fan-out 8; waves of 64 rays, workgroups of 256), is
watertight on a closed mesh, pure, and prunes; camera_rays agrees with MeshRenderer; point_visibility and the visibility-aware scores on
known answers; the example's report."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import poison
import ref_mesh_distance as refd
import ref_mesh_ray as ref
import ref_mesh_surface as refs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = np.float32(np.nan), np.float32(np.inf)
LEAF = 8  # faces per leaf (csrc/ts_bvh_layout.h)
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cast(o, d, v, f, keep=None, **kw):
    from diff_recon_hip import MeshBVH, RayHits, ray_cast
    visits = torch.zeros(1, device=DEV, dtype=torch.int64)
    if "t_limit" in kw and kw["t_limit"] is not None:
        kw = dict(kw, t_limit=_dev(kw["t_limit"]))
    hits = ray_cast(MeshBVH(_dev(v), _dev(f), None if keep is None else _dev(keep)), _dev(o), _dev(d), leaf_visits=visits, **kw)
    assert isinstance(hits, RayHits)
    assert hits.face.dtype == torch.int32 and hits.t.dtype == torch.float64 and hits.bary.dtype == torch.float32 and hits.side.dtype == torch.int8
    assert hits.face.shape == hits.t.shape == hits.side.shape == (len(o),) and hits.bary.shape == (len(o), 3)
    return hits.face.cpu().numpy(), hits.t.cpu().numpy(), hits.bary.cpu().numpy(), hits.side.cpu().numpy(), int(visits.item())


def _same(got, want):
    face, t, bary, side = got[:4]
    wf, wt, wb, ws = want
    assert np.array_equal(face, wf), (np.nonzero(face != wf)[0][:10], face[face != wf][:10], wf[face != wf][:10])
    assert np.array_equal(t.view(np.uint64), wt.view(np.uint64)), np.nonzero(t.view(np.uint64) != wt.view(np.uint64))[0][:10]
    assert np.array_equal(bary.view(np.uint32), wb.view(np.uint32)), np.nonzero((bary.view(np.uint32) != wb.view(np.uint32)).any(axis=1))[0][:10]
    assert np.array_equal(side, ws)


def _check(o, d, v, f, keep=None, **kw):
    got = _cast(o, d, v, f, keep, **kw)
    _same(got, ref.cast(o, d, v, f, keep, **kw))
    return got


@functools.lru_cache(maxsize=None)
def _soup(F):
    return refd.heavy_tailed_soup(F, seed=F)


@functools.lru_cache(maxsize=None)
def _grid(F):
    v, f = refs.grid_mesh(max(1, int(np.ceil(np.sqrt(F / 2)))), seed=F)
    return v, f[:F]


@functools.lru_cache(maxsize=None)
def _closed():
    return ref.closed_mesh(3, seed=1)


# ---- parity ------------------------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (9, 2), (65, 63), (64, 8), (257, 9), (64, 64), (130, 65), (256, 512), (100, 513), (700, 1025), (1500, 4097)]


@pytest.mark.parametrize("cull_back", [False, True])
@pytest.mark.parametrize("kind", ["soup", "grid"])
@pytest.mark.parametrize("Q,F", SIZES)
def test_ray_cast_matches_brute_force(Q, F, kind, cull_back):
    v, f = (_soup if kind == "soup" else _grid)(F)
    assert len(f) == F
    o, d = ref.mixed_rays(Q, v, f, seed=Q + F)
    face, t, _, side, _ = _check(o, d, v, f, cull_back=cull_back)
    if Q >= 64:
        assert (face >= 0).any() and (face < 0).any()
        assert cull_back or ((side == 1).any() and (side == -1).any())


def test_every_face_repeated_and_shuffled_the_smallest_index_wins():
    v, f = _soup(64)
    which = np.random.default_rng(2).permutation(np.repeat(np.arange(64), 40))
    o, d = ref.mixed_rays(500, v, f, seed=3)
    face, _, _, _, _ = _check(o, d, v, f[which])
    first = np.array([np.nonzero(which == k)[0][0] for k in range(64)])
    assert (face >= 0).sum() > 100 and np.isin(face[face >= 0], first).all()


def test_grid_mesh_rays_through_shared_edges_and_vertices_tie_to_the_smallest_index():
    v, f = _grid(800)
    rng = np.random.default_rng(1)
    tri = v[f[rng.integers(0, len(f), 600)]]
    on_edge = (0.5 * tri[:, 0] + 0.5 * tri[:, 1]).astype(np.float32)
    target = np.concatenate([v, on_edge])
    # straight down the z axis: x and y of the ray ARE those of the vertex, so the edge functions through it are exactly 0 and every face
    # that uses the vertex is a candidate; their t' differ by roundings, the smallest wins
    o = target + np.array([0, 0, 2], np.float32)
    d = np.tile(np.array([[0, 0, -1]], np.float32), (len(o), 1))
    face, t, _, _, _ = _check(o, d, v, f)
    uses = [np.nonzero((f == k).any(axis=1))[0] for k in range(len(v))]
    assert all(face[k] in u for k, u in enumerate(uses) if len(u))
    # the same mesh pressed flat: every t' is exactly 2 (the numerator is twice the denominator), so the ties are exact -- the smallest index
    flat = v * np.array([1, 1, 0], np.float32)
    face, t, _, _, _ = _check(np.concatenate([flat[:, :2], np.full((len(v), 1), 2, np.float32)], axis=1), d[:len(v)], flat, f)
    assert all(face[k] == u.min() and t[k] == 2.0 for k, u in enumerate(uses) if len(u))
    assert sum(len(u) > 1 for u in uses) > 300
    # and from one eye, aimed at them in fp32
    eye = np.array([0.4, 0.6, 1.5], np.float32)
    _check(np.broadcast_to(eye, target.shape).copy(), target - eye, v, f)


# ---- watertightness --------------------------------------------------------------------------------------------------------------------------------
def test_no_ray_from_inside_a_closed_mesh_escapes():
    v, f = _closed()
    assert len(f) == 512
    o, d = ref.rays_from_inside(v, f, 4096, seed=21)
    tri = v[f]
    d[:len(v)] = v - o[:len(v)]                                                                           # every vertex
    d[len(v):len(v) + 512] = (0.5 * tri[:, 0] + 0.5 * tri[:, 1]).astype(np.float32) - o[len(v):len(v) + 512]  # one edge of every face
    face, t, _, side, _ = _check(o, d, v, f)
    assert (face >= 0).all() and np.isfinite(t).all() and (side == -1).all()


# ---- spoiled meshes --------------------------------------------------------------------------------------------------------------------------------
def _spoiled(F, seed):
    v, f = (a.copy() for a in _soup(F))
    rng = np.random.default_rng(seed)
    keep = (rng.random(F) < 0.93).astype(np.uint8)
    n = max(1, F // 15)
    f[rng.choice(F, n, replace=False), rng.integers(0, 3, n)] = rng.choice([-1, 3 * F, 2 ** 31 - 1, -2 ** 31], n)
    v[rng.choice(3 * F, n, replace=False), rng.integers(0, 3, n)] = rng.choice([NAN, INF, -INF], n)
    return v, f, keep


def test_ineligible_faces_are_never_returned_and_zero_area_faces_never_hit():
    v, f, keep = _spoiled(2000, 4)
    eligible = refs.eligible_faces(v, f, keep)
    assert 0.7 * 2000 < len(eligible) < 0.9 * 2000
    o, d = ref.mixed_rays(700, v, f, seed=5)
    face, _, _, _, _ = _check(o, d, v, f, keep)
    assert (face >= 0).sum() > 100 and np.isin(face[face >= 0], eligible).all()
    _check(o, d, v, f, keep.astype(bool))
    face, _, _, _, _ = _check(o, d, v, f)  # no mask: more faces are eligible
    assert not np.isin(face[face >= 0], eligible).all()
    v, f = (a.copy() for a in _soup(300))
    rng = np.random.default_rng(6)
    seg, pt = rng.choice(300, 60, replace=False), rng.choice(300, 30, replace=False)
    v[f[seg, 1]] = v[f[seg, 0]]
    v[f[pt, 1]] = v[f[pt, 2]] = v[f[pt, 0]]
    o, d = ref.mixed_rays(400, v, f, seed=7)
    eye = np.array([0.5, 0.5, 3], np.float32)
    o = np.concatenate([o, np.broadcast_to(eye, (90, 3))])
    d = np.concatenate([d, v[f[pt, 0]] - eye, (v[f[seg, 0]] * np.float32(0.25) + v[f[seg, 2]] * np.float32(0.75)) - eye])  # aimed AT them
    face, _, _, _, _ = _check(o, d, v, f)
    assert not np.isin(face, np.concatenate([seg, pt])).any() and (face >= 0).sum() > 100


def test_no_eligible_face_no_face_no_ray_and_bad_rays():
    v, f = _soup(100)
    o, d = ref.mixed_rays(70, v, f, seed=8)
    o[5, 1], o[69, 0], d[7, 2], d[8, 0] = NAN, INF, NAN, -INF
    d[9] = 0.0
    limit = np.full(70, 100.0, np.float32)
    limit[11] = NAN
    bad = np.zeros(70, bool)
    bad[[5, 69, 7, 8, 9, 11]] = True
    for vv, ff, keep in ((v, f, np.zeros(100, np.uint8)), (np.full_like(v, NAN), f, None), (v, np.zeros((0, 3), np.int32), None),
                         (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None)):
        face, t, bary, side, visits = _check(o, d, vv, ff, keep, t_limit=limit)
        assert (face == -1).all() and np.isnan(t[bad]).all() and np.isposinf(t[~bad]).all() and np.isnan(bary).all() and (side == 0).all()
        assert visits == 0
    face, t, bary, side, _ = _check(o, d, v, f, t_limit=limit)
    assert (face[bad] == -1).all() and np.isnan(t[bad]).all() and np.isnan(bary[bad]).all() and (side[bad] == 0).all() and (face[~bad] >= 0).any()
    _check(np.full((64, 3), INF, np.float32), d[:64], v, f)  # one wave, nobody alive
    q = np.tile(o[:1], (200, 1))
    dd = np.tile(d[:1], (200, 1))
    dd[:130] = 0.0  # whole waves of zero directions
    _check(q, dd, v, f)
    from diff_recon_hip import ray_cast
    empty = ray_cast((_dev(v), _dev(f)), _dev(np.zeros((0, 3), np.float32)), _dev(np.zeros((0, 3), np.float32)))
    assert empty.face.shape == (0,) and empty.t.shape == (0,) and empty.bary.shape == (0, 3) and empty.side.shape == (0,)


# ---- ranges ----------------------------------------------------------------------------------------------------------------------------------------
def test_ranges_on_two_parallel_squares_and_on_a_soup():
    v, f = ref.two_squares(0.5)
    rng = np.random.default_rng(9)
    xy = (rng.integers(1, 255, (200, 2)) / 256).astype(np.float32)
    o = np.concatenate([xy, np.full((200, 1), -2.0, np.float32)], axis=1)
    d = np.tile(np.array([[0, 0, 1]], np.float32), (200, 1))
    face, t, _, side, _ = _check(o, d, v, f)
    assert (t == 2.0).all() and np.isin(face, (0, 1)).all() and (side == -1).all()
    face, t, _, _, _ = _check(o, d, v, f, tmin=2.25)  # skips the nearer square and finds the next
    assert (t == 2.5).all() and np.isin(face, (2, 3)).all()
    face, t, _, _, _ = _check(o, d, v, f, tmin=2.0, tmax=2.0)
    assert (t == 2.0).all()
    face, t, _, _, _ = _check(o, d, v, f, tmin=2.125, tmax=2.375)
    assert (face == -1).all() and np.isposinf(t).all()
    face, t, _, _, _ = _check(o, d, v, f, tmax=1.5)
    assert (face == -1).all()
    limit = np.where(np.arange(200) % 2 == 0, 1.999, 2.0).astype(np.float32)
    limit[7], limit[9] = NAN, INF
    face, t, _, _, _ = _check(o, d, v, f, t_limit=limit, tmax=2.25)
    assert np.isnan(t[7]) and t[9] == 2.0 and (face[::2] == -1).all() and (t[1::2][np.arange(1, 200, 2) != 7] == 2.0).all()
    face, t, _, side, _ = _check(o + np.array([0, 0, 4], np.float32), -d, v, f, cull_back=True)
    assert (t == 1.5).all() and (side == 1).all()
    face, t, _, side, _ = _check(o, d, v, f, cull_back=True)  # both squares show these rays their backs
    assert (face == -1).all()
    v, f = _soup(1025)
    o, d = ref.mixed_rays(700, v, f, seed=10)
    base = _check(o, d, v, f)
    hit = base[0] >= 0
    tmin = float(np.median(base[1][hit]))
    later = _check(o, d, v, f, tmin=tmin)
    moved = hit & (base[1] < tmin)
    assert moved.sum() > 50 and (later[0][moved] != base[0][moved]).all() and (later[0][moved] >= 0).any() and (later[1][moved] >= tmin).all()
    nearer = _check(o, d, v, f, tmax=tmin)
    assert np.array_equal(nearer[0][hit & (base[1] <= tmin)], base[0][hit & (base[1] <= tmin)]) and (nearer[0][hit & (base[1] > tmin)] == -1).all()
    limit = np.where(np.arange(700) % 3 == 0, tmin, INF).astype(np.float32)
    _check(o, d, v, f, t_limit=limit, tmin=0.125 * tmin, tmax=4 * tmin)


def test_coordinates_at_the_fp32_range():
    rng = np.random.default_rng(12)
    v = (rng.uniform(-1, 1, (600, 3)) * 3e38).astype(np.float32)
    f = rng.integers(0, 600, (900, 3)).astype(np.int32)
    o = (rng.uniform(-1, 1, (500, 3)) * 3e38).astype(np.float32)
    o[::5] = v[rng.integers(0, 600, 100)]
    d = rng.normal(size=(500, 3)).astype(np.float32)
    d[1::4] = (v[rng.integers(0, 600, 125)].astype(np.float64) * 0.5 - o[1::4].astype(np.float64) * 0.5).astype(np.float32)
    d[2::4] *= np.float32(1e-45)  # the smallest subnormal, or zero
    d[3::8] = np.float32(1e-45) * np.sign(d[3::8])
    assert (np.abs(d[np.isfinite(d)]) == np.float32(1e-45)).sum() > 100
    face, t, bary, _, _ = _check(o, d, v, f)
    good = ~ref.bad_rays(o, d)
    assert (face >= 0).sum() > 50 and not np.isnan(t[good]).any() and np.isfinite(t[face >= 0]).all() and np.isfinite(bary[face >= 0]).all()
    assert t[face >= 0].max() > float(np.finfo(np.float32).max)  # distances in units of d that fp32 could not hold


# ---- purity, determinism ------------------------------------------------------------------------------------------------------------------------------
def test_cast_is_pure_and_permuting_the_rays_permutes_the_results():
    from diff_recon_hip import MeshBVH, ray_cast
    v, f, keep = _spoiled(1025, 13)
    o, d = ref.mixed_rays(700, v, f, seed=14)
    o[3, 2], d[4, 1] = NAN, INF
    limit = np.where(np.arange(700) % 5 == 0, 0.5, INF).astype(np.float32)
    gv, gf, gk, go, gd, gl = _dev(v), _dev(f), _dev(keep), _dev(o), _dev(d), _dev(limit)

    def call(pattern):  # the index, both workspaces and the four outputs come from torch.empty: all poisoned
        visits = torch.zeros(1, device=DEV, dtype=torch.int64)
        hits = ray_cast(MeshBVH(gv, gf, gk), go, gd, t_limit=gl, cull_back=True, leaf_visits=visits)
        return {"face": hits.face, "t": hits.t, "bary": hits.bary, "side": hits.side, "visits": int(visits.item())}

    base = poison.assert_pure(call)
    want = ref.cast(o, d, v, f, keep, t_limit=limit, cull_back=True)
    got = (base["face"].numpy().view(np.int32), base["t"].numpy().view(np.float64), base["bary"].numpy().view(np.float32).reshape(-1, 3),
           base["side"].numpy().view(np.int8))
    _same(got, want)
    perm = np.random.default_rng(15).permutation(700)
    _same(_cast(o[perm], d[perm], v, f, keep, t_limit=limit[perm], cull_back=True), tuple(w[perm] for w in want))


def test_bary_and_side_may_be_null_through_the_c_abi():
    from diff_recon_hip import MeshBVH, mesh_ray
    from diff_triangle_rasterization_2D import _C as native
    lib = mesh_ray._lib
    v, f = _soup(513)
    o, d = ref.mixed_rays(300, v, f, seed=16)
    want = ref.cast(o, d, v, f)
    bvh = MeshBVH(_dev(v), _dev(f))
    go, gd = _dev(o), _dev(d)
    for with_bary, with_side in ((False, False), (True, False), (False, True)):
        with poison.PoisonedEmpty("nan") as pe:
            face, t = torch.empty(300, device=DEV, dtype=torch.int32), torch.empty(300, device=DEV, dtype=torch.float64)
            bary, side = torch.empty((300, 3), device=DEV, dtype=torch.float32), torch.empty(300, device=DEV, dtype=torch.int8)
            ws = torch.empty(lib.tsr_cast_workspace_bytes(300), device=DEV, dtype=torch.uint8)
            rc = lib.tsr_cast(300, go.data_ptr(), gd.data_ptr(), None, 0.0, float("inf"), 0, 513, bvh.bvh.data_ptr(), bvh.bvh.numel(), face.data_ptr(),
                              t.data_ptr(), bary.data_ptr() if with_bary else None, side.data_ptr() if with_side else None, None, ws.data_ptr(),
                              ws.numel(), native.stream())
            assert rc == 0, lib.tsr_last_error()
            torch.cuda.synchronize()
            pe.check_guards()
        assert np.array_equal(face.cpu().numpy(), want[0]) and np.array_equal(t.cpu().numpy().view(np.uint64), want[1].view(np.uint64))
        if with_bary:
            assert np.array_equal(bary.cpu().numpy().view(np.uint32), want[2].view(np.uint32))
        else:
            assert (bary.cpu().numpy().view(np.uint32) == 0x7FC00000).all()  # untouched: still the poison
        if with_side:
            assert np.array_equal(side.cpu().numpy(), want[3])


# ---- pruning ------------------------------------------------------------------------------------------------------------------------------------------
class Cam:
    """The duck-typed camera of MeshRenderer: looks from `eye` at `target`, row-vector world_view_transform."""

    def __init__(self, W, H, eye, target, tan_fov):
        eye, target = np.array(eye, np.float64), np.array(target, np.float64)
        fwd = (target - eye) / np.linalg.norm(target - eye)
        right = np.cross([0.0, 1.0, 0.0], fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        view = np.eye(4)
        view[:3, :3] = np.stack([right, down, fwd], axis=1)
        view[3, :3] = -eye @ view[:3, :3]
        self.device = "cuda:0"
        self.image_width, self.image_height = W, H
        self.tan_fovx, self.tan_fovy = tan_fov, tan_fov * H / W
        self.world_view_transform = torch.from_numpy(view.astype(np.float32)).to(self.device)


def test_the_hierarchy_prunes_camera_rays():
    from diff_recon_hip import MeshBVH, camera_rays
    v, f = refs.small_triangle_soup(16384, seed=16)
    cam = Cam(128, 128, (0.3, 0.2, -2.0), (0.5, 0.5, 0.5), 0.3)
    o, d = camera_rays(cam)
    assert o.shape == d.shape == (16384, 3) and o.dtype == d.dtype == torch.float32
    visits = torch.zeros(1, device=DEV, dtype=torch.int64)
    hits = MeshBVH(_dev(v), _dev(f)).ray_cast(o, d, leaf_visits=visits)
    waves, leaves = 16384 // 64, 16384 // LEAF
    n = int(visits.item())
    share = float((hits.face >= 0).float().mean())
    print(f"16384 camera rays on 16384 small triangles: {n} leaf visits = {n / waves:.1f} per wave, brute force {waves * leaves}; hit share {share:.3f}")
    assert n < waves * leaves // 2
    assert 0.02 < share < 0.95  # the view is neither empty nor full: the walk has both hits and misses to prune for
    sub = np.arange(0, 16384, 16)
    want = ref.cast(o.cpu().numpy()[sub], d.cpu().numpy()[sub], v, f)
    _same((hits.face.cpu().numpy()[sub], hits.t.cpu().numpy()[sub], hits.bary.cpu().numpy()[sub], hits.side.cpu().numpy()[sub]), want)


# ---- camera_rays against MeshRenderer -----------------------------------------------------------------------------------------------------------------
TRIANGLES = np.array([[[-1.3, -1.2, 1.0], [1.5, -1.1, 1.6], [0.2, 0.9, 0.4]],
                      [[-1.3, -0.6, -0.6], [-0.3, 0.1, -0.2], [-1.2, 1.3, 0.1]],
                      [[0.3, -0.2, -1.0], [0.9, 0.1, -0.7], [0.45, 0.75, -1.2]],
                      [[0.3, 1.0, -0.3], [1.3, 0.2, 0.1], [1.2, 1.3, -0.6]]], np.float32)


def _segment_distance(p, a, b):
    ab = b - a
    s = np.clip(((p - a) @ ab) / (ab @ ab), 0.0, 1.0)
    return np.linalg.norm(p - (a + s[:, None] * ab), axis=1)


def test_camera_rays_agree_with_the_mesh_renderer():
    from diff_recon_hip import MeshRenderer, camera_rays, ray_cast
    W = H = 64
    cam = Cam(W, H, (0.5, 0.25, -3.0), (0.1, 0.0, 0.5), 0.42)
    v, f = TRIANGLES.reshape(-1, 3), np.arange(12, dtype=np.int32).reshape(4, 3)
    # the triangles do not touch: every vertex of one is well away from the surface of the others
    for k in range(4):
        others = np.delete(np.arange(4), k)
        w = np.array([(a, b, 6 - a - b) for a in range(7) for b in range(7 - a)], np.float32) / 6
        _, d2, _ = refs.closest((w @ TRIANGLES[k]).astype(np.float32), v, f[others])
        assert d2.min() > 0.1 ** 2, (k, d2.min())
    out = MeshRenderer(cam).render(_dev(v), _dev(f), _dev(np.ones((4, 3), np.float32)))
    o, d = camera_rays(cam)
    hits = ray_cast((_dev(v), _dev(f)), o, d)
    face_idx, depth = out["face_idx"].cpu().numpy().reshape(-1), out["depth"].cpu().numpy().reshape(-1).astype(np.float64)
    face, t = hits.face.cpu().numpy(), hits.t.cpu().numpy()
    # the pixels within one pixel of a projected edge, from the float64 projection of the vertices
    view = cam.world_view_transform.cpu().numpy().astype(np.float64)
    pv = v.astype(np.float64) @ view[:3, :3] + view[3, :3]
    assert pv[:, 2].min() > 1.0  # beyond znear: every face is drawn
    s = np.stack([(pv[:, 0] / (pv[:, 2] * cam.tan_fovx) + 1) * W / 2, (pv[:, 1] / (pv[:, 2] * cam.tan_fovy) + 1) * H / 2], axis=1).reshape(4, 3, 2)
    px = np.stack(np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5), axis=-1).reshape(-1, 2)
    near = np.zeros(W * H, bool)
    for tri in s:
        for k in range(3):
            near |= _segment_distance(px, tri[k], tri[(k + 1) % 3]) <= 1.0
    covered = face_idx >= 0
    left_out = covered & near
    print(f"covered pixels {covered.sum()}, within one pixel of an edge {left_out.sum()} ({left_out.sum() / covered.sum():.3f}); faces seen {np.unique(face_idx[covered])}")
    assert covered.sum() > 1500 and left_out.sum() < covered.sum() / 4 and set(np.unique(face_idx[covered])) == {0, 1, 2, 3}
    clear = ~near
    assert np.array_equal(face[clear], face_idx[clear]), np.nonzero(face[clear] != face_idx[clear])[0][:10]
    both = clear & covered
    err = np.abs(t[both] - depth[both]) / depth[both]
    print(f"|t - depth| / depth over {both.sum()} pixels: max {err.max() / 2.0 ** -24:.2f} x 2^-24")
    assert (err <= 8 * 2.0 ** -24).all()
    assert np.isposinf(t[clear & ~covered]).all()


# ---- point_visibility and the scores ----------------------------------------------------------------------------------------------------------------------
def test_point_visibility_two_parallel_squares():
    from diff_recon_hip import point_visibility, sample_mesh_surface
    v, f = ref.two_squares(0.5)
    v = v.copy()
    v[:4, :2] = v[:4, :2] * np.float32(0.5) + np.float32(0.25)  # the near square (z = 0) is the smaller one: it hides the middle of the far one
    centre = np.array([[0.5, 0.5, -1000.0]], np.float32)     # far away: the shadow of the near square is all but its own outline
    gv, gf = _dev(v), _dev(f)
    keep_far = _dev(np.array([0, 0, 1, 1], np.uint8))
    far = sample_mesh_surface(gv, gf, 2000, seed=3, keep=keep_far).points
    near = sample_mesh_surface(gv, gf, 500, seed=4, keep=_dev(np.array([1, 1, 0, 0], np.uint8))).points
    seen_far = point_visibility((gv, gf), far, _dev(centre)).cpu().numpy()
    seen_near = point_visibility((gv, gf), near, _dev(centre)).cpu().numpy()
    assert seen_far.dtype == np.int32 and (seen_near == 1).all()
    xy = far.cpu().numpy()[:, :2].astype(np.float64)
    margin = np.abs(xy - 0.5).max(axis=1) - 0.25  # < 0: behind the near square, as the centre sees it (up to the perspective of 1 in 2000)
    sure = np.abs(margin) > 1e-3
    assert np.array_equal(seen_far[sure], (margin[sure] > 0).astype(np.int32)) and (margin[sure] < 0).sum() > 300
    assert np.array_equal(seen_far, ref.visibility(far.cpu().numpy(), centre, v, f))
    assert np.array_equal(seen_near, ref.visibility(near.cpu().numpy(), centre, v, f))


def _cube(h):
    """The cube [-h, h]^3: eight vertices, twelve outward counter-clockwise faces.  For h a power of two the sampler's points lie exactly on it."""
    v = np.array(list(itertools.product((-h, h), repeat=3)), np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)


@functools.lru_cache(maxsize=None)
def _nested():
    """A small closed mesh inside a larger one, and 14 centres outside both: on the axes and on the diagonals, 4 from the middle."""
    (vo, fo), (vi, fi) = _cube(1.0), _cube(0.25)
    centres = np.array([4.0 * np.array(p) / np.linalg.norm(p) for p in itertools.product((-1, 0, 1), repeat=3) if sum(map(abs, p)) in (1, 3)], np.float32)
    return (vo, fo), (np.concatenate([vo, vi]), np.concatenate([fo, fi + len(vo)]).astype(np.int32)), centres


def test_a_mesh_buried_inside_another_is_hidden_and_stops_counting():
    from diff_recon_hip import mesh_surface_distance, point_visibility, sample_mesh_surface
    (vo, fo), (vc, fc), centres = _nested()
    assert len(centres) == 14
    outer, both, gc = (_dev(vo), _dev(fo)), (_dev(vc), _dev(fc)), _dev(centres)
    sa = sample_mesh_surface(*both, 2000, seed=0)
    inner = sa.face.cpu().numpy() >= len(fo)
    assert 50 < inner.sum() < 500  # by area: one sample in seventeen
    seen = point_visibility(both, sa.points, gc).cpu().numpy()
    assert (seen[inner] == 0).all() and (seen[~inner] >= 1).all()
    assert np.array_equal(seen, ref.visibility(sa.points.cpu().numpy(), centres, vc, fc))
    res = mesh_surface_distance(both, outer, 2000, seed=0, thresholds=[0.01], visible_from=gc)
    plain = mesh_surface_distance(both, outer, 2000, seed=0, thresholds=[0.01])
    print(f"inner samples {inner.sum()}: accuracy {plain['accuracy']:.4g} -> {res['accuracy']:.4g}, precision {plain['precision']} -> {res['precision']}")
    assert res["a_hidden"] == int(inner.sum()) and res["a_count"] == 2000 - int(inner.sum()) and res["b_hidden"] == 0 and res["b_count"] == 2000
    assert res["accuracy"] == 0.0 and res["precision"] == [1.0] and plain["accuracy"] > 0 and plain["precision"][0] < 1.0
    assert "a_hidden" not in plain and set(res) == set(plain) | {"a_hidden", "b_hidden"}


def test_without_centres_the_scores_are_what_they_were():
    """mesh_surface_distance(visible_from=None) against the computation it replaced, written out: key for key, bit for bit."""
    from diff_recon_hip import MeshBVH, mesh_surface_distance, sample_mesh_surface
    from diff_recon_hip import mesh_surface as ms
    va, fa = _grid(800)
    vb, fb = refs.grid_mesh(17, seed=99)
    a, b = (_dev(va), _dev(fa)), (_dev(vb + np.float32(0.01)), _dev(fb))
    thresholds = [0.005, 0.02, 0.1]
    got = mesh_surface_distance(a, b, 3000, seed=5, thresholds=thresholds)
    assert got == mesh_surface_distance(a, b, 3000, seed=5, thresholds=thresholds, visible_from=None)
    sa, sb = sample_mesh_surface(*a, 3000, 5), sample_mesh_surface(*b, 3000, 6)
    face_ab, d2_ab, _ = MeshBVH(*b).closest(sa.points)
    face_ba, d2_ba, _ = MeshBVH(*a).closest(sb.points)
    sq_a, da, a_dropped = ms._one_way(d2_ab, face_ab)
    sq_b, db, b_dropped = ms._one_way(d2_ba, face_ba)
    acc, comp = ms._mean(da), ms._mean(db)
    want = {"accuracy": acc, "completeness": comp, "chamfer": (acc + comp) / 2, "chamfer_sq": ms._mean(sq_a) + ms._mean(sq_b),
            "hausdorff": max(float(da.max().item()), float(db.max().item())), "a_count": 3000, "b_count": 3000, "a_dropped": 0, "b_dropped": 0,
            "thresholds": thresholds, "area_a": sa.area, "area_b": sb.area,
            "a_within": [int((da <= tau).sum().item()) for tau in thresholds], "b_within": [int((db <= tau).sum().item()) for tau in thresholds]}
    want["precision"], want["recall"] = [n / 3000 for n in want["a_within"]], [n / 3000 for n in want["b_within"]]
    want["fscore"] = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(want["precision"], want["recall"])]
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
    fwant = refs.scores(*refs.closest(sa.points.cpu().numpy(), vb + np.float32(0.01), fb)[:2], *refs.closest(sb.points.cpu().numpy(), va, fa)[:2], thresholds)
    assert np.allclose(got["accuracy"], fwant["accuracy"], rtol=1e-12, atol=0) and got["a_within"] == fwant["a_within"]


# ---- example ------------------------------------------------------------------------------------------------------------------------------------------
def test_example_reports_visible_surface_scores():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    s = train_synthetic.mesh_scores(m, "2D", surface=2000, visible=True, **cfg)["surface"]
    lines = train_synthetic.geometry_report(s, title="mesh surface")
    print("\n".join(lines))
    for k in ("accuracy", "completeness", "chamfer", "chamfer_sq", "hausdorff", "area_a", "area_b", "median_edge"):
        assert np.isfinite(s[k]) and s[k] > 0, k
    assert s["a_hidden"] + s["a_count"] == 2000 and s["b_hidden"] + s["b_count"] == 2000 and s["a_dropped"] == s["b_dropped"] == 0
    assert len(lines) == 4 and "hidden" in lines[3] and str(s["a_hidden"]) in lines[3]
    plain = train_synthetic.mesh_scores(m, "2D", surface=2000, **cfg)["surface"]
    assert "a_hidden" not in plain and plain["a_count"] == 2000 and len(train_synthetic.geometry_report(plain, title="mesh surface")) == 3
