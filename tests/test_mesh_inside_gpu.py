"""GPU tests of the inside test and the signed distance of a mesh against tests/ref_mesh_inside.py: ray_crossings returns the brute-force
counts -- hits, half crossings and touches bit for bit -- on every boundary of the structure (leaves of 8 faces, fan-out 8; waves of 64 rays,
workgroups of 256), with per-ray and shared directions; it is pure, does not depend on the order of rays or faces and agrees with ray_cast on
who hits nothing; signed_distance, contains_points, mesh_to_sdf, remesh and mesh_volume_iou on known answers; the example's report."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import poison
import ref_mesh_distance as refd
import ref_mesh_inside as ref
import ref_mesh_ray as refr
import ref_mesh_surface as refs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = np.float32(np.nan), np.float32(np.inf)
LEAF = 8  # faces per leaf (csrc/ts_bvh_layout.h)
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cross(o, d, v, f, keep=None, **kw):
    from diff_recon_hip import MeshBVH, RayCrossings, ray_crossings
    visits = torch.zeros(1, device=DEV, dtype=torch.int64)
    if kw.get("t_limit") is not None:
        kw = dict(kw, t_limit=_dev(kw["t_limit"]))
    c = ray_crossings(MeshBVH(_dev(v), _dev(f), None if keep is None else _dev(keep)), _dev(o), _dev(np.asarray(d, np.float32)), leaf_visits=visits, **kw)
    assert isinstance(c, RayCrossings)
    assert c.hits.dtype == c.winding2.dtype == c.touches.dtype == torch.int32 and c.hits.shape == c.winding2.shape == c.touches.shape == (len(o),)
    return c.hits.cpu().numpy(), c.winding2.cpu().numpy(), c.touches.cpu().numpy(), int(visits.item())


def _same(got, want):
    for name, g, w in zip(("hits", "winding2", "touches"), got[:3], want):
        assert np.array_equal(g, w), (name, np.nonzero(g != w)[0][:10], g[g != w][:10], w[g != w][:10])


def _check(o, d, v, f, keep=None, **kw):
    got = _cross(o, d, v, f, keep, **kw)
    _same(got, ref.crossings(o, d, v, f, keep, **kw))
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
    return refr.closed_mesh(3, seed=1)


# ---- parity ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 8, 9, 65, 600])  # one leaf; one full leaf; two leaves; two levels; four levels (75 -> 10 -> 2 -> 1)
@pytest.mark.parametrize("Q", [1, 63, 65, 1000])
def test_crossings_match_brute_force(Q, F):
    total = 0
    for kind in (_soup, _grid):
        v, f = kind(F)
        assert len(f) == F
        o, d = refr.mixed_rays(Q, v, f, seed=Q + F)
        hits, _, _, _ = _check(o, d, v, f)                       # a direction per ray
        total += int((hits > 0).sum())
        _check(o, ref.DIRECTIONS[(Q + F) % 3], v, f)             # one direction for all
        _check(o, d[Q // 2], v, f)                               # a shared direction aimed at something
    assert Q < 64 or total > 0


def test_grid_mesh_rays_through_shared_edges_and_vertices():
    v, f = _grid(600)
    rng = np.random.default_rng(1)
    tri = v[f[rng.integers(0, len(f), 500)]]
    on_edge = (0.5 * tri[:, 0] + 0.5 * tri[:, 1]).astype(np.float32)
    inner = (tri.astype(np.float64).mean(axis=1)).astype(np.float32)
    target = np.concatenate([v, on_edge, inner])
    # straight down the z axis: x and y of the ray ARE those of the vertex, so the edge functions through it are exactly 0
    o = target + np.array([0, 0, 2], np.float32)
    hits, w2, touches, _ = _check(o, np.array([0, 0, -1], np.float32), v, f)
    nv = len(v)
    uses = np.array([(f == k).any(axis=1).sum() for k in range(nv)])
    assert np.array_equal(touches[:nv], uses) and np.array_equal(hits[:nv], uses) and (w2[:nv] == 0).all() and (uses > 1).sum() > 200
    through_edge = (touches == 0) & (hits == 2)
    assert through_edge[nv:nv + 500].sum() > 100 and (np.abs(w2[through_edge]) == 2).all()   # two halves on equal sides: one crossing
    boundary = (touches == 0) & (hits == 1) & (np.abs(w2) == 1)
    assert boundary[nv:nv + 500].sum() > 0                                                   # the rim of the open mesh: odd
    assert ((hits[nv + 500:] == 1) & (np.abs(w2[nv + 500:]) == 2)).sum() > 400               # face interiors
    _check(o, np.tile(np.array([[0, 0, -1]], np.float32), (len(o), 1)), v, f)
    eye = np.array([0.4, 0.6, 1.5], np.float32)  # and from one eye, aimed at them in fp32
    _check(np.broadcast_to(eye, target.shape).copy(), target - eye, v, f)


def test_closed_mesh_every_clean_ray_from_inside_leaves_once():
    v, f = _closed()
    assert len(f) == 512
    o, d = refr.rays_from_inside(v, f, 1000, seed=21)
    tri = v[f]
    d[:len(v)] = v - o[:len(v)]                                                                             # every vertex
    d[len(v):len(v) + 512] = (0.5 * tri[:, 0] + 0.5 * tri[:, 1]).astype(np.float32) - o[len(v):len(v) + 512]  # one edge of every face
    hits, w2, touches, _ = _check(o, d, v, f)
    good = ~refr.bad_rays(o, d)
    assert (hits[good] >= 1).all()
    clean = ref.clean(hits, w2, touches)
    assert clean.sum() > 900 and (w2[clean] == -2).all()  # aimed at a vertex in fp32 a ray all but never meets it exactly: nearly all are clean
    for k in range(3):  # the inside test's own rays, from inside and from outside
        p = np.concatenate([o, o * np.float32(8)])
        hits, w2, touches, _ = _check(p, ref.DIRECTIONS[k], v, f)
        assert ref.clean(hits, w2, touches).all() and (w2[:1000] == -2).all() and (w2[1000:][np.linalg.norm(p[1000:], axis=1) > 1.3] == 0).all()


# ---- ranges ----------------------------------------------------------------------------------------------------------------------------------------
def test_ranges_on_nested_cubes_and_on_a_soup():
    v, f = ref.join(ref.cube(), ref.cube(0.5))
    rng = np.random.default_rng(9)
    yz = (rng.integers(-100, 100, (200, 2)) / 256).astype(np.float32)
    o = np.concatenate([np.full((200, 1), -3.0, np.float32), yz], axis=1)
    d = np.array([1, 0, 0], np.float32)
    hits, w2, _, _ = _check(o, d, v, f)
    assert (hits >= 4).all() and (w2 == 0).all()
    hits, w2, _, _ = _check(o, d, v, f, tmax=3.0)
    assert (w2 == 4).all()
    hits, w2, _, _ = _check(o, d, v, f, tmin=3.0)
    assert (w2 == -4).all()
    hits, w2, _, _ = _check(o, d, v, f, tmin=2.0, tmax=2.0)
    assert (w2 == 2).all()
    limit = np.where(np.arange(200) % 2 == 0, 2.25, 3.75).astype(np.float32)
    limit[7], limit[9] = NAN, INF
    hits, w2, _, _ = _check(o, d, v, f, t_limit=limit, tmax=5.0)
    assert hits[7] == -1 and w2[9] == 0 and (w2[::2] == 2).all() and (np.delete(w2[1::2], [3, 4]) == 2).all()
    v, f = _soup(600)
    o, d = refr.mixed_rays(1000, v, f, seed=10)
    base = _check(o, d, v, f)
    t = refr.cast(o, d, v, f)[1]
    tmid = float(np.median(t[np.isfinite(t)]))
    later, nearer = _check(o, d, v, f, tmin=tmid), _check(o, d, v, f, tmax=tmid)
    assert (later[0] <= base[0]).all() and (later[0] < base[0]).sum() > 50 and (nearer[0] < base[0]).sum() > 50
    limit = np.where(np.arange(1000) % 3 == 0, tmid, INF).astype(np.float32)
    _check(o, d, v, f, t_limit=limit, tmin=0.125 * tmid, tmax=4 * tmid)
    _check(o, ref.DIRECTIONS[0], v, f, t_limit=limit, tmin=0.125 * tmid, tmax=4 * tmid)


# ---- spoiled meshes, bad rays ----------------------------------------------------------------------------------------------------------------------
def _spoiled(F, seed):
    v, f = (a.copy() for a in _soup(F))
    rng = np.random.default_rng(seed)
    keep = (rng.random(F) < 0.93).astype(np.uint8)
    n = max(1, F // 15)
    f[rng.choice(F, n, replace=False), rng.integers(0, 3, n)] = rng.choice([-1, 3 * F, 2 ** 31 - 1, -2 ** 31], n)
    v[rng.choice(3 * F, n, replace=False), rng.integers(0, 3, n)] = rng.choice([NAN, INF, -INF], n)
    return v, f, keep


def test_ineligible_and_zero_area_faces_are_never_counted():
    v, f, keep = _spoiled(600, 4)
    o, d = refr.mixed_rays(700, v, f, seed=5)
    with_mask = _check(o, d, v, f, keep)
    _check(o, d, v, f, keep.astype(bool))
    without = _check(o, d, v, f)
    assert (without[0] >= with_mask[0]).all() and (without[0] > with_mask[0]).any()
    v, f = (a.copy() for a in _soup(300))
    rng = np.random.default_rng(6)
    seg, pt = rng.choice(300, 60, replace=False), rng.choice(300, 30, replace=False)
    v[f[seg, 1]] = v[f[seg, 0]]
    v[f[pt, 1]] = v[f[pt, 2]] = v[f[pt, 0]]
    eye = np.array([0.5, 0.5, 3], np.float32)
    o = np.broadcast_to(eye, (90, 3)).copy()
    d = np.concatenate([v[f[pt, 0]] - eye, (v[f[seg, 0]] * np.float32(0.25) + v[f[seg, 2]] * np.float32(0.75)) - eye])  # aimed AT them
    got = _check(o, d, v, f)
    alive = np.ones(300, np.uint8)
    alive[seg], alive[pt] = 0, 0
    _same(_cross(o, d, v, f, alive), got[:3])  # with the degenerate faces masked out nothing changes: they were never counted


def test_no_eligible_face_no_face_no_ray_and_bad_rays():
    v, f = _soup(100)
    o, d = refr.mixed_rays(70, v, f, seed=8)
    o[5, 1], o[69, 0], d[7, 2], d[8, 0] = NAN, INF, NAN, -INF
    d[9] = 0.0
    limit = np.full(70, 100.0, np.float32)
    limit[11] = NAN
    bad = np.zeros(70, bool)
    bad[[5, 69, 7, 8, 9, 11]] = True
    for vv, ff, keep in ((v, f, np.zeros(100, np.uint8)), (np.full_like(v, NAN), f, None), (v, np.zeros((0, 3), np.int32), None),
                         (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None)):
        hits, w2, touches, visits = _check(o, d, vv, ff, keep, t_limit=limit)
        assert (hits[bad] == -1).all() and (hits[~bad] == 0).all() and (w2 == 0).all() and (touches == 0).all() and visits == 0
        hits, _, _, _ = _check(o, ref.DIRECTIONS[0], vv, ff, keep, t_limit=limit)
        assert (hits == np.where(np.isin(np.arange(70), [5, 69, 11]), -1, 0)).all()
        for shared_bad in ([0, 0, 0], [NAN, 0, 1], [1, INF, 0]):  # a bad shared direction makes every ray bad
            hits, _, _, _ = _check(o, np.array(shared_bad, np.float32), vv, ff, keep)
            assert (hits == -1).all()
    hits, w2, touches, _ = _check(o, d, v, f, t_limit=limit)
    assert (hits[bad] == -1).all() and (w2[bad] == 0).all() and (touches[bad] == 0).all() and (hits[~bad] > 0).any()
    hits, _, _, _ = _check(o, np.zeros(3, np.float32), v, f)
    assert (hits == -1).all()
    _check(np.full((64, 3), INF, np.float32), d[:64], v, f)  # one wave, nobody alive
    q, dd = np.tile(o[:1], (200, 1)), np.tile(d[:1], (200, 1))
    dd[:130] = 0.0  # whole waves of zero directions
    _check(q, dd, v, f)
    from diff_recon_hip import ray_crossings
    empty = ray_crossings((_dev(v), _dev(f)), _dev(np.zeros((0, 3), np.float32)), _dev(np.zeros((0, 3), np.float32)))
    assert empty.hits.shape == empty.winding2.shape == empty.touches.shape == (0,)
    empty = ray_crossings((_dev(v), _dev(f)), _dev(np.zeros((0, 3), np.float32)), _dev(ref.DIRECTIONS[0]))
    assert empty.hits.shape == (0,)


def test_coordinates_at_the_fp32_range():
    rng = np.random.default_rng(12)
    v = (rng.uniform(-1, 1, (400, 3)) * 3e38).astype(np.float32)
    f = rng.integers(0, 400, (600, 3)).astype(np.int32)
    o = (rng.uniform(-1, 1, (500, 3)) * 3e38).astype(np.float32)
    o[::5] = v[rng.integers(0, 400, 100)]
    d = rng.normal(size=(500, 3)).astype(np.float32)
    d[1::4] = (v[rng.integers(0, 400, 125)].astype(np.float64) * 0.5 - o[1::4].astype(np.float64) * 0.5).astype(np.float32)
    d[2::4] *= np.float32(1e-45)  # the smallest subnormal, or zero
    d[3::8] = np.float32(1e-45) * np.sign(d[3::8])
    hits, _, _, _ = _check(o, d, v, f)
    assert (hits > 0).sum() > 50 and (hits > 1).sum() > 5
    _check(o, np.array([1e-45, -1e-45, 0], np.float32), v, f)
    _check(o, np.array([3e38, -1e38, 2e38], np.float32), v, f)


# ---- purity, invariants -------------------------------------------------------------------------------------------------------------------------------
def test_crossings_and_signed_distance_are_pure_and_permutations_do_what_they_should():
    from diff_recon_hip import MeshBVH, ray_crossings, signed_distance
    v, f, keep = _spoiled(600, 13)
    o, d = refr.mixed_rays(700, v, f, seed=14)
    o[3, 2], d[4, 1] = NAN, INF
    limit = np.where(np.arange(700) % 5 == 0, 0.5, INF).astype(np.float32)
    gv, gf, gk, go, gd, gl = _dev(v), _dev(f), _dev(keep), _dev(o), _dev(d), _dev(limit)
    cv, cf = _closed()
    gcv, gcf = _dev(cv), _dev(cf)
    pts = np.random.default_rng(3).uniform(-1.3, 1.3, (300, 3)).astype(np.float32)
    pts[:40] = cv[:40]  # on the mesh: no clean ray, the distance decides
    gp = _dev(pts)

    def call(pattern):  # the index, the workspaces and all outputs come from torch.empty: all poisoned
        visits = torch.zeros(1, device=DEV, dtype=torch.int64)
        c = ray_crossings(MeshBVH(gv, gf, gk), go, gd, t_limit=gl, leaf_visits=visits)
        s = ray_crossings(MeshBVH(gv, gf, gk), go, gd[17], tmin=0.01)
        sdf, face, decided = signed_distance(gp, (gcv, gcf), rule="odd")
        return {"hits": c.hits, "winding2": c.winding2, "touches": c.touches, "visits": int(visits.item()), "shits": s.hits, "swinding2": s.winding2,
                "stouches": s.touches, "sdf": sdf, "face": face, "decided": decided}

    base = poison.assert_pure(call)
    want = ref.crossings(o, d, v, f, keep, t_limit=limit)
    _same(tuple(base[k].numpy().view(np.int32) for k in ("hits", "winding2", "touches")), want)
    _same(tuple(base[k].numpy().view(np.int32) for k in ("shits", "swinding2", "stouches")), ref.crossings(o, d[17], v, f, keep, tmin=0.01))
    wsdf, wface, wdec = ref.signed_distance(pts, cv, cf, rule="odd")
    assert np.array_equal(base["sdf"].numpy().view(np.uint32), wsdf.view(np.uint32)) and np.array_equal(base["face"].numpy().view(np.int32), wface)
    assert np.array_equal(base["decided"].numpy().view(bool), wdec)
    perm = np.random.default_rng(15).permutation(700)
    _same(_cross(o[perm], d[perm], v, f, keep, t_limit=limit[perm]), tuple(w[perm] for w in want))  # permuting the rays permutes the results
    fperm = np.random.default_rng(16).permutation(600)
    _same(_cross(o, d, v, f[fperm], keep[fperm], t_limit=limit), want)                              # permuting the faces changes nothing


def test_nobody_is_hit_exactly_where_ray_cast_finds_no_face():
    from diff_recon_hip import MeshBVH
    v, f = _soup(600)
    o, d = refr.mixed_rays(1000, v, f, seed=17)
    bvh = MeshBVH(_dev(v), _dev(f))
    for kw in ({}, {"tmin": 0.05, "tmax": 0.6}):
        first = bvh.ray_cast(_dev(o), _dev(d), **kw)
        c = bvh.ray_crossings(_dev(o), _dev(d), **kw)
        good = c.hits >= 0
        assert torch.equal((c.hits == 0)[good], (first.face < 0)[good]) and torch.equal(~good, torch.isnan(first.t))
        assert int((c.hits == 0).sum()) > 50 and int((c.hits > 1).sum()) > 50


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
        self.image_width, self.image_height = W, H
        self.tan_fovx, self.tan_fovy = tan_fov, tan_fov * H / W
        self.world_view_transform = torch.from_numpy(view.astype(np.float32)).to("cuda:0")


def test_the_walk_skips_what_camera_rays_do_not_cross():
    from diff_recon_hip import MeshBVH, camera_rays
    v, f = refs.small_triangle_soup(16384, seed=16)
    o, d = camera_rays(Cam(128, 128, (0.3, 0.2, -2.0), (0.5, 0.5, 0.5), 0.3))
    bvh = MeshBVH(_dev(v), _dev(f))
    visits, first = torch.zeros(1, device=DEV, dtype=torch.int64), torch.zeros(1, device=DEV, dtype=torch.int64)
    c = bvh.ray_crossings(o, d, leaf_visits=visits)
    bvh.ray_cast(o, d, leaf_visits=first)
    waves, leaves = 16384 // 64, 16384 // LEAF
    n = int(visits.item())
    print(f"16384 camera rays on 16384 small triangles: {n} leaf visits = {n / waves:.1f} per wave (first hit: {int(first.item()) / waves:.1f}), "
          f"brute force {waves * leaves}; rays that hit {float((c.hits > 0).float().mean()):.3f}")
    assert 0 < n < waves * leaves and n >= int(first.item())  # it cannot prune on a nearest hit, but it does skip the boxes nobody crosses
    sub = np.arange(0, 16384, 16)
    _same(tuple(x.cpu().numpy()[sub] for x in c), ref.crossings(o.cpu().numpy()[sub], d.cpu().numpy()[sub], v, f))


# ---- the signed distance call -------------------------------------------------------------------------------------------------------------------------
def test_signed_distance_call_every_case_every_rule_and_only_undecided():
    from diff_recon_hip import mesh_inside
    from diff_triangle_rasterization_2D import _C as native
    lib = mesh_inside._lib
    rng = np.random.default_rng(20)
    Q = 1000
    d2 = (rng.random(Q) * 4).astype(np.float64)
    d2[::7], d2[1::50], d2[2::50], d2[3::50] = 0.0, np.nan, np.inf, 5e-324
    w2 = rng.integers(-7, 8, Q).astype(np.int32)
    touches = (rng.random(Q) < 0.1).astype(np.int32)
    hits = np.where(rng.random(Q) < 0.05, -1, np.abs(w2) + touches).astype(np.int32)
    clean = ref.clean(hits, w2, touches)
    w = -(w2 // 2)
    assert clean.sum() > 300 and (~clean).sum() > 300
    g = [_dev(a) for a in (d2, w2, touches, hits)]
    previous = None
    for code, rule in enumerate(ref.RULES):
        with np.errstate(invalid="ignore"):
            r = np.sqrt(d2).astype(np.float32)
        want = np.where(clean & ref.inside_by(w, rule), -r, r).astype(np.float32)
        wdec = clean.copy()
        want[d2 == 0], wdec[d2 == 0] = 0.0, True
        want[~(d2 < np.inf)], wdec[~(d2 < np.inf)] = NAN, False
        with poison.PoisonedEmpty("nan") as pe:
            out, dec = torch.empty(Q, device=DEV, dtype=torch.float32), torch.empty(Q, device=DEV, dtype=torch.uint8)
            rc = lib.tsi_signed_distance(Q, *(t.data_ptr() for t in g), code, 0, out.data_ptr(), dec.data_ptr(), native.stream())
            assert rc == 0, lib.tsi_last_error()
            torch.cuda.synchronize()
            pe.check_guards()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)) and np.array_equal(dec.cpu().numpy(), wdec.astype(np.uint8)), rule
        assert previous is None or not np.array_equal(previous, want)  # the rules differ on these windings
        previous = want
        # only_undecided: what is decided stays, bit for bit; the rest is worked out anew
        held = np.where(np.arange(Q) % 3 == 0, 1, 0).astype(np.uint8)
        held[5] = 255
        mark = np.full(Q, 123.5, np.float32)
        out, dec = _dev(mark.copy()), _dev(held.copy())
        assert lib.tsi_signed_distance(Q, *(t.data_ptr() for t in g), code, 1, out.data_ptr(), dec.data_ptr(), native.stream()) == 0
        assert np.array_equal(out.cpu().numpy().view(np.uint32), np.where(held != 0, mark, want).view(np.uint32))
        assert np.array_equal(dec.cpu().numpy(), np.where(held != 0, held, wdec.astype(np.uint8)))


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cube_grid():
    """The cube [-1, 1]^3 and the 17^3 grid of spacing 0.25 over [-2, 2]^3: its eight corners have no clean ray."""
    v, f = ref.cube()
    p = ref.grid_points((-2.0, -2.0, -2.0), 0.25, (17, 17, 17))
    return v, f, p, ref.signed_distance(p, v, f), ref.winding_number(p, v, f)


def _points_with_everything():
    cv, cf = _closed()
    rng = np.random.default_rng(30)
    p = rng.uniform(-1.4, 1.4, (700, 3)).astype(np.float32)
    p[:100] = cv[rng.integers(0, len(cv), 100)]                                    # ON vertices: touches along every direction
    tri = cv[cf[rng.integers(0, len(cf), 100)]]
    p[100:200] = (0.5 * tri[:, 0] + 0.5 * tri[:, 1]).astype(np.float32)            # on edges, up to rounding
    p[200:300] = (p[200:300] * np.float32(0.2))                                    # well inside
    p[360], p[361] = (NAN, 0, 0), (0, INF, 0)
    return cv, cf, p


def test_signed_distance_contains_points_and_winding_number_match_the_reference_retries_included():
    from diff_recon_hip import MeshBVH, contains_points, signed_distance, winding_number
    v, f, p, (wsdf, wface, wdec), (ww, wdecided, tried) = _cube_grid()
    assert tried.sum(axis=1).tolist() == [4913, 8, 8]
    for mesh, pts, keep in ((ref.cube(), p, None), (_points_with_everything()[:2], _points_with_everything()[2], None),
                            (ref.join(ref.cube(), ref.cube(0.5, reverse=True)), p[::3], None), (ref.cube(reverse=True), p[::5], None),
                            (_soup(65), p[::9] * np.float32(0.25) + np.float32(0.5), np.arange(65) % 4 != 0)):
        bvh = MeshBVH(_dev(mesh[0]), _dev(mesh[1]), None if keep is None else _dev(keep))
        w, decided = winding_number(_dev(pts), bvh)
        want_w, want_decided, want_tried = ref.winding_number(pts, *mesh, keep)
        assert w.dtype == torch.int32 and decided.dtype == torch.bool
        assert np.array_equal(w.cpu().numpy(), want_w) and np.array_equal(decided.cpu().numpy(), want_decided)
        for rule in ref.RULES:
            sdf, face, dec = signed_distance(_dev(pts), bvh, rule=rule)
            want = ref.signed_distance(pts, *mesh, keep, rule=rule)
            assert sdf.dtype == torch.float32 and face.dtype == torch.int32 and dec.dtype == torch.bool
            assert np.array_equal(sdf.cpu().numpy().view(np.uint32), want[0].view(np.uint32)), rule
            assert np.array_equal(face.cpu().numpy(), want[1]) and np.array_equal(dec.cpu().numpy(), want[2])
            inside, dec = contains_points(_dev(pts), bvh, rule=rule)
            want = ref.contains_points(pts, *mesh, keep, rule=rule)
            assert inside.dtype == torch.bool and np.array_equal(inside.cpu().numpy(), want[0]) and np.array_equal(dec.cpu().numpy(), want[1])
    cv, cf, pts = _points_with_everything()
    _, _, tried = ref.winding_number(pts, cv, cf)
    assert tried[1].sum() >= 100 and tried[2].sum() >= 100 and tried[1].sum() < 200  # the retries ran, and on the undecided points only
    sdf, face, dec = signed_distance(_dev(np.zeros((0, 3), np.float32)), (_dev(cv), _dev(cf)))
    assert sdf.shape == face.shape == dec.shape == (0,)
    with pytest.raises(ValueError):
        signed_distance(_dev(pts), (_dev(cv), _dev(cf)), rule="even")


def test_mesh_to_sdf_of_the_cube_extracts_one_closed_piece_within_a_voxel():
    from diff_recon_hip import extract_isosurface, mesh_to_sdf, mesh_topology, point_to_mesh_distance, weld_mesh
    v, f, p, (wsdf, _, wdec), _ = _cube_grid()
    mesh = (_dev(v), _dev(f))
    field = mesh_to_sdf(mesh, (-2.0, -2.0, -2.0), 0.25, (17, 17, 17))
    assert field.shape == (17, 17, 17) and field.dtype == torch.float32 and wdec.all()
    assert np.array_equal(field.cpu().numpy().reshape(-1).view(np.uint32), wsdf.view(np.uint32))
    soup_v, soup_f = extract_isosurface(field, (-2.0, -2.0, -2.0), 0.25)
    w = weld_mesh(soup_v, soup_f, eps=0.0)
    topo = mesh_topology(w.stats["num_vertices"], w.faces)
    print("mesh_to_sdf of the cube at 17^3, extracted and welded:", topo)
    assert topo["faces"] > 100 and topo["pieces"] == 1 and topo["boundary"] == 0 and topo["euler"] == 2
    # a vertex sits on a grid edge whose ends have opposite signs, and the surface crosses that same edge: within h, and the fp32 roundings
    _, d2, _ = point_to_mesh_distance(w.vertices, mesh)
    worst = float(d2.max().sqrt())
    print(f"largest distance of an extracted vertex to the cube: {worst:.6g} (h = 0.25)")
    assert worst <= 0.25 + 4 * float(np.spacing(np.float32(2.0)))
    # in units of trunc, clipped; undecided samples are NaN
    unit = mesh_to_sdf(mesh, (-2.0, -2.0, -2.0), 0.25, (17, 17, 17), trunc=0.5).cpu().numpy().reshape(-1)
    assert np.array_equal(unit, np.clip(wsdf.astype(np.float64) / 0.5, -1, 1).astype(np.float32))
    nx_field = mesh_to_sdf(mesh, (-2.0, -1.0, 0.0), 0.5, (9, 5, 3), rule="positive")
    assert nx_field.shape == (3, 5, 9)
    assert np.array_equal(nx_field.cpu().numpy().reshape(-1), ref.signed_distance(ref.grid_points((-2.0, -1.0, 0.0), 0.5, (9, 5, 3)), v, f, rule="positive")[0])
    open_v, open_f = v, f[2:]  # a face pair missing: samples whose three rays all leave through the rim or run along it may stay undecided
    holed = mesh_to_sdf((_dev(open_v), _dev(open_f)), (-2.0, -2.0, -2.0), 0.25, (17, 17, 17)).cpu().numpy().reshape(-1)
    want, _, wdec = ref.signed_distance(p, open_v, open_f)
    assert np.array_equal(np.isnan(holed), ~wdec) and np.array_equal(holed[wdec], want[wdec])


def test_mesh_volume_iou_of_two_overlapping_cubes_is_exactly_a_third():
    from diff_recon_hip import mesh_volume_iou
    a, b = ref.cube(), ref.cube(centre=(1.0, 0.0, 0.0))
    res = mesh_volume_iou((_dev(a[0]), _dev(a[1])), (_dev(b[0]), _dev(b[1])), None, origin=(-1.875, -1.875, -1.875), voxel_size=0.25, dims=(20, 16, 16))
    print("mesh_volume_iou:", res)
    assert (res["inside_a"], res["inside_b"], res["inside_both"], res["inside_either"], res["undecided"]) == (512, 512, 256, 768, 0)
    assert res["iou"] == 256 / 768 and res["samples"] == 20 * 16 * 16
    auto = mesh_volume_iou((_dev(a[0]), _dev(a[1])), (_dev(a[0]), _dev(a[1])), 24)
    assert auto["iou"] == 1.0 and auto["inside_a"] == auto["inside_b"] == auto["inside_both"] > 1000 and max(auto["dims"]) == 24
    far = mesh_volume_iou((_dev(a[0]), _dev(a[1])), ref_to_dev(ref.cube(centre=(5.0, 0.0, 0.0))), 24)
    assert far["iou"] == 0.0 and far["inside_both"] == 0 and far["inside_a"] > 0 and far["inside_b"] > 0


def ref_to_dev(mesh):
    return _dev(mesh[0]), _dev(mesh[1])


def test_remesh_closes_the_cube_and_its_offset_surface_encloses_it():
    from diff_recon_hip import contains_points, mesh_topology, point_to_mesh_distance, remesh
    v, f = ref.cube()
    mesh = ref_to_dev((v, f))
    plain = remesh(mesh, 24)
    topo = mesh_topology(plain.vertices.shape[0], plain.faces)
    print("remesh(cube, 24):", topo, {k: plain.stats[k] for k in ("dims", "voxel_size", "undecided", "inside")})
    assert topo["pieces"] == 1 and topo["boundary"] == 0 and topo["euler"] == 2 and plain.stats["undecided"] == 0 and plain.stats["dims"] == (24, 24, 24)
    _, d2, _ = point_to_mesh_distance(plain.vertices, mesh)
    assert float(d2.max().sqrt()) <= plain.stats["voxel_size"] * (1 + 1e-6)
    grown = remesh(mesh, 24, offset=0.25)
    topo = mesh_topology(grown.vertices.shape[0], grown.faces)
    assert topo["pieces"] == 1 and topo["boundary"] == 0 and topo["euler"] == 2 and grown.stats["offset"] == 0.25
    assert grown.stats["inside"] * grown.stats["voxel_size"] ** 3 > plain.stats["inside"] * plain.stats["voxel_size"] ** 3  # the grids differ: by volume
    inside, decided = contains_points(_dev(v), (grown.vertices, grown.faces))
    assert bool(inside.all()) and bool(decided.all())  # the cube's own vertices lie inside its offset surface
    inside, decided = contains_points(plain.vertices, (grown.vertices, grown.faces))
    assert bool(inside.all()) and bool(decided.all())
    shrunk = remesh(mesh, 24, offset=-0.25)
    inside, decided = contains_points(shrunk.vertices, mesh)
    assert bool(inside.all()) and bool(decided.all()) and shrunk.stats["inside"] < plain.stats["inside"]  # the same grid: a negative offset grows no box
    with pytest.raises(ValueError):
        remesh(mesh, 4)


# ---- example ------------------------------------------------------------------------------------------------------------------------------------------
def test_example_reports_the_remeshed_mesh():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    res = train_synthetic.mesh_scores(m, "2D", extract=32, remesh=40, **cfg)["fused"]
    r = res["remeshed"]
    lines = train_synthetic.remeshed_report(r)
    print("\n".join(lines))
    assert r is not None and r["resolution"] == 40 and max(r["dims"]) == 40 and r["samples"] == r["dims"][0] * r["dims"][1] * r["dims"][2]
    assert r["topology"]["faces"] > 0 and r["inside"] > 0 and 0 <= r["undecided"] < r["samples"]
    for k in ("accuracy", "completeness", "chamfer", "hausdorff"):
        assert np.isfinite(r["to_fused"][k]) and r["to_fused"][k] >= 0, k
    assert len(lines) == 2 and "undecided" in lines[0] and "Euler characteristic" in lines[0] and "boundary edges" in lines[0] and "pieces" in lines[0]
    plain = train_synthetic.mesh_scores(m, "2D", extract=32, **cfg)["fused"]
    assert "remeshed" not in plain and plain["topology"] == res["topology"]
    assert train_synthetic.remeshed_report(None) == ["remeshed mesh: no surface was extracted, nothing to remesh"]
