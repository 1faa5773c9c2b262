"""numpy reference of include/ts_geom.h and diff_recon_hip/mesh_distance.py: the cross-set nearest search by brute force in fp32, the surface
sampler in 64-bit integers, the scores in float64.  Plain and slow on purpose; nothing here is shared with the code under test."""
import numpy as np

_M1, _M2, _GOLD = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB), np.uint64(0x9E3779B97F4A7C15)
_ONE = np.uint64(1)


def nearest(queries, refs, chunk=512):
    """(idx int32 (Q,), dist2 float32 (Q,)): d = (dx*dx + dy*dy) + dz*dz with every fp32 operation rounded; the eligible (all-finite) ref with
    the smallest d, ties to the smallest index (also when every d is +inf); -1 / +inf without an eligible ref; -1 / NaN for a non-finite query."""
    q, r = np.ascontiguousarray(queries, np.float32).reshape(-1, 3), np.ascontiguousarray(refs, np.float32).reshape(-1, 3)
    Q = q.shape[0]
    idx, dist2 = np.full(Q, -1, np.int32), np.full(Q, np.inf, np.float32)
    ids = np.nonzero(np.isfinite(r).all(axis=1))[0]
    re = r[ids]
    if len(ids):
        with np.errstate(over="ignore", invalid="ignore"):
            for a in range(0, Q, chunk):
                c = q[a:a + chunk]
                dx, dy, dz = (c[:, None, k] - re[None, :, k] for k in range(3))
                d = (dx * dx + dy * dy) + dz * dz
                assert d.dtype == np.float32
                j = np.argmin(np.where(np.isnan(d), np.float32(np.inf), d), axis=1)  # the first minimum: the smallest eligible index
                idx[a:a + chunk], dist2[a:a + chunk] = ids[j], d[np.arange(len(c)), j]
    bad = ~np.isfinite(q).all(axis=1)
    idx[bad], dist2[bad] = -1, np.nan
    return idx, dist2


def face_areas(vertices, faces, keep=None):
    v, f = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = v.shape[0], f.shape[0]
    ok = ((f >= 0) & (f < V)).all(axis=1)
    if keep is not None:
        ok &= np.asarray(keep).astype(bool)
    area = np.zeros(F, np.float64)
    g = f[ok]
    p = v[g].astype(np.float64)  # (n, 3, 3)
    fin = np.isfinite(p).all(axis=(1, 2))
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        a = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    area[np.nonzero(ok)[0]] = np.where(fin, a, 0.0)
    return area


def splitmix64(seed, k):
    """k: uint64 array of counters."""
    z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (k + _ONE) * _GOLD
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def weights(area):
    """(w uint64 (F,), C uint64 (F,)) for amax > 0."""
    area = np.asarray(area, np.float64)
    w = np.floor(area / area.max() * 4294967296.0).astype(np.uint64)
    return w, np.cumsum(w, dtype=np.uint64)


def sample(vertices, faces, area, n, seed):
    """(points float32 (n, 3), face int32 (n,))."""
    v, f, area = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3), np.asarray(area, np.float64)
    points, face = np.zeros((n, 3), np.float32), np.full(n, -1, np.int32)
    if len(area) == 0 or area.max() == 0 or n == 0:
        return points, face
    _, C = weights(area)
    W = int(C[-1])
    assert W >= 2 ** 32 > n
    s = np.arange(n, dtype=np.uint64)
    r0, r1 = splitmix64(seed, s * np.uint64(2)), splitmix64(seed, s * np.uint64(2) + _ONE)
    qn, rem = np.uint64(W // n), np.uint64(W % n)
    start = s * qn + np.minimum(s, rem)
    length = qn + (s < rem).astype(np.uint64)
    t = start + r0 % length
    face = np.searchsorted(C, t, "right").astype(np.int32)
    iu, iv = (r1 >> np.uint64(40)).astype(np.int64), ((r1 >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.int64)
    flip = iu + iv > 2 ** 24
    iu, iv = np.where(flip, 2 ** 24 - iu, iu), np.where(flip, 2 ** 24 - iv, iv)
    u, w = (iu.astype(np.float32) * np.float32(2.0 ** -24))[:, None], (iv.astype(np.float32) * np.float32(2.0 ** -24))[:, None]
    p0, p1, p2 = (v[f[face, k]] for k in range(3))
    points = (p0 + u * (p1 - p0)) + w * (p2 - p0)
    assert points.dtype == np.float32
    return points, face


def scores(idx_ab, d2_ab, idx_ba, d2_ba, thresholds=()):
    """The dict of point_cloud_distance from the two one-way searches, in float64."""
    def one_way(idx, d2):
        found = idx >= 0
        sq = d2[found].astype(np.float64)
        return sq, np.sqrt(sq), int((~found).sum())
    sq_a, da, a_dropped = one_way(idx_ab, d2_ab)
    sq_b, db, b_dropped = one_way(idx_ba, d2_ba)
    mean = lambda x: float(x.sum() / len(x)) if len(x) else float("nan")
    res = {"accuracy": mean(da), "completeness": mean(db), "chamfer": (mean(da) + mean(db)) / 2, "chamfer_sq": mean(sq_a) + mean(sq_b),
           "hausdorff": max([float(d.max()) for d in (da, db) if len(d)], default=float("nan")), "a_count": len(da), "b_count": len(db),
           "a_dropped": a_dropped, "b_dropped": b_dropped, "thresholds": [float(t) for t in thresholds], "precision": [], "recall": [], "fscore": [],
           "a_within": [], "b_within": []}
    for tau in res["thresholds"]:
        na, nb = int((da <= tau).sum()), int((db <= tau).sum())
        p, r = (na / len(da) if len(da) else 0.0), (nb / len(db) if len(db) else 0.0)
        res["a_within"].append(na)
        res["b_within"].append(nb)
        res["precision"].append(p)
        res["recall"].append(r)
        res["fscore"].append(2 * p * r / (p + r) if p + r > 0 else 0.0)
    return res


def point_cloud_distance(a, b, thresholds=()):
    return scores(*nearest(a, b), *nearest(b, a), thresholds)


def mesh_distance(mesh_a, mesh_b, samples, seed=0, thresholds=()):
    (va, fa), (vb, fb) = mesh_a, mesh_b
    area_a, area_b = face_areas(va, fa), face_areas(vb, fb)
    pa, _ = sample(va, fa, area_a, samples, seed)
    pb, _ = sample(vb, fb, area_b, samples, seed + 1)
    res = point_cloud_distance(pa, pb, thresholds)
    res["area_a"], res["area_b"] = float(area_a.sum()), float(area_b.sum())
    return res


def barycentric_excess(vertices, faces, points, face):
    """How far outside its face the worst point lies, as float64 barycentrics: max(-u, -v, u + v - 1) over the samples (<= 0: all inside)."""
    p = np.asarray(vertices, np.float32).reshape(-1, 3)[np.asarray(faces)[face]].astype(np.float64)
    T = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]], axis=2)
    uv = np.einsum("nij,nj->ni", np.linalg.pinv(T), np.asarray(points, np.float64) - p[:, 0])
    return float(max(-uv.min(), uv.sum(axis=1).max() - 1))


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------------
def heavy_tailed_soup(F, seed):
    """(vertices (3 F, 3) float32, faces (F, 3) int32): random triangles whose sizes span orders of magnitude (log-normal, sigma 2)."""
    rng = np.random.default_rng(seed)
    centre = rng.random((F, 1, 3))
    size = np.exp(rng.normal(size=(F, 1, 1)) * 2.0) * 0.05
    tri = (centre + rng.normal(size=(F, 3, 3)) * size).astype(np.float32)
    return tri.reshape(-1, 3), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def two_squares(h):
    """Two unit squares of two triangles each, parallel, `h` apart."""
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    return (sq, faces), (sq + np.array([0, 0, h], np.float32), faces)
