"""numpy reference of include/ts_bvh.h and diff_recon_hip/mesh_surface.py: the closest face of every query by brute force over all faces, in
float64 with every operation written out as the header writes it, and an independent closest-point routine (the region walk of Ericson,
"Real-Time Collision Detection" 5.1.5) that only checks the reference.  Plain and slow on purpose; nothing here is shared with the code
under test."""
import numpy as np

import ref_mesh_distance as refd


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _sub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def _clamp01(x):
    return np.where(x < 0.0, 0.0, np.where(x > 1.0, 1.0, x))


def _segment(q, p0, p1):
    """seg(p0, p1): (value, point)."""
    d, w = _sub(p1, p0), _sub(q, p0)
    den = _dot(d, d)
    t = np.where(den == 0.0, 0.0, _clamp01(_dot(w, d) / np.where(den == 0.0, 1.0, den)))
    td = (t * d[0], t * d[1], t * d[2])
    r = _sub(w, td)
    return _dot(r, r), (p0[0] + td[0], p0[1] + td[1], p0[2] + td[2])


def _axis_excess(lo, hi, q):
    below, above = lo - q, q - hi
    return np.where(below > 0.0, below, np.where(above > 0.0, above, 0.0))


def box_bound(q, lo, hi):
    """L(q, box); q, lo, hi: triples of broadcastable float64 arrays."""
    e = [_axis_excess(lo[k], hi[k], q[k]) for k in range(3)]
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def point_triangle(q, a, b, c):
    """(D', point) of the header for broadcastable triples of float64 arrays: q the queries, a / b / c the faces' vertices."""
    best, point = _segment(q, a, b)
    point = [np.broadcast_to(p, best.shape).copy() for p in point]
    for p0, p1 in ((b, c), (c, a)):
        v, pt = _segment(q, p0, p1)
        take = v < best
        best = np.where(take, v, best)
        point = [np.where(take, pt[k], point[k]) for k in range(3)]
    e1, e2 = _sub(b, a), _sub(c, a)
    n = _cross(e1, e2)
    nn = _dot(n, n)
    wa, wb, wc = _sub(q, a), _sub(q, b), _sub(q, c)
    s1 = _dot(_cross(e1, wa), n)
    s2 = _dot(_cross(_sub(c, b), wb), n)
    s3 = _dot(_cross(_sub(a, c), wc), n)
    s = _dot(wa, n)
    safe = np.where(nn > 0.0, nn, 1.0)
    v = (s * s) / safe
    take = (nn > 0.0) & (s1 >= 0.0) & (s2 >= 0.0) & (s3 >= 0.0) & (v < best)
    k = s / safe
    pt = (q[0] - k * n[0], q[1] - k * n[1], q[2] - k * n[2])
    best = np.where(take, v, best)
    point = [np.where(take, pt[i], point[i]) for i in range(3)]
    lo = [np.minimum(np.minimum(a[i], b[i]), c[i]) for i in range(3)]
    hi = [np.maximum(np.maximum(a[i], b[i]), c[i]) for i in range(3)]
    bound = box_bound(q, lo, hi)
    return np.where(best > bound, best, bound), point


def eligible_faces(vertices, faces, keep=None):
    v, f = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < v.shape[0])).all(axis=1)
    if keep is not None:
        ok &= np.asarray(keep).astype(bool)
    ids = np.nonzero(ok)[0]
    fin = np.isfinite(v[f[ids]]).all(axis=(1, 2)) if len(ids) else np.zeros(0, bool)
    return ids[fin]


def closest(queries, vertices, faces, keep=None, chunk=128):
    """(face int32 (Q,), dist2 float64 (Q,), point float32 (Q, 3)): the eligible face with the smallest D', ties to the smallest index;
    -1 / +inf / NaN without an eligible face; -1 / NaN / NaN for a non-finite query."""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    v, f = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    Q = q.shape[0]
    face, dist2, point = np.full(Q, -1, np.int32), np.full(Q, np.inf, np.float64), np.full((Q, 3), np.nan, np.float32)
    ids = eligible_faces(v, f, keep)
    if len(ids):
        tri = v[f[ids]].astype(np.float64)  # (n, 3, 3): the fp32 coordinates widened
        a, b, c = ([tri[None, :, k, i] for i in range(3)] for k in range(3))
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            for lo in range(0, Q, chunk):
                qc = q[lo:lo + chunk].astype(np.float64)
                d, pt = point_triangle([qc[:, None, i] for i in range(3)], a, b, c)
                j = np.argmin(np.where(np.isnan(d), np.inf, d), axis=1)  # the first minimum: the smallest eligible index
                rows = np.arange(len(qc))
                face[lo:lo + chunk], dist2[lo:lo + chunk] = ids[j], d[rows, j]
                point[lo:lo + chunk] = np.stack([pt[i][rows, j] for i in range(3)], axis=1).astype(np.float32)
    bad = ~np.isfinite(q).all(axis=1)
    face[bad], dist2[bad], point[bad] = -1, np.nan, np.nan
    return face, dist2, point


def ericson_dist2(p, a, b, c):
    """Squared distance of the points p (n, 3) to the triangles (a, b, c) (n, 3 each), float64, by Voronoi-region classification: an
    algorithm of another shape than point_triangle (no per-edge minimum, no plane test), for non-degenerate triangles."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    dot = lambda u, w: (u * w).sum(axis=-1)
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = p - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = p - c
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ab, t_ac = d1 / (d1 - d3), d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = 1.0 / (va + vb + vc)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    pts = [a, b, a + t_ab[:, None] * ab, c, a + t_ac[:, None] * ac, b + t_bc[:, None] * (c - b)]
    inside = a + ab * (vb * denom)[:, None] + ac * (vc * denom)[:, None]
    region = np.select(conds, np.arange(6), default=6)
    out = inside
    for k in range(5, -1, -1):
        out = np.where((region == k)[:, None], pts[k], out)
    r = p - out
    return dot(r, r)


def scores(face_ab, d2_ab, face_ba, d2_ba, thresholds=()):
    """The dict of mesh_surface_distance without the areas, from the two one-way queries."""
    return refd.scores(face_ab, np.asarray(d2_ab, np.float64), face_ba, np.asarray(d2_ba, np.float64), thresholds)


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------------
def grid_mesh(n, seed=0, jitter=0.2):
    """(vertices ((n+1)^2, 3) float32, faces (2 n^2, 3) int32): an indexed height field over the unit square with SHARED vertices, so that
    the edges and vertices between faces are hit by more than one face at the same distance."""
    rng = np.random.default_rng(seed)
    g = np.linspace(0.0, 1.0, n + 1)
    x, y = np.meshgrid(g, g, indexing="ij")
    z = 0.1 * np.sin(5 * x) * np.cos(4 * y) + jitter / n * rng.random(x.shape)
    v = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    p = (i * (n + 1) + j).reshape(-1)
    faces = np.concatenate([np.stack([p, p + n + 1, p + n + 2], axis=1), np.stack([p, p + n + 2, p + 1], axis=1)]).astype(np.int32)
    return v, faces[rng.permutation(len(faces))]


def small_triangle_soup(F, seed, edge=0.01):
    """(vertices (3 F, 3) float32, faces (F, 3) int32): triangles of edge about `edge` spread over the unit cube."""
    rng = np.random.default_rng(seed)
    tri = (rng.random((F, 1, 3)) + (rng.random((F, 3, 3)) - 0.5) * edge).astype(np.float32)
    return tri.reshape(-1, 3), np.arange(3 * F, dtype=np.int32).reshape(F, 3)
