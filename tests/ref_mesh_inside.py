"""numpy reference of include/ts_inside.h and diff_recon_hip/mesh_inside.py: the crossing counts of every ray by brute force over all faces, in
float64 on top of ref_mesh_ray (shear, evaluate, bad_rays: numpy rounds every operation, so this is the bit-exact oracle), and the winding
number, the inside test and the signed distance that follow, on top of ref_mesh_surface.closest.  U, V and W are recomputed here: the zero tests
are on the raw values, not on the U / det that evaluate returns, because a quotient can underflow to 0.  Plain and slow on purpose; nothing
here is shared with the code under test."""
import itertools

import numpy as np

import ref_mesh_ray as refr
import ref_mesh_surface as refs

INF, NAN = np.inf, np.nan
DIRECTIONS = np.array([(0.7548777, 0.5698403, 0.3247180), (-0.4301597, 0.6823278, -0.5905000), (0.2360680, -0.4142136, 0.8793852)], np.float32)
RULES = ("nonzero", "odd", "positive")


def edge_values(o, d, tri):
    """(U, V, W) (R, n) of every ray o, d (R, 3) float64 against every face tri (n, 3, 3) float64: the header's formulas, every operation
    rounded."""
    R, n = len(o), len(tri)
    kx, ky, kz, Sx, Sy, _ = refr.shear(d)
    P = []
    for v in range(3):
        p = tri[None, :, v, :] - o[:, None, :]
        pick = lambda k: np.take_along_axis(p, np.broadcast_to(k[:, None, None], (R, n, 1)), axis=2)[..., 0]
        pz = pick(kz)
        P.append((pick(kx) - Sx[:, None] * pz, pick(ky) - Sy[:, None] * pz))
    (Ax, Ay), (Bx, By), (Cx, Cy) = P
    return Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax


def crossings(o, d, v, f, keep=None, tmin=0.0, tmax=INF, t_limit=None, chunk=64):
    """(hits, winding2, touches), int32 (Q,) each.  d: (Q, 3), or (3,) for one direction shared by every ray."""
    o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, np.float32)
    d = np.broadcast_to(d, o.shape).copy() if d.ndim == 1 else d.reshape(-1, 3)
    v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    Q = len(o)
    hits, winding2, touches = np.zeros(Q, np.int32), np.zeros(Q, np.int32), np.zeros(Q, np.int32)
    bad = refr.bad_rays(o, d, t_limit)
    hi = np.full(Q, float(tmax), np.float64)
    if t_limit is not None:
        hi = refr.min2(hi, np.where(bad, 0.0, np.asarray(t_limit, np.float32).astype(np.float64)))
    ids = refs.eligible_faces(v, f, keep)
    if len(ids) and Q:
        tri = v[f[ids]].astype(np.float64)
        o64, d64 = np.where(bad[:, None], 0.0, o.astype(np.float64)), np.where(bad[:, None], [1.0, 0.0, 0.0], d.astype(np.float64))
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            for s in range(0, Q, chunk):
                e = slice(s, s + chunk)
                hit, _, _, _, _, det = refr.evaluate(o64[e], d64[e], tri, float(tmin), hi[e], False)
                U, V, W = edge_values(o64[e], d64[e], tri)
                assert np.array_equal((U + V) + W, det)  # the same numbers as the ray reference's
                z = (U == 0).astype(np.int64) + (V == 0) + (W == 0)
                side = np.where(det > 0, 1, -1)
                hits[e] = hit.sum(axis=1)
                winding2[e] = (np.where(hit & (z == 0), 2 * side, 0) + np.where(hit & (z == 1), side, 0)).sum(axis=1)
                touches[e] = (hit & (z >= 2)).sum(axis=1)
    hits[bad], winding2[bad], touches[bad] = -1, 0, 0
    return hits, winding2, touches


def clean(hits, winding2, touches):
    return (hits >= 0) & (touches == 0) & (winding2 % 2 == 0)


def inside_by(w, rule):
    assert rule in RULES, rule
    return w != 0 if rule == "nonzero" else (w % 2 != 0 if rule == "odd" else w > 0)


def winding_number(points, v, f, keep=None):
    """(w int32, decided bool, tried (3, Q) bool): w = -winding2 / 2 of the first clean direction, 0 where undecided; tried[k]: direction k
    was needed."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    w, decided, tried = np.zeros(len(p), np.int32), np.zeros(len(p), bool), np.zeros((3, len(p)), bool)
    for k in range(3):
        todo = np.nonzero(~decided)[0]
        if not len(todo):
            break
        tried[k, todo] = True
        h, w2, t = crossings(p[todo], DIRECTIONS[k], v, f, keep)
        ok = clean(h, w2, t)
        w[todo[ok]] = -(w2[ok] // 2)
        decided[todo[ok]] = True
    return w, decided, tried


def contains_points(points, v, f, keep=None, rule="nonzero"):
    w, decided, _ = winding_number(points, v, f, keep)
    return inside_by(w, rule) & decided, decided


def signed_distance(points, v, f, keep=None, rule="nonzero"):
    """(sdf float32, face int32, decided bool) of the header's four cases."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    face, d2, _ = refs.closest(p, v, f, keep)
    w, clean_ray, _ = winding_number(p, v, f, keep)
    with np.errstate(invalid="ignore"):
        r = np.sqrt(d2).astype(np.float32)
    out = np.where(clean_ray & inside_by(w, rule), -r, r).astype(np.float32)
    decided = clean_ray.copy()
    out[d2 == 0], decided[d2 == 0] = 0.0, True
    nodata = ~(d2 < INF)
    out[nodata], decided[nodata] = NAN, False
    return out, face, decided


def grid_points(origin, h, dims):
    """(nz ny nx, 3) float32, x fastest: (float)((double)o + (double)h idx) with o and h rounded to fp32 first (include/ts_volume.h)."""
    o, h = np.asarray(origin, np.float32).astype(np.float64), float(np.float32(h))
    ax = [(o[a] + h * np.arange(n, dtype=np.float64)).astype(np.float32) for a, n in enumerate(dims)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], axis=-1).reshape(-1, 3)


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------------
def cube(h=1.0, centre=(0.0, 0.0, 0.0), reverse=False):
    """The cube centre + [-h, h]^3: eight vertices, twelve outward counter-clockwise faces (inward with reverse)."""
    v = (np.array(list(itertools.product((-h, h), repeat=3)), np.float64) + np.array(centre, np.float64)).astype(np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, (f[:, ::-1].copy() if reverse else f)


def join(*meshes):
    """One mesh of several: the vertices stacked, the faces shifted."""
    vs, fs, at = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + at)
        at += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)
