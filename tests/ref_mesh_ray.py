"""numpy reference of include/ts_ray.h and diff_recon_hip/mesh_ray.py: the first hit of every ray by brute force over all faces, in float64
with every operation written out as the header writes it (numpy rounds every operation, so this is the bit-exact oracle), a pruned walk
over groups of faces that only checks the header's argument, and the inputs the tests share.  Plain and slow on purpose; nothing here is
shared with the code under test."""
import numpy as np

import ref_mesh_surface as refs

INF, NAN = np.inf, np.nan
PAD = 2.0 ** -40


def min2(x, y):
    """min of the header: y < x ? y : x -- of a +0 and a -0 the first stays."""
    return np.where(y < x, y, x)


def max2(x, y):
    return np.where(y > x, y, x)


def slab(o, d, lo, hi):
    """(ok, tn, tf) of the slab interval; o, d, lo, hi: triples of broadcastable float64 arrays.  ok: every zero-direction axis passes and
    tn <= tf; tmin and the upper limit are the caller's."""
    shape = np.broadcast(o[0], d[0], lo[0], hi[0]).shape
    tn, tf, ok = np.full(shape, -INF), np.full(shape, INF), np.ones(shape, bool)
    for k in range(3):
        zero = np.broadcast_to(d[k] == 0.0, shape)
        dk = np.where(d[k] == 0.0, 1.0, d[k])
        ta, tb = (lo[k] - o[k]) / dk, (hi[k] - o[k]) / dk
        near, far = min2(ta, tb), max2(ta, tb)
        near_p, far_p = near - np.abs(near) * PAD, far + np.abs(far) * PAD
        tn, tf = np.where(zero, tn, max2(tn, near_p)), np.where(zero, tf, min2(tf, far_p))
        ok = ok & (~zero | ((lo[k] <= o[k]) & (o[k] <= hi[k])))
    return ok & (tn <= tf), tn, tf


def shear(d):
    """(kx, ky, kz, Sx, Sy, Sz) of the rays d (R, 3) float64, none of them zero."""
    a = np.abs(d)
    kz = np.zeros(len(d), np.int64)
    kz[a[:, 1] > a[:, 0]] = 1
    kz[a[:, 2] > a[np.arange(len(d)), kz]] = 2
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    rows = np.arange(len(d))
    swap = d[rows, kz] < 0.0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    dz = d[rows, kz]
    return kx, ky, kz, d[rows, kx] / dz, d[rows, ky] / dz, 1.0 / dz


def evaluate(o, d, tri, tmin, hi, cull_back):
    """Every ray against every face: o, d (R, 3) float64 (good rays), tri (n, 3, 3) float64, hi (R,).  Returns (hit (R, n) bool, t' (R, n),
    U / det, V / det, W / det, det)."""
    R, n = len(o), len(tri)
    kx, ky, kz, Sx, Sy, Sz = shear(d)
    rows = np.arange(R)[:, None]
    P = []
    for v in range(3):
        p = tri[None, :, v, :] - o[:, None, :]                       # (R, n, 3)
        pz = np.take_along_axis(p, np.broadcast_to(kz[:, None, None], (R, n, 1)), axis=2)[..., 0]
        px = np.take_along_axis(p, np.broadcast_to(kx[:, None, None], (R, n, 1)), axis=2)[..., 0]
        py = np.take_along_axis(p, np.broadcast_to(ky[:, None, None], (R, n, 1)), axis=2)[..., 0]
        P.append((px - Sx[:, None] * pz, py - Sy[:, None] * pz, Sz[:, None] * pz))
    (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = P
    U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
    det = (U + V) + W
    neg, pos = (U < 0) | (V < 0) | (W < 0), (U > 0) | (V > 0) | (W > 0)
    cand = (det != 0) & ~(neg & pos)
    if cull_back:
        cand &= det > 0
    safe = np.where(det != 0, det, 1.0)
    tt = ((U * Az + V * Bz) + W * Cz) / safe
    lo, up = tri.min(axis=1), tri.max(axis=1)                        # AABB(T): exact on fp32 values
    ok, tn, tf = slab([o[:, None, k] for k in range(3)], [d[:, None, k] for k in range(3)], [lo[None, :, k] for k in range(3)],
                      [up[None, :, k] for k in range(3)])
    crossed = ok & (tf >= tmin) & (tn <= hi[:, None])
    tp = max2(tt, tn)
    hit = cand & crossed & (tp >= tmin) & (tp <= hi[:, None])
    return hit, tp, U / safe, V / safe, W / safe, det


def bad_rays(o, d, t_limit=None):
    o, d = np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)
    bad = ~np.isfinite(o).all(axis=1) | ~np.isfinite(d).all(axis=1) | (d == 0).all(axis=1)
    if t_limit is not None:
        bad |= np.isnan(np.asarray(t_limit, np.float32))
    return bad


def cast(o, d, v, f, keep=None, tmin=0.0, tmax=INF, t_limit=None, cull_back=False, chunk=64):
    """(face int32 (Q,), t float64 (Q,), bary float32 (Q, 3), side int8 (Q,)) by brute force over the eligible faces."""
    o, d = np.ascontiguousarray(o, np.float32).reshape(-1, 3), np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    Q = len(o)
    face, t = np.full(Q, -1, np.int32), np.full(Q, INF, np.float64)
    bary, side = np.full((Q, 3), NAN, np.float32), np.zeros(Q, np.int8)
    bad = bad_rays(o, d, t_limit)
    hi = np.full(Q, float(tmax), np.float64)
    if t_limit is not None:
        tl = np.where(bad, 0.0, np.asarray(t_limit, np.float32).astype(np.float64))
        hi = min2(hi, tl)
    ids = refs.eligible_faces(v, f, keep)
    if len(ids) and Q:
        tri = v[f[ids]].astype(np.float64)
        o64, d64 = np.where(bad[:, None], 0.0, o.astype(np.float64)), np.where(bad[:, None], [1.0, 0.0, 0.0], d.astype(np.float64))
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            for s in range(0, Q, chunk):
                e = slice(s, s + chunk)
                hit, tp, bu, bv, bw, det = evaluate(o64[e], d64[e], tri, float(tmin), hi[e], cull_back)
                key = np.where(hit, tp, INF)
                j = np.argmin(key, axis=1)                              # the first minimum: the smallest eligible index
                rows = np.arange(len(j))
                j = np.where(hit[rows, j], j, np.argmax(hit, axis=1))   # a hit at t' = +inf still beats no hit
                found = hit[rows, j]
                face[e] = np.where(found, ids[j], -1)
                t[e] = np.where(found, tp[rows, j], INF)
                bary[e] = np.where(found[:, None], np.stack([bu[rows, j], bv[rows, j], bw[rows, j]], axis=1), NAN).astype(np.float32)
                side[e] = np.where(found, np.where(det[rows, j] > 0, 1, -1), 0)
    face[bad], t[bad], bary[bad], side[bad] = -1, NAN, NAN, 0
    return face, t, bary, side


def pruned_cast(o, d, v, f, groups, tmin=0.0, tmax=INF, cull_back=False, order=None):
    """The header's argument as a program: `groups` is a list of arrays of face indices, each with the union box of its faces; a group is
    skipped when its box is not crossed or tn(box) > best (strict).  Returns what cast() returns, and the number of groups entered."""
    o, d = np.asarray(o, np.float32).reshape(-1, 3).astype(np.float64), np.asarray(d, np.float32).reshape(-1, 3).astype(np.float64)
    v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    tri = v[f].astype(np.float64)
    boxes = [(tri[g].min(axis=(0, 1)), tri[g].max(axis=(0, 1))) for g in groups]
    Q = len(o)
    face, t = np.full(Q, -1, np.int32), np.full(Q, INF, np.float64)
    bary, side = np.full((Q, 3), NAN, np.float32), np.zeros(Q, np.int8)
    entered = 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for i in range(Q):
            best, best_id = float(tmax), -1
            oi, di = o[i:i + 1], d[i:i + 1]
            for g in (range(len(groups)) if order is None else order[i]):
                lo, up = boxes[g]
                ok, tn, tf = slab(list(oi[0]), list(di[0]), list(lo), list(up))
                if not (ok and tf >= tmin and not tn > best):
                    continue
                entered += 1
                hit, tp, bu, bv, bw, det = evaluate(oi, di, tri[groups[g]], float(tmin), np.array([float(tmax)]), cull_back)
                for j in np.nonzero(hit[0])[0]:
                    fid = int(groups[g][j])
                    if tp[0, j] < best or (tp[0, j] == best and (best_id < 0 or fid < best_id)):
                        best, best_id = tp[0, j], fid
                        face[i], t[i], side[i] = fid, tp[0, j], 1 if det[0, j] > 0 else -1
                        bary[i] = np.array([bu[0, j], bv[0, j], bw[0, j]]).astype(np.float32)
    return (face, t, bary, side), entered


def visibility(points, centres, v, f, keep=None, rel_eps=1e-5):
    """(Q,) int32: how many centres see each point -- no hit of the ray o = c, d = fp32(p - c) with t' <= 1 - rel_eps."""
    p, c = np.asarray(points, np.float32).reshape(-1, 3), np.asarray(centres, np.float32).reshape(-1, 3)
    seen = np.zeros(len(p), np.int32)
    for k in range(len(c)):
        face, _, _, _ = cast(np.broadcast_to(c[k], p.shape), p - c[k], v, f, keep, 0.0, 1.0 - float(rel_eps))
        seen += face < 0
    return seen


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------------
def closed_mesh(levels, seed, spread=0.2):
    """(vertices float32, faces int32): an octahedron subdivided `levels` times (8 * 4^levels faces, SHARED vertices, outward counter-clockwise),
    every vertex pushed out radially by a random fp32 factor in [1 - spread, 1 + spread]: closed, star-shaped around the origin, not convex."""
    verts = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    verts = [np.array(p, np.float64) for p in verts]
    for _ in range(levels):
        mid, out = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = verts[i] + verts[j]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = out
    rng = np.random.default_rng(seed)
    scale = (1.0 + spread * (2.0 * rng.random(len(verts)) - 1.0)).astype(np.float32)
    v = (np.array(verts) * scale[:, None]).astype(np.float32)
    f = np.array(faces, np.int32)
    return v, f[rng.permutation(len(f))]


def rays_from_inside(v, f, n, seed, radius=0.3):
    """n rays (o, d float32) from inside the star-shaped mesh: origins within `radius` of the centre; a quarter each aimed at a vertex, at an
    edge midpoint, at a face centroid and in a random direction (some with one or two zero components)."""
    rng = np.random.default_rng(seed)
    o = (rng.normal(size=(n, 3)) * radius / 3).clip(-radius / 2, radius / 2).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = np.arange(n)
    tri = v[f[rng.integers(0, len(f), n)]]
    at_vertex = tri[:, 0]
    at_edge = (0.5 * tri[:, 0] + 0.5 * tri[:, 1]).astype(np.float32)
    at_face = (tri.astype(np.float64).mean(axis=1)).astype(np.float32)
    for r, target in ((0, at_vertex), (1, at_edge), (2, at_face)):
        d[k % 4 == r] = (target - o)[k % 4 == r]
    d[k % 32 == 3, 0] = 0.0
    d[k % 64 == 7, 1:] = 0.0
    return o, d


def mixed_rays(Q, v, f, seed):
    """Q rays (o, d float32) around the finite part of the mesh: origins in its box grown by a half, every thirteenth ON a vertex; directions
    aimed at face centroids, exactly at vertices, random, and with one or two zero components."""
    rng = np.random.default_rng(seed)
    fin = v[np.isfinite(v).all(axis=1)]
    lo, hi = fin.min(axis=0).astype(np.float64), fin.max(axis=0).astype(np.float64)
    ext = np.where(hi > lo, hi - lo, 1.0)
    o = (lo - 0.5 * ext + rng.random((Q, 3)) * 2.0 * ext).astype(np.float32)
    o[::13] = fin[rng.integers(0, len(fin), len(o[::13]))]
    ok = refs.eligible_faces(v, f)
    d = rng.normal(size=(Q, 3)).astype(np.float32)
    k = np.arange(Q)
    if len(ok):
        tri = v[f[ok[rng.integers(0, len(ok), Q)]]]
        centroid = tri.astype(np.float64).mean(axis=1).astype(np.float32)
        d[k % 4 == 0] = (centroid - o)[k % 4 == 0]
        d[k % 4 == 1] = (tri[:, 1] - o)[k % 4 == 1]
    d[k % 16 == 2, rng.integers(0, 3)] = 0.0
    two = k % 16 == 6
    axis = rng.integers(0, 3, Q)
    keep = d[k, axis].copy()
    d[two] = 0.0
    d[two, axis[two]] = np.where(keep[two] == 0, 1.0, keep[two])
    return o, d


def two_squares(gap):
    """Two parallel unit squares, z = 0 (faces 0, 1; normal +z) and z = gap (faces 2, 3; normal +z)."""
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    v = np.concatenate([sq, sq + np.array([0, 0, gap], np.float32)])
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    return v, f
