"""numpy reference of include/ts_color.h, operation by operation: colour integration in integers, the colour field, the trilinear sampler
that leaves out samples without data, and the interpolation of vertex attributes over a face_idx image.  Everything is float64 on fp32
inputs widened, every operation rounded (numpy float64 arrays never contract).  Positions, views and the analytic sphere are ref_volume's."""
from __future__ import annotations

import numpy as np

import ref_volume as ref

Q16 = 65536.0  # the fixed-point scale of the colour sums
INT32_MAX = ref.INT32_MAX
NAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def project(dims, origin, h, view, tan_fovx, tan_fovy, W, H, mask=None):
    """Steps 1-3 of the header for every sample: (ok, pix, z); pix is 0 where ok is False."""
    (p0, p1, p2), _ = ref.sample_positions(dims, origin, h)
    M = np.asarray(view, np.float32).astype(np.float64).reshape(4, 4)
    tx, ty = float(np.float32(tan_fovx)), float(np.float32(tan_fovy))
    with np.errstate(all="ignore"):
        v = [((p0 * M[0, c] + p1 * M[1, c]) + p2 * M[2, c]) + M[3, c] for c in range(3)]
        z = v[2]
        ok = np.isfinite(z) & (z > 0)
        col = np.floor((v[0] / (z * tx) + 1.0) * (0.5 * W))
        row = np.floor((v[1] / (z * ty) + 1.0) * (0.5 * H))
        ok &= (col >= 0) & (col < W) & (row >= 0) & (row < H)  # a NaN fails
        pix = np.where(ok, row * W + col, 0).astype(np.int64)
    if mask is not None:
        ok &= np.asarray(mask, np.uint8).reshape(-1)[pix] != 0
    return ok, pix, z


def in_band(dims, origin, h, trunc, view, tan_fovx, tan_fovy, W, H, depth, mask=None):
    """Steps 1-5: the samples whose pixel is covered (depth finite and > 0) and that lie within trunc of it; and pix."""
    ok, pix, z = project(dims, origin, h, view, tan_fovx, tan_fovy, W, H, mask)
    tr = float(np.float32(trunc))
    with np.errstate(all="ignore"):
        d = np.asarray(depth, np.float32).reshape(-1)[pix].astype(np.float64)
        sd = d - z
        ok = ok & np.isfinite(d) & (d > 0) & (sd >= -tr) & (sd <= tr)
    return ok, pix


def quantise(x):
    """(int64) rint(min(max(x, 0), 1) 65536) of finite values."""
    return np.rint(np.minimum(np.maximum(np.asarray(x, np.float64), 0.0), 1.0) * Q16).astype(np.int64)


def integrate(csum, cweight, dims, origin, h, trunc, view, tan_fovx, tan_fovy, W, H, depth, image, mask=None):
    """One view's colour into the state (csum (n, 3) int64, cweight (n,) int32, both updated in place).  Returns the number coloured."""
    ok, pix = in_band(dims, origin, h, trunc, view, tan_fovx, tan_fovy, W, H, depth, mask)
    x = np.asarray(image, np.float32).reshape(3, -1)[:, pix]  # (3, n)
    ok &= np.isfinite(x).all(axis=0)
    ok &= cweight != INT32_MAX
    q = quantise(np.where(ok[None, :], x, 0.0).astype(np.float64))
    csum[ok] += q[:, ok].T
    cweight[ok] += 1
    return int(ok.sum())


def color_field(csum, cweight, min_weight=1):
    """(3, n) float32, channel-planar."""
    with np.errstate(all="ignore"):
        f = (csum.astype(np.float64) / (cweight.astype(np.float64)[:, None] * Q16)).astype(np.float32)
    return np.ascontiguousarray(np.where((cweight >= min_weight)[:, None], f, NAN32).astype(np.float32).T)


def sample(grid, dims, origin, h, points):
    """grid (C, n) or (n,) float32; points (N, 3) float32.  Returns (out (N, C) float32, valid (N,) uint8)."""
    nx, ny, nz = dims
    n = nx * ny * nz
    g = np.asarray(grid, np.float32).reshape(-1, n)
    C = g.shape[0]
    pts = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    N = len(pts)
    o = np.asarray(origin, np.float32).astype(np.float64)
    hd = float(np.float32(h))
    has_data = np.isfinite(g).all(axis=0)
    with np.errstate(all="ignore"):
        gg = [(pts[:, a] - o[a]) / hd for a in range(3)]
        inside = np.ones(N, bool)
        for a in range(3):
            inside &= (gg[a] >= 0) & (gg[a] <= dims[a] - 1)  # a NaN fails
        b, t = [], []
        for a in range(3):
            ga = np.where(inside, gg[a], 0.0)
            ba = np.minimum(np.floor(ga).astype(np.int64), dims[a] - 2) if dims[a] >= 2 else np.zeros(N, np.int64)
            b.append(ba)
            t.append(ga - ba.astype(np.float64))
    den = np.zeros(N)
    num = np.zeros((C, N))
    first = np.ones(N, bool)
    for k in range(8):
        bits = (k & 1, k >> 1 & 1, k >> 2 & 1)
        if any(bits[a] and dims[a] < 2 for a in range(3)):
            continue  # the corner does not exist
        w = ((t[0] if bits[0] else 1.0 - t[0]) * (t[1] if bits[1] else 1.0 - t[1])) * (t[2] if bits[2] else 1.0 - t[2])
        idx = ((b[2] + bits[2]) * ny + (b[1] + bits[1])) * nx + (b[0] + bits[0])
        use = inside & has_data[idx]
        den = np.where(use, np.where(first, w, den + w), den)
        for c in range(C):
            term = w * np.where(use, g[c, idx], 0.0).astype(np.float64)
            num[c] = np.where(use, np.where(first, term, num[c] + term), num[c])
        first &= ~use
    valid = inside & (den > 0)
    with np.errstate(all="ignore"):
        out = np.where(valid[None, :], (num / np.where(valid, den, 1.0)[None, :]).astype(np.float32), NAN32).astype(np.float32)
    return np.ascontiguousarray(out.T), valid.astype(np.uint8)


def interpolate(view, tan_fovx, tan_fovy, W, H, vertices, faces, face_idx, attributes, background):
    """Returns (out (C, H, W) float32, bary (3, H, W) float32)."""
    M = np.asarray(view, np.float32).astype(np.float64).reshape(4, 4)
    tx, ty = float(np.float32(tan_fovx)), float(np.float32(tan_fovy))
    P = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    Fc = np.asarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    A = np.asarray(attributes, np.float32).astype(np.float64).reshape(len(P), -1)
    C = A.shape[1]
    V, F = len(P), len(Fc)
    fi = np.asarray(face_idx, np.int32).reshape(-1).astype(np.int64)
    drawn = (fi >= 0) & (fi < F)
    tri = Fc[np.where(drawn, fi, 0)] if F else np.zeros((len(fi), 3), np.int64)
    drawn &= ((tri >= 0) & (tri < V)).all(axis=1)
    tri = np.where(drawn[:, None], tri, 0)
    if V == 0:
        P, A = np.zeros((1, 3)), np.zeros((1, C))
    p = np.arange(W * H)
    col, row = (p % W).astype(np.float64), (p // W).astype(np.float64)
    with np.errstate(all="ignore"):
        corner = []
        for m in range(3):
            q = P[tri[:, m]]
            corner.append([((q[:, 0] * M[0, k] + q[:, 1] * M[1, k]) + q[:, 2] * M[2, k]) + M[3, k] for k in range(3)])
        a, b, c = corner
        r0 = ((col + 0.5) / (0.5 * W) - 1.0) * tx
        r1 = ((row + 0.5) / (0.5 * H) - 1.0) * ty

        def rdc(x, y):
            n0, n1, n2 = x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]
            return (r0 * n0 + r1 * n1) + n2

        wa, wb, wc = rdc(b, c), rdc(c, a), rdc(a, b)
        neg = (wa + wb) + wc < 0
        wa, wb, wc = (np.where(neg, -w, w) for w in (wa, wb, wc))
        wa, wb, wc = (np.where(w >= 0, w, 0.0) for w in (wa, wb, wc))
        s = (wa + wb) + wc
        good = np.isfinite(s) & (s > 0)
        third = 1.0 / 3.0
        al, be, ga = (np.where(good, w / np.where(good, s, 1.0), third) for w in (wa, wb, wc))
        out = np.empty((C, W * H), np.float32)
        bg = np.asarray(background, np.float32).reshape(-1)
        for ch in range(C):
            val = ((al * A[tri[:, 0], ch] + be * A[tri[:, 1], ch]) + ga * A[tri[:, 2], ch]).astype(np.float32)
            out[ch] = np.where(drawn, val, bg[ch])
        bary = np.stack([np.where(drawn, w.astype(np.float32), np.float32(0)) for w in (al, be, ga)]).astype(np.float32)
    return out.reshape(C, H, W), bary.reshape(3, H, W)


# ---- the analytic sphere with a colour ---------------------------------------------------------------------------------------------------
def sphere_color(points, radius=None):
    """0.5 + 0.4 n at points of a sphere about the origin, n the outward unit normal."""
    p = np.asarray(points, np.float64)
    return 0.5 + 0.4 * p / np.linalg.norm(p, axis=-1, keepdims=True)


def sphere_image(view, tan_fov, W, H, radius):
    """(3, H, W) float32: sphere_color at the hit point of every pixel-centre ray on the sphere of ref_volume.sphere_depth; 0 where it misses."""
    M = np.asarray(view, np.float32).astype(np.float64)
    R, t = M[:3, :3], M[3, :3]
    Rinv = np.linalg.inv(R)
    eye = -t @ Rinv
    depth = ref.sphere_depth(view, tan_fov, W, H, radius).astype(np.float64).reshape(-1)
    x = ((np.arange(W) + 0.5) / (0.5 * W) - 1.0) * tan_fov
    y = ((np.arange(H) + 0.5) / (0.5 * H) - 1.0) * tan_fov
    d_view = np.stack([np.broadcast_to(x[None, :], (H, W)), np.broadcast_to(y[:, None], (H, W)), np.ones((H, W))], axis=-1).reshape(-1, 3)
    hit = eye[None, :] + depth[:, None] * (d_view @ Rinv)
    with np.errstate(all="ignore"):
        colour = np.where((depth > 0)[:, None], sphere_color(hit), 0.0)
    return np.ascontiguousarray(colour.T.reshape(3, H, W).astype(np.float32))


def fuse_colored_sphere(order=range(6), radius=0.6, res=20, h=0.1, origin=-0.95, size=48, tan_fov=0.45):
    """ref_volume.fuse_sphere with carving, and the analytic colour of every view: (sum, weight, csum, cweight, dims, origin, h)."""
    dims = (res, res, res)
    n = res ** 3
    s, w = np.zeros(n, np.int64), np.zeros(n, np.int32)
    cs, cw = np.zeros((n, 3), np.int64), np.zeros(n, np.int32)
    trunc = np.float32(4) * np.float32(h)
    for v in order:
        M = ref.look_at_view(ref.AXIS_EYES[v])
        depth = ref.sphere_depth(M, tan_fov, size, size, radius)
        ref.integrate(s, w, dims, (origin,) * 3, h, trunc, M, tan_fov, tan_fov, size, size, depth, flags=ref.CARVE_UNCOVERED)
        integrate(cs, cw, dims, (origin,) * 3, h, trunc, M, tan_fov, tan_fov, size, size, depth, sphere_image(M, tan_fov, size, size, radius))
    return s, w, cs, cw, dims, (origin,) * 3, h
