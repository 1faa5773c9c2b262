"""Brute-force float64 checker of the opaque mesh renderer (include/ts_mesh.h, DESIGN.md "Opaque mesh renderer"), numpy only.

Semantics restated: view space p_view = [p, 1] @ view; a face is valid iff its three vertices have depth > znear; screen position
x = (x_v / (z_v tan_fovx) + 1) W / 2 (y alike), pixel centre (i + .5, j + .5); a pixel is covered when its centre lies inside or on the
projected triangle; depth there = ray / plane intersection (n . a) / (n . r); winner = smallest depth > 0, ties to the smaller index.

Besides the images, `render` says where float32 may legitimately decide otherwise.  Two constants, which are conditions and not tuned
results (float32 evaluation of the same formulas stays >= 14x / >= 200x inside them):
    DELTA = 1e-2 px   a pixel centre this close to an edge may fall on either side of it
    EPS_C = 1e-5      the depth of face f is known to d (1 +- eps_f), eps_f = EPS_C / max(|cos_f|, 1e-4), cos_f = cosine between the face
                      normal and the ray to its centroid (the error grows as the face turns edge-on)
A pixel is AMBIGUOUS when (a) its centre is within DELTA of the boundary of a valid face whose depth interval reaches the winner's (on an
uncovered pixel: of any valid face), or (b) a covering face other than the winner (and its coincident reversed twin) has a depth interval
that reaches the winner's.  For every ambiguous pixel the checker lists the CANDIDATES: the faces that cover it or come within DELTA,
whose interval is not wholly behind the interval of a face that covers it for certain (by more than DELTA); -1 ("uncovered") is a
candidate when no face covers the pixel for certain.  On a non-ambiguous pixel the only candidate is the winner (or its twin).
"""
from __future__ import annotations

import numpy as np

DELTA = 1e-2
EPS_C = 1e-5
MAX_AMBIGUOUS_SHARE = 0.05  # a comparison may leave out at most this share of a scene's pixels


def scene_mesh(s, twins: bool, seed: int):
    """(vertices, faces, colors) of a synthetic.scene: un-shared vertices, faces arange(3P).reshape(P, 3), with `twins` the same rows reversed
    and appended; colours default_rng(seed).random((F, 3), float32)."""
    P = s["vertex"].shape[0]
    vertices = np.ascontiguousarray(s["vertex"].reshape(-1, 3), np.float32)
    faces = np.arange(3 * P, dtype=np.int64).reshape(P, 3)
    if twins:
        faces = np.concatenate([faces, faces[:, ::-1]], 0)
    colors = np.random.default_rng(seed).random((len(faces), 3), dtype=np.float32)
    return vertices, faces, colors


def _setup(vertices, faces, W, H, tx, ty, view, znear):
    view = np.asarray(view, np.float64)
    V = np.asarray(vertices, np.float64)
    faces = np.asarray(faces, np.int64)
    inb = ((faces >= 0) & (faces < len(V))).all(1)
    vv = (V @ view[:3, :3] + view[3, :3])[np.where(inb[:, None], faces, 0)]  # (F, 3, 3)
    valid = inb & (vv[:, :, 2] > znear).all(1)
    with np.errstate(all="ignore"):
        sx = (vv[:, :, 0] / (vv[:, :, 2] * tx) + 1) * W / 2
        sy = (vv[:, :, 1] / (vv[:, :, 2] * ty) + 1) * H / 2
    return vv, valid, sx, sy


def _visit(vv, valid, sx, sy, W, H, tx, ty):
    """Per valid face: its index, the slice of pixels its DELTA-widened bounding box holds, the signed distance of their centres to its
    boundary (>= 0 inside), the ray / plane depth there, where that depth is usable, and eps_f."""
    for f in np.nonzero(valid)[0]:
        x, y = sx[f], sy[f]
        x0 = max(int(np.floor(x.min() - 0.5 - DELTA)), 0); x1 = min(int(np.ceil(x.max() - 0.5 + DELTA)), W - 1)
        y0 = max(int(np.floor(y.min() - 0.5 - DELTA)), 0); y1 = min(int(np.ceil(y.max() - 0.5 + DELTA)), H - 1)
        if x1 < x0 or y1 < y0:
            continue
        area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
        if abs(area) < 1e-12:
            continue
        px = np.arange(x0, x1 + 1)[None, :] + 0.5
        py = np.arange(y0, y1 + 1)[:, None] + 0.5
        sgn, dmin = np.sign(area), None
        for i in range(3):
            j = (i + 1) % 3
            ex, ey = x[j] - x[i], y[j] - y[i]
            dd = sgn * (ex * (py - y[i]) - ey * (px - x[i])) / np.hypot(ex, ey)
            dmin = dd if dmin is None else np.minimum(dmin, dd)
        a, b, c = vv[f]
        n = np.cross(b - a, c - a)
        cen = vv[f].mean(0)
        cos = abs(n @ cen) / (np.linalg.norm(n) * np.linalg.norm(cen))
        epsf = EPS_C / max(cos, 1e-4)
        with np.errstate(all="ignore"):
            d = (n @ a) / (n[0] * ((px * 2 / W - 1) * tx) + n[1] * ((py * 2 / H - 1) * ty) + n[2])
        ok = np.isfinite(d) & (d > 0)
        yield f, (slice(y0, y1 + 1), slice(x0, x1 + 1)), dmin, d, ok, epsf


def render(vertices, faces, colors, W, H, tan_fovx, tan_fovy, view, znear=1.0, background=(0.0, 0.0, 0.0), twin_period=None):
    """twin_period = P: faces f and f + P are coincident reversed twins (either may win a pixel; they never make one ambiguous)."""
    vv, valid, sx, sy = _setup(vertices, faces, W, H, tan_fovx, tan_fovy, view, znear)
    F = len(vv)
    same = (lambda idx, f: idx % twin_period == f % twin_period) if twin_period else (lambda idx, f: idx == f)
    best = np.full((H, W), np.inf); idx = np.full((H, W), -1, np.int64); hi = np.full((H, W), np.inf)
    eps = np.zeros(F)
    for f, sl, dmin, d, ok, epsf in _visit(vv, valid, sx, sy, W, H, tan_fovx, tan_fovy):
        eps[f] = epsf
        closer = (dmin >= 0) & ok & (d < best[sl])  # ascending f and a strict `<`: ties stay with the smaller index
        idx[sl] = np.where(closer, f, idx[sl]); hi[sl] = np.where(closer, d * (1 + epsf), hi[sl]); best[sl] = np.where(closer, d, best[sl])
    amb = np.zeros((H, W), bool)
    certain_hi = np.full((H, W), np.inf)  # the nearest upper interval end among the faces that cover the pixel for certain
    for f, sl, dmin, d, ok, epsf in _visit(vv, valid, sx, sy, W, H, tan_fovx, tan_fovy):
        lo = d * (1 - epsf)
        amb[sl] |= (dmin >= 0) & ok & ~same(idx[sl], f) & (lo <= hi[sl])  # (b)
        amb[sl] |= (np.abs(dmin) < DELTA) & ok & (lo <= hi[sl])          # (a); hi = inf on uncovered pixels
        certain_hi[sl] = np.where((dmin >= DELTA) & ok, np.minimum(certain_hi[sl], d * (1 + epsf)), certain_hi[sl])
    candidates = {}
    for f, sl, dmin, d, ok, epsf in _visit(vv, valid, sx, sy, W, H, tan_fovx, tan_fovy):
        can = amb[sl] & (dmin > -DELTA) & ok & (d * (1 - epsf) <= certain_hi[sl])
        if can.any():
            ys, xs = np.nonzero(can)
            for yy, xx in zip(ys + sl[0].start, xs + sl[1].start):
                candidates.setdefault((int(yy), int(xx)), set()).add(int(f))
    for yy, xx in zip(*np.nonzero(amb)):
        c = candidates.setdefault((int(yy), int(xx)), set())
        if not np.isfinite(certain_hi[yy, xx]):
            c.add(-1)
        if idx[yy, xx] >= 0:
            c.add(int(idx[yy, xx]))
    mask = idx >= 0
    colors = np.asarray(colors, np.float64)
    bg = np.asarray(background, np.float64)
    img = np.where(mask[None], colors[np.maximum(idx, 0)].transpose(2, 0, 1) if F else 0.0, bg[:, None, None])
    return {"face_idx": idx, "depth": np.where(mask, best, 0.0), "mask": mask, "render": np.clip(img, 0.0, 1.0), "ambiguous": amb,
            "candidates": candidates, "eps": eps, "valid": valid, "view_vertices": vv}


def render_scene(s, vertices, faces, colors, znear=1.0, twin_period=None):
    return render(vertices, faces, colors, s["image_width"], s["image_height"], s["tanfovx"], s["tanfovy"], s["viewmatrix"], znear,
                  s["background"], twin_period)


SCENES = {  # name: (synthetic.scene arguments, twins, colour seed)
    "A": (dict(P=3000, W=160, H=120, seed=11, edge_px=14.0), True),
    "B": (dict(P=20000, W=256, H=192, seed=12, edge_px=6.0), False),
    "C": (dict(P=5000, W=200, H=150, seed=13, edge_px=10.0, mode="centered"), True),
    "D": (dict(P=300, W=192, H=128, seed=14, mode="maincu"), False),
}


def build_scene(name):
    import synthetic
    kw, twins = SCENES[name]
    s = synthetic.scene(D=0, with_grads=False, **kw)
    vertices, faces, colors = scene_mesh(s, twins, kw["seed"])
    return s, vertices, faces, colors, (kw["P"] if twins else None)
