"""Numpy reference of vertex welding and edge topology (include/ts_weld.h), brute force.

The pair test is evaluated exactly as the header states it, in float32 with every operation rounded (numpy never contracts):
    adjacent(i, j)  iff  i != j, all six coordinates finite, (dx*dx + dy*dy) + dz*dz <= eps*eps
over all O(V^2) pairs in blocks; then a plain union-find, the numbering by ascending label, both position modes, the face remap with its
keep mask, and the edge census by np.unique over (min, max) rows with the connected pieces."""
from __future__ import annotations

import numpy as np


def adjacent_pairs(vertices, eps, block=512):
    """(i, j) arrays with i < j of all adjacent pairs."""
    v = np.ascontiguousarray(vertices, np.float32)
    V = len(v)
    with np.errstate(over="ignore"):
        eps2 = np.float32(eps) * np.float32(eps)  # may overflow to inf, like the device's
    finite = np.isfinite(v).all(1)
    out_i, out_j = [], []
    with np.errstate(all="ignore"):
        for a in range(0, V, block):
            va = v[a:a + block]
            for b in range(a, V, block):
                vb = v[b:b + block]
                dx = va[:, None, 0] - vb[None, :, 0]
                dy = va[:, None, 1] - vb[None, :, 1]
                dz = va[:, None, 2] - vb[None, :, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                assert d2.dtype == np.float32
                hit = (d2 <= eps2) & finite[a:a + block, None] & finite[None, b:b + block]
                i, j = np.nonzero(hit)
                i, j = i + a, j + b
                sel = i < j
                out_i.append(i[sel]); out_j.append(j[sel])
    return np.concatenate(out_i) if out_i else np.zeros(0, np.int64), np.concatenate(out_j) if out_j else np.zeros(0, np.int64)


def _components(n, a, b):
    """label[i] = the smallest index of i's component under the edges (a[k], b[k])."""
    parent = np.arange(n, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for x, y in zip(a.tolist(), b.tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(i) for i in range(n)], np.int64)


def labels(vertices, eps):
    i, j = adjacent_pairs(vertices, eps)
    return _components(len(vertices), i, j)


def compact(label, vertices, position="first"):
    """(remap, welded vertices (V', 3) float32, V')."""
    v = np.ascontiguousarray(vertices, np.float32)
    roots = np.unique(label)
    remap = np.searchsorted(roots, label).astype(np.int64)
    if position == "first":
        out = v[roots].copy()
    else:
        out = np.zeros((len(roots), 3), np.float32)
        with np.errstate(all="ignore"):
            for r, root in enumerate(roots):
                members = np.nonzero(label == root)[0]  # ascending
                s = v[members[0]].astype(np.float64)
                for m in members[1:]:
                    s = s + v[m].astype(np.float64)
                out[r] = (s / np.float64(len(members))).astype(np.float32)
    return remap, out, len(roots)


def remap_faces(V, faces, remap):
    """(new faces (F, 3) int64 with -1 rows for faces that name no vertex, keep (F,) bool)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1)
    new = np.where(ok[:, None], np.asarray(remap, np.int64)[np.where(ok[:, None], f, 0)] if V else -1, -1)
    keep = ok & (new[:, 0] != new[:, 1]) & (new[:, 1] != new[:, 2]) & (new[:, 0] != new[:, 2])
    return new, keep


def weld(vertices, faces, eps, position="first"):
    lab = labels(vertices, eps)
    remap, out, n = compact(lab, vertices, position)
    new, keep = remap_faces(len(vertices), faces, remap)
    return {"label": lab, "remap": remap, "vertices": out, "num_vertices": n, "faces": new, "keep": keep,
            "largest_cluster": int(np.bincount(remap, minlength=max(n, 1)).max()) if len(lab) else 0}


def topology(V, faces, keep=None):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1)
    if keep is not None:
        ok &= np.asarray(keep, bool)
    f = f[ok]
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    e = np.stack([e.min(1), e.max(1)], 1)
    if len(e):
        uniq, count = np.unique(e, axis=0, return_counts=True)
    else:
        uniq, count = np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
    lab = _components(V, uniq[:, 0], uniq[:, 1])
    ref = np.unique(f)
    return {"edges": int(len(uniq)), "boundary": int((count == 1).sum()), "manifold": int((count == 2).sum()),
            "nonmanifold": int((count >= 3).sum()), "pieces": int(len(np.unique(lab[ref]))), "vertices_referenced": int(len(ref)),
            "faces": int(len(f)), "euler": int(len(ref)) - int(len(uniq)) + int(len(f)), "label": lab}


def same_partition(label_a, label_b):
    """Whether two labelings describe the same partition."""
    a, b = np.asarray(label_a, np.int64), np.asarray(label_b, np.int64)
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


# ---- the fixtures the CPU and GPU tests share ---------------------------------------------------------------------------------------------
def grid_soup(n=20, eps=1e-3, seed=0, origin=(0.0, 0.0, 0.0), rotation=None):
    """An n x n vertex grid with spacing 10 eps in the plane z = 0, turned by `rotation` (3 x 3, applied to row vectors) and moved to `origin`
    (the position of grid vertex 0), split into 2 (n - 1)^2 triangles, exploded to a soup whose every vertex is moved by less than eps / 4 per
    axis, the triangle order shuffled.  Returns (vertices (3 T, 3) float32, faces (T, 3) int64, grid_id (3 T,): the grid vertex every soup
    vertex came from)."""
    rng = np.random.default_rng(seed)
    gy, gx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    grid = np.stack([gx.reshape(-1) * 10.0 * eps, gy.reshape(-1) * 10.0 * eps, np.zeros(n * n)], 1)
    if rotation is not None:
        grid = grid @ np.asarray(rotation, np.float64)
    grid = grid + np.asarray(origin, np.float64)
    tris = []
    for y in range(n - 1):
        for x in range(n - 1):
            a, b, c, d = y * n + x, y * n + x + 1, (y + 1) * n + x, (y + 1) * n + x + 1
            tris += [(a, b, d), (a, d, c)]
    tris = np.array(tris, np.int64)[rng.permutation(len(tris))]
    grid_id = tris.reshape(-1)
    move = (rng.random((len(grid_id), 3)) * 2 - 1) * (eps * 0.24)
    vertices = (grid[grid_id] + move).astype(np.float32)
    return vertices, np.arange(len(grid_id), dtype=np.int64).reshape(-1, 3), grid_id


def rotation_xz(deg_x, deg_z):
    """Row-vector rotation: about x by deg_x, then about z by deg_z."""
    ax, az = np.deg2rad(deg_x), np.deg2rad(deg_z)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), np.sin(ax)], [0, -np.sin(ax), np.cos(ax)]])
    rz = np.array([[np.cos(az), np.sin(az), 0], [-np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return rx @ rz


# the jittered grid of the GPU tests, posed for the 70 x 37 camera of synthetic.camera (at z = 1200, looking down -z): centred on the optical
# axis at depth 1100, tilted so that no edge runs along a pixel row; a grid cell is about 3.6 pixels wide and part of the grid is off screen
GRID_EPS = 3.6
RENDER_W, RENDER_H = 70, 37


def posed_grid(seed=1):
    r = rotation_xz(35.0, 17.0)
    half = 9.5 * 10.0 * GRID_EPS
    origin = np.array([0.0, 0.0, 100.0]) - np.array([half, half, 0.0]) @ r
    return grid_soup(20, GRID_EPS, seed=seed, origin=origin, rotation=r)


def face_colors(F, seed=3):
    return np.random.default_rng(seed).random((F, 3), dtype=np.float32)
