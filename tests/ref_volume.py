"""numpy / plain-float reference of include/ts_volume.h, operation by operation: TSDF integration in integers, the field, and marching
tetrahedra with edge vertices that are functions of the edge alone.  Everything is float64 on fp32 inputs widened, every operation rounded
(Python floats and numpy float64 arrays never contract).  It defines the case table and derives the orientation (flip) table that
csrc/volume.hip carries as constants."""
from __future__ import annotations

import numpy as np

ONE = 1048576.0  # 2^20: the fixed-point scale of the sums
INT32_MAX = 2 ** 31 - 1
CARVE_UNCOVERED = 1

# the six tetrahedra of a cell: the axis permutations in lexicographic order, each a path 0 -> 7; corner c = bit0 x + bit1 y + bit2 z
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))


def case_triangles(mask):
    """The triangles of a tetrahedron whose vertex m (in tetrahedron order) is inside iff bit m of `mask` is set, before orientation: a list
    of triangles, each three edges (p, q) of positions 0..3 in the tetrahedron."""
    ins = [m for m in range(4) if mask >> m & 1]
    outs = [m for m in range(4) if not mask >> m & 1]
    if len(ins) == 1:
        return [tuple((ins[0], o) for o in outs)]
    if len(ins) == 3:
        return [tuple((outs[0], i) for i in ins)]
    if len(ins) == 2:
        (a, b), (c, d) = ins, outs
        q0, q1, q2, q3 = (a, c), (a, d), (b, d), (b, c)
        return [(q0, q1, q2), (q0, q2, q3)]
    return []


def _corner(c):
    return np.array([c & 1, c >> 1 & 1, c >> 2 & 1], np.int64)


def derive_flip_table():
    """FLIP[t] = 16 bits, bit `mask` set iff the triangles of (tetrahedron t, case mask) get their 2nd and 3rd vertices swapped so that the
    normal points from inside to outside.  Exact integers: vertices at the edge midpoints (doubled), the direction from the inside corners'
    centroid to the outside corners' (scaled).  The sign cannot change while a vertex slides along its edge: the triangle's plane separates
    the inside corners from the outside ones."""
    table = []
    for tet in TETS:
        bits = 0
        for mask in range(1, 15):
            ins = [tet[m] for m in range(4) if mask >> m & 1]
            outs = [tet[m] for m in range(4) if not mask >> m & 1]
            direction = len(ins) * sum(_corner(c) for c in outs) - len(outs) * sum(_corner(c) for c in ins)
            signs = set()
            for tri in case_triangles(mask):
                v = [_corner(tet[p]) + _corner(tet[q]) for p, q in tri]
                dot = int(np.cross(v[1] - v[0], v[2] - v[0]) @ direction)
                assert dot != 0
                signs.add(dot > 0)
            assert len(signs) == 1  # both halves of a quad agree
            if not signs.pop():
                bits |= 1 << mask
        table.append(bits)
    return tuple(table)


FLIP = derive_flip_table()
TRIANGLES_OF_CASE = tuple(len(case_triangles(m)) for m in range(16))


# ---- the volume ------------------------------------------------------------------------------------------------------------------------------
def sample_positions(dims, origin, h):
    """(p0, p1, p2) float64 arrays over the linear sample index (k ny + j) nx + i, and (i, j, k)."""
    nx, ny, nz = dims
    idx = np.arange(nx * ny * nz, dtype=np.int64)
    ijk = (idx % nx, (idx // nx) % ny, idx // (nx * ny))
    o = np.asarray(origin, np.float32).astype(np.float64)
    hd = float(np.float32(h))
    return tuple(o[a] + hd * ijk[a].astype(np.float64) for a in range(3)), ijk


def integrate(sum_, weight, dims, origin, h, trunc, view, tan_fovx, tan_fovy, W, H, depth, mask=None, flags=0):
    """One view into the state (sum_ int64, weight int32, both updated in place).  Returns the number of samples updated."""
    (p0, p1, p2), _ = sample_positions(dims, origin, h)
    M = np.asarray(view, np.float32).astype(np.float64).reshape(4, 4)
    depth = np.asarray(depth, np.float32).reshape(-1)
    tr = float(np.float32(trunc))
    tx, ty = float(np.float32(tan_fovx)), float(np.float32(tan_fovy))
    with np.errstate(all="ignore"):
        v = [((p0 * M[0, c] + p1 * M[1, c]) + p2 * M[2, c]) + M[3, c] for c in range(3)]
        z = v[2]
        ok = np.isfinite(z) & (z > 0)
        u = (v[0] / (z * tx) + 1.0) * (0.5 * W)
        w = (v[1] / (z * ty) + 1.0) * (0.5 * H)
        col, row = np.floor(u), np.floor(w)
        ok &= (col >= 0) & (col < W) & (row >= 0) & (row < H)  # a NaN fails
        pix = np.where(ok, row * W + col, 0).astype(np.int64)
        if mask is not None:
            ok &= np.asarray(mask, np.uint8).reshape(-1)[pix] != 0
        d = depth[pix].astype(np.float64)
        ok &= np.isfinite(d) & (d >= 0)
        uncovered = d == 0
        sd = d - z
        s = np.minimum(sd / tr, 1.0)
        q = np.rint(s * ONE)
        ok &= np.where(uncovered, bool(flags & CARVE_UNCOVERED), ~(sd < -tr))
        q = np.where(uncovered, ONE, q)
        ok &= weight != INT32_MAX
    sum_[ok] += q[ok].astype(np.int64)
    weight[ok] += 1
    return int(ok.sum())


def field(sum_, weight, min_weight=1):
    with np.errstate(all="ignore"):
        f = (sum_.astype(np.float64) / (weight.astype(np.float64) * ONE)).astype(np.float32)
    return np.where(weight >= min_weight, f, np.float32(np.nan)).astype(np.float32)


# ---- marching tetrahedra -----------------------------------------------------------------------------------------------------------------------
def extract(fld, dims, origin, h, iso=0.0):
    """(triangles (T, 3, 3) float32, cell (T,) int32): the soup in ascending cell index (the linear sample index of the cell's corner 0),
    then tetrahedron, then case order."""
    nx, ny, nz = dims
    f = np.asarray(fld, np.float32).reshape(-1)
    assert f.size == nx * ny * nz
    o = [float(x) for x in np.asarray(origin, np.float32)]
    hd = float(np.float32(h))
    iso = float(np.float32(iso))
    tris, cells = [], []
    if min(dims) < 2:
        return np.zeros((0, 3, 3), np.float32), np.zeros((0,), np.int32)
    step = (1, nx, nx * ny)
    offs = np.array([(c & 1) + (c >> 1 & 1) * nx + (c >> 2 & 1) * nx * ny for c in range(8)], np.int64)
    vol = f.reshape(nz, ny, nx)
    finite = np.isfinite(vol)
    inside = finite & (vol < np.float32(iso))
    act = np.ones((nz - 1, ny - 1, nx - 1), bool)
    any_in = np.zeros_like(act)
    all_in = np.ones_like(act)
    for c in range(8):
        sl = (slice(c >> 2 & 1, nz - 1 + (c >> 2 & 1)), slice(c >> 1 & 1, ny - 1 + (c >> 1 & 1)), slice(c & 1, nx - 1 + (c & 1)))
        act &= finite[sl]
        any_in |= inside[sl]
        all_in &= inside[sl]
    ks, js, is_ = np.nonzero(act & any_in & ~all_in)  # ascending cell index

    def vertex(a, b):
        if a > b:
            a, b = b, a
        fa, fb = float(f[a]), float(f[b])
        t = (iso - fa) / (fb - fa)
        out = []
        for axis in range(3):
            ga = (a // step[axis]) % dims[axis]
            gb = (b // step[axis]) % dims[axis]
            g = float(ga) + t * (float(gb) - float(ga))
            out.append(np.float32(o[axis] + hd * g))
        return out

    for k, j, i in zip(ks.tolist(), js.tolist(), is_.tolist()):
        base = (k * ny + j) * nx + i
        corner = base + offs
        for t, tet in enumerate(TETS):
            s = [int(corner[c]) for c in tet]
            mask = sum(1 << m for m in range(4) if float(f[s[m]]) < iso)
            flip = FLIP[t] >> mask & 1
            for tri in case_triangles(mask):
                v = [vertex(s[p], s[q]) for p, q in tri]
                if flip:
                    v[1], v[2] = v[2], v[1]
                tris.append(v)
                cells.append(base)
    return np.array(tris, np.float32).reshape(-1, 3, 3), np.array(cells, np.int32)


# ---- what the tests measure --------------------------------------------------------------------------------------------------------------------
def weld_exact(triangles):
    """(vertices (V, 3), faces (T, 3)): vertices with equal bits merged (-0 and +0 are equal here, as for weld_mesh(eps=0))."""
    pts = triangles.reshape(-1, 3) + np.float32(0.0)
    verts, inverse = np.unique(pts, axis=0, return_inverse=True)
    return verts, inverse.reshape(-1, 3).astype(np.int64)


def topology(faces):
    """dict: vertices, edges, faces, boundary (edges used once), nonmanifold (three or more), directed_repeats (directed edges that appear
    more than once), euler."""
    und = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    _, counts = np.unique(und, axis=0, return_counts=True)
    directed = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    _, dcounts = np.unique(directed, axis=0, return_counts=True)
    V, E, F = len(np.unique(faces)), len(counts), len(faces)
    return {"vertices": V, "edges": E, "faces": F, "boundary": int((counts == 1).sum()), "nonmanifold": int((counts >= 3).sum()),
            "directed_repeats": int((dcounts > 1).sum()), "euler": V - E + F}


def signed_volume(triangles):
    t = triangles.astype(np.float64)
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


def sphere_field(dims, centre, radius):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d = np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2)
    return (d - radius).astype(np.float32).reshape(-1)


def torus_field(dims, centre, major, minor):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ring = np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2) - major
    return (np.sqrt(ring ** 2 + (k - centre[2]) ** 2) - minor).astype(np.float32).reshape(-1)


# ---- analytic views of a sphere at the origin ----------------------------------------------------------------------------------------------------
def look_at_view(eye):
    """world_view_transform (4, 4) float32, row-vector convention (view = [p, 1] @ M), of a camera at `eye` looking at the origin, +z forward."""
    eye = np.asarray(eye, np.float64)
    fwd = -eye / np.linalg.norm(eye)
    up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(up, fwd)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd], axis=1)  # columns: the view axes in world coordinates
    M = np.eye(4)
    M[:3, :3] = R
    M[3, :3] = -eye @ R
    return M.astype(np.float32)


AXIS_EYES = ((3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, -3, 0), (0, 0, 3), (0, 0, -3))


def sphere_depth(view, tan_fov, W, H, radius):
    """View-space depth of the unit-view-depth pixel-centre rays on a sphere at the world origin; 0 where the ray misses."""
    M = np.asarray(view, np.float32).astype(np.float64)
    R, t = M[:3, :3], M[3, :3]
    eye = -t @ np.linalg.inv(R)
    x = ((np.arange(W) + 0.5) / (0.5 * W) - 1.0) * tan_fov
    y = ((np.arange(H) + 0.5) / (0.5 * H) - 1.0) * tan_fov
    d_view = np.stack([np.broadcast_to(x[None, :], (H, W)), np.broadcast_to(y[:, None], (H, W)), np.ones((H, W))], axis=-1).reshape(-1, 3)
    d = d_view @ np.linalg.inv(R)
    a = (d * d).sum(axis=1)
    b = 2.0 * (d @ eye)
    c = eye @ eye - radius * radius
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        tt = (-b - np.sqrt(disc)) / (2 * a)
    return np.where(disc > 0, tt, 0.0).astype(np.float32).reshape(H, W)


def fuse_sphere(order=range(6), carve=True, radius=0.6, res=20, h=0.1, origin=-0.95, size=48, tan_fov=0.45):
    dims = (res, res, res)
    n = res ** 3
    s, w = np.zeros(n, np.int64), np.zeros(n, np.int32)
    trunc = np.float32(4) * np.float32(h)
    for v in order:
        M = look_at_view(AXIS_EYES[v])
        integrate(s, w, dims, (origin,) * 3, h, trunc, M, tan_fov, tan_fov, size, size, sphere_depth(M, tan_fov, size, size, radius),
                  flags=CARVE_UNCOVERED if carve else 0)
    return s, w, dims, (origin,) * 3, h
