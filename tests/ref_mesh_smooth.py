"""numpy float64 reference of include/ts_smooth.h: the one-ring adjacency, Taubin lambda|mu smoothing, face and vertex normals, written
operation by operation.  Every elementwise numpy operation below rounds once, like the kernels built with -ffp-contract=off; the sequential
sums are np.add.at, which applies its updates one by one in the order given (a real left-to-right sum per destination, never np.sum).
np.sqrt and the division of float64 are the correctly rounded IEEE operations.
"""
import numpy as np

ISOLATED, INTERIOR, BOUNDARY, NONMANIFOLD = 0, 1, 2, 3
FIXED, CURVE, FREE = 0, 1, 2
BOUNDARY_MODES = {"fixed": FIXED, "curve": CURVE, "free": FREE}
AREA, UNIFORM = 0, 1
WEIGHTINGS = {"area": AREA, "uniform": UNIFORM}


def _faces(faces):
    return np.asarray(faces, np.int64).reshape(-1, 3)


def _kept(faces, keep):
    return np.ones(len(faces), bool) if keep is None else np.asarray(keep).reshape(len(faces)) != 0


# ---- adjacency ----------------------------------------------------------------------------------------------------------------------------
def adjacency(V, faces, keep=None):
    """dict: offsets (V + 1,) int32, neighbors / edge_faces (6 F,) int32 (-1 / 0 from offsets[V] on), vertex_class (V,) uint8,
    counts [entries, boundary, manifold, nonmanifold]."""
    f = _faces(faces)
    F = len(f)
    part = _kept(f, keep) & ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    p = f[part]
    src = np.concatenate([p[:, 0], p[:, 1], p[:, 1], p[:, 2], p[:, 2], p[:, 0]])
    dst = np.concatenate([p[:, 1], p[:, 0], p[:, 2], p[:, 1], p[:, 0], p[:, 2]])
    key, uses = np.unique(src * (V + 1) + dst, return_counts=True)  # ascending (src, dst)
    row, col = key // (V + 1), key % (V + 1)
    entries = len(key)
    neighbors = np.full(6 * F, -1, np.int32)
    edge_faces = np.zeros(6 * F, np.int32)
    neighbors[:entries], edge_faces[:entries] = col, uses
    offsets = np.searchsorted(row, np.arange(V + 1), side="left").astype(np.int32)
    degree = np.diff(offsets)
    one, many = np.zeros(V, bool), np.zeros(V, bool)
    one[row[uses == 1]] = True
    many[row[uses >= 3]] = True
    cls = np.where(degree == 0, ISOLATED, np.where(many, NONMANIFOLD, np.where(one, BOUNDARY, INTERIOR))).astype(np.uint8)
    counts = [entries, int((uses == 1).sum()), int((uses == 2).sum()), int((uses >= 3).sum())]
    return {"offsets": offsets, "neighbors": neighbors, "edge_faces": edge_faces, "vertex_class": cls, "counts": counts}


# ---- smoothing ----------------------------------------------------------------------------------------------------------------------------
def stencils(vertices, adj, mode=FIXED, pinned=None):
    """(stencil (V,) 0 none / 1 whole row / 2 boundary entries only, live (V,) bool)."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    V = len(v)
    live = np.isfinite(v).all(1)
    cls = np.asarray(adj["vertex_class"])
    free = live & (cls != ISOLATED)
    if pinned is not None:
        free &= np.asarray(pinned).reshape(V) == 0
    st = np.zeros(V, np.uint8)
    if mode == FREE:
        st[free] = 1
    else:
        st[free & (cls == INTERIOR)] = 1
        if mode == CURVE:
            st[free & (cls == BOUNDARY)] = 2
    return st, live


def smooth(vertices, adj, iterations=10, lam=0.5, mu=-0.53, mode=FIXED, pinned=None, max_move=np.inf):
    """(V, 3) float32: `iterations` times the step with lam and the step with mu on the float64 state, rounded once at the end."""
    v32 = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    V = len(v32)
    st, live = stencils(v32, adj, mode, pinned)
    offsets = np.asarray(adj["offsets"], np.int64)
    entries = int(offsets[V]) if V else 0
    row = np.repeat(np.arange(V), np.diff(offsets))
    col = np.asarray(adj["neighbors"], np.int64)[:entries]
    uses = np.asarray(adj["edge_faces"], np.int64)[:entries]
    use = (st[row] != 0) & live[col] & ((st[row] != 2) | (uses == 1))  # the stencil's live members, in ascending neighbour order per row
    row, col = row[use], col[use]
    n = np.bincount(row, minlength=V)
    moving = n > 0
    q0 = v32.astype(np.float64)
    q = q0.copy()
    with np.errstate(all="ignore"):
        for _ in range(int(iterations)):
            for k in (np.float64(np.float32(lam)), np.float64(np.float32(mu))):
                s = np.zeros((V, 3))
                np.add.at(s, row, q[col])
                m = s / n.astype(np.float64)[:, None]
                d = m - q
                q = np.where(moving[:, None], q + k * d, q)
        mm = np.float64(np.float32(max_move))
        out = np.minimum(np.maximum(q, q0 - mm), q0 + mm).astype(np.float32)
    return np.where((st != 0)[:, None], out.view(np.uint32), v32.view(np.uint32)).view(np.float32)


# ---- normals ------------------------------------------------------------------------------------------------------------------------------
def _cross(vertices, faces, keep=None):
    """(n (F, 3) float64, part (F,) bool): the cross product of every face (zeros where it does not take part)."""
    v32 = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    V = len(v32)
    f = _faces(faces)
    part = _kept(f, keep) & ((f >= 0) & (f < V)).all(1)
    fs = np.where(part[:, None], f, 0)
    p = v32.astype(np.float64)[fs] if V else np.zeros((len(f), 3, 3))
    with np.errstate(all="ignore"):
        part &= np.isfinite(p).all((1, 2))
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                      e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    return np.where(part[:, None], n, 0.0), part


def _unit(n):
    """(u (N, 3) float64, valid (N,) bool): n / sqrt(l2) where l2 = (nx nx + ny ny) + nz nz is finite and > 0, else zeros."""
    with np.errstate(all="ignore"):
        l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        valid = np.isfinite(l2) & (l2 > 0.0)
        u = n / np.sqrt(np.where(valid, l2, 1.0))[:, None]
    return np.where(valid[:, None], u, 0.0), valid


def face_normals(vertices, faces, keep=None):
    """(normals (F, 3) float32, valid (F,) uint8)."""
    n, part = _cross(vertices, faces, keep)
    u, valid = _unit(n)
    valid &= part
    return np.where(valid[:, None], u, 0.0).astype(np.float32), valid.astype(np.uint8)


def vertex_normals(vertices, faces, weighting=AREA, keep=None):
    """(normals (V, 3) float32, valid (V,) uint8, normal_sum (V, 3) float64)."""
    V = len(np.asarray(vertices).reshape(-1, 3))
    f = _faces(faces)
    n, part = _cross(vertices, f, keep)
    term = n
    if weighting == UNIFORM:
        term, ok = _unit(n)
        part = part & ok
    first = [part, part & (f[:, 1] != f[:, 0]), part & (f[:, 2] != f[:, 0]) & (f[:, 2] != f[:, 1])]  # a face counts once for a vertex
    rec_f = np.concatenate([np.nonzero(t)[0] for t in first])
    rec_v = np.concatenate([f[t, k] for k, t in enumerate(first)])
    order = np.lexsort((rec_f, rec_v))  # per vertex, ascending face index
    s = np.zeros((V, 3))
    with np.errstate(all="ignore"):
        np.add.at(s, rec_v[order], term[rec_f[order]])
    u, valid = _unit(s)
    return u.astype(np.float32), valid.astype(np.uint8), s


# ---- what the tests measure ---------------------------------------------------------------------------------------------------------------
def centroid(vertices):
    """The float64 mean of the vertices: the centre the radial figures of the sphere fixture are taken about (the CLEAN sphere's, for
    every row of the table in DESIGN.md 16j)."""
    return np.asarray(vertices, np.float64).mean(0)


def noisy(vertices, sigma=0.15, seed=7):
    """The fixture's noise: N(0, sigma) per coordinate from default_rng(seed), added in float64, rounded to fp32."""
    v = np.asarray(vertices, np.float32)
    return (v.astype(np.float64) + np.random.default_rng(seed).normal(0.0, sigma, v.shape)).astype(np.float32)


def radial_std(vertices, centre):
    return float(np.linalg.norm(np.asarray(vertices, np.float64) - centre, axis=1).std())


def normal_dot_radial(vertices, faces, centre):
    """(mean over the valid faces of face normal . unit(face centroid - centre), the number of faces where it is negative)."""
    n, valid = face_normals(vertices, faces)
    c = np.asarray(vertices, np.float64)[_faces(faces)].mean(1) - centre
    dots = (n.astype(np.float64) * (c / np.linalg.norm(c, axis=1, keepdims=True))).sum(1)[valid != 0]
    return float(dots.mean()), int((dots < 0).sum())


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)
