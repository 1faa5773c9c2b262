"""numpy reference of include/ts_winding.h and diff_recon_hip/mesh_winding.py: the generalised winding number by brute force over the
eligible faces, the node moments of the tree that a leaf-face table restates, and the tree form with its far-field terms, in float64 with
the header's operation order (numpy rounds every operation; only arctan2 may differ from the device's by a few ulp).  Every sum is the
int64 sum of quantised terms in units of 2^-38 turns.  Plain and slow on purpose; nothing here is shared with the code under test."""
import numpy as np

import ref_mesh_surface as refs

PI = np.float64(np.pi)  # the double nearest pi
UNIT = 2.0 ** 38        # units per turn
BAD = np.iinfo(np.int64).min
LEAF = FAN = 8
MAX_FACES = 2 ** 24 - 1


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def max2(x, y):
    return np.where(y > x, y, x)


def quantise(x):
    return np.rint(x).astype(np.int64)  # round half to even


def face_terms(q, tri):
    """(Q, n) int64: the quantised term of every face tri (n, 3, 3) float64 seen from every query q (Q, 3) float64."""
    a, b, c = (tri[None, :, k, :] - q[:, None, :] for k in range(3))
    la, lb, lc = np.sqrt(dot(a, a)), np.sqrt(dot(b, b)), np.sqrt(dot(c, c))
    det = dot(a, cross(b, c))
    den = ((la * lb) * lc + dot(a, b) * lc) + (dot(b, c) * la + dot(c, a) * lb)
    theta = np.where(det == 0, 0.0, np.arctan2(det, den))
    return quantise((theta / PI) * 2.0 ** 37)


def _points(points):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    return p.astype(np.float64), np.isfinite(p).all(axis=1)


def winding_exact(points, v, f, keep=None, chunk=256):
    """wq (Q,) int64: brute force over the eligible faces; INT64_MIN for a point with a non-finite coordinate."""
    q, good = _points(points)
    v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    wq = np.zeros(len(q), np.int64)
    ids = refs.eligible_faces(v, f, keep)
    if len(ids):
        tri = v[f[ids]].astype(np.float64)
        todo = np.nonzero(good)[0]
        for s in range(0, len(todo), chunk):
            e = todo[s:s + chunk]
            wq[e] = face_terms(q[e], tri).sum(axis=1)
    wq[~good] = BAD
    return wq


def to_turns(wq):
    """w float64 = wq 2^-38, NaN for a bad point."""
    wq = np.asarray(wq, np.int64)
    return np.where(wq == BAD, np.nan, wq.astype(np.float64) / UNIT)


class Tree:
    """The implicit 8-ary tree that `leaf_faces` (8 face ids per leaf, -1 for none) restates: per level the node count and the offset of
    its first node; per node the box (exact fp32 minima and maxima, (+inf, -inf) when empty) and the record [N, p, R2, S]."""

    def __init__(self, v, f, leaf_faces):
        v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
        lf = np.asarray(leaf_faces, np.int64).reshape(-1, LEAF)
        self.leaf_faces = lf
        self.tri = v[f[np.where(lf >= 0, lf, 0)]].astype(np.float64) if len(lf) else np.zeros((0, LEAF, 3, 3))  # (nleaves, 8, 3, 3)
        self.count, self.offset = [], []
        c, total = len(lf), 0
        while c > 0:
            self.count.append(c)
            self.offset.append(total)
            total += c
            if c == 1:
                break
            c = (c + FAN - 1) // FAN
        self.total = total
        lo, hi = np.full((total, 3), np.inf), np.full((total, 3), -np.inf)
        N, M, S = np.zeros((total, 3)), np.zeros((total, 3)), np.zeros(total)
        n0 = len(lf)
        for j in range(LEAF):  # slot order
            ok = lf[:, j] >= 0
            A, B, C = self.tri[:, j, 0], self.tri[:, j, 1], self.tri[:, j, 2]
            n = 0.5 * cross(B - A, C - A)
            ar = np.sqrt(dot(n, n))
            g = ((A + B) + C) / 3.0
            N[:n0] = np.where(ok[:, None], N[:n0] + n, N[:n0])
            S[:n0] = np.where(ok, S[:n0] + ar, S[:n0])
            M[:n0] = np.where(ok[:, None], M[:n0] + ar[:, None] * g, M[:n0])
            lo[:n0] = np.where(ok[:, None], np.minimum(lo[:n0], self.tri[:, j].min(axis=1)), lo[:n0])
            hi[:n0] = np.where(ok[:, None], np.maximum(hi[:n0], self.tri[:, j].max(axis=1)), hi[:n0])
        for l in range(1, len(self.count)):
            o, ob, cnt, below = self.offset[l], self.offset[l - 1], self.count[l], self.count[l - 1]
            for c in range(FAN):  # index order
                child = np.arange(cnt) * FAN + c
                ok = child < below
                src = ob + np.where(ok, child, 0)
                N[o:o + cnt] = np.where(ok[:, None], N[o:o + cnt] + N[src], N[o:o + cnt])
                S[o:o + cnt] = np.where(ok, S[o:o + cnt] + S[src], S[o:o + cnt])
                M[o:o + cnt] = np.where(ok[:, None], M[o:o + cnt] + M[src], M[o:o + cnt])
                lo[o:o + cnt] = np.where(ok[:, None], np.minimum(lo[o:o + cnt], lo[src]), lo[o:o + cnt])
                hi[o:o + cnt] = np.where(ok[:, None], np.maximum(hi[o:o + cnt], hi[src]), hi[o:o + cnt])
        has = S > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            p = np.where(has[:, None], M / np.where(has, S, 1.0)[:, None], 0.0)
            e = max2(p - lo, hi - p)
            R2 = np.where(has, dot(e, e), np.inf)
        self.lo, self.hi = lo, hi
        self.moments = np.concatenate([N, p, R2[:, None], S[:, None]], axis=1)  # (total, 8)


def moments(v, f, leaf_faces):
    """(nodes, 8) float64: [Nx, Ny, Nz, px, py, pz, R2, S] of every node, level 0 first."""
    return Tree(v, f, leaf_faces).moments


def winding_tree(points, v, f, leaf_faces, beta):
    """(wq (Q,) int64, terms (Q, 2) int32: faces evaluated, nodes accepted) of the header's walk on the tree of `leaf_faces`."""
    q, good = _points(points)
    t = Tree(v, f, leaf_faces)
    wq, terms = np.zeros(len(q), np.int64), np.zeros((len(q), 2), np.int32)
    beta2 = np.float64(beta) * np.float64(beta)

    def visit(level, k, idx):
        at = t.offset[level] + k
        if t.lo[at, 0] > t.hi[at, 0]:
            return
        m = t.moments[at]
        if m[7] > 0:
            r = m[3:6] - q[idx]
            d2 = dot(r, r)
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                accepted = d2 > beta2 * m[6]
                term = ((dot(m[0:3], r) / (d2 * np.sqrt(d2))) / (4.0 * PI)) * UNIT
            wq[idx[accepted]] += quantise(term[accepted])
            terms[idx[accepted], 1] += 1
            idx = idx[~accepted]
        if not len(idx):
            return
        if level == 0:
            ok = t.leaf_faces[k] >= 0
            if ok.any():
                wq[idx] += face_terms(q[idx], t.tri[k][ok]).sum(axis=1)
                terms[idx, 0] += int(ok.sum())
            return
        for c in range(k * FAN, min(k * FAN + FAN, t.count[level - 1])):
            visit(level - 1, c, idx)

    if t.total:
        visit(len(t.count) - 1, 0, np.nonzero(good)[0])
    wq[~good], terms[~good] = BAD, -1
    return wq, terms


def stand_in_leaf_faces(v, f, keep=None):
    """A leaf-face table without the library: the eligible faces in the order of their centroids' x, y, z, padded with -1.  Any table is a
    valid tree for the reference; the library's own Morton order is what the GPU tests feed it."""
    v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    ids = refs.eligible_faces(v, f, keep)
    c = v[f[ids]].astype(np.float64).mean(axis=1) if len(ids) else np.zeros((0, 3))
    cells = np.floor((c - c.min(axis=0)) / max(float(np.ptp(c)), 1e-30) * 3.999).astype(np.int64) if len(ids) else np.zeros((0, 3), np.int64)
    order = np.lexsort((c[:, 0], cells[:, 0], cells[:, 1], cells[:, 2])) if len(ids) else np.zeros(0, np.int64)
    nleaves = (len(f) + LEAF - 1) // LEAF
    out = np.full(nleaves * LEAF, -1, np.int32)
    out[:len(ids)] = ids[order]
    return out


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------------
def cube_grid(n, drop_bottom=False):
    """The cube [-1, 1]^3 with n x n quads per side: 12 n^2 outward faces, each side with vertices of its own; without the z = -1 side
    (10 n^2 faces) when drop_bottom."""
    t = np.linspace(-1.0, 1.0, n + 1)
    vs, fs, at = [], [], 0
    for axis in range(3):
        for sign in (-1.0, 1.0):
            if drop_bottom and axis == 2 and sign < 0:
                continue
            u, w = (axis + 1) % 3, (axis + 2) % 3
            p = np.zeros((n + 1, n + 1, 3))
            p[..., axis], p[..., u], p[..., w] = sign, t[:, None], t[None, :]
            i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
            p00, p10, p11, p01 = (at + (i + di) * (n + 1) + (j + dj) for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)))
            quads = np.stack([p00, p10, p11, p00, p11, p01], axis=-1).reshape(-1, 3)  # e_u x e_w = e_axis: outward on the + side
            fs.append(quads if sign > 0 else quads[:, ::-1])
            vs.append(p.reshape(-1, 3))
            at += (n + 1) ** 2
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)
