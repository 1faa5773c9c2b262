"""Numpy reference of the nearest-neighbour helpers (include/ts_knn.h, csrc/knn.hip, csrc/ts_knn_front.h), bit for bit.

The searches are exact, so WHICH distance wins is mathematics; what is left to the implementation is WHO wins among candidates at
the same distance, and the header answers that: the one that comes first in (Morton code, index) order.  This module restates
    * the front half in float32, operation by operation (numpy never contracts): the bounding box of the points that ignores NaN like
      fminf / fmaxf and always contains the ORIGIN, t = ((v - lo) / (hi - lo)) * 1023 per axis, the conversion that sends NaN and negatives to 0
      and saturates, the bit interleave, and a stable sort of the codes -- `morton_order`;
    * the searches by brute force over all pairs in float64 -- `search`, `nearest_other`, `mean_dist3`.
The inputs of the exact tests (the generators at the bottom) have coordinates that are small integers times a power of two, so every
difference, square and sum of the fp32 kernel is exact whether or not the compiler contracts to FMA, the float64 squared distance IS the
kernel's fp32 value, and equality needs no tolerance.  `search(..., exact=True)` asserts that: every finite squared distance survives the
round trip through float32."""
from __future__ import annotations

import functools

import numpy as np

FLT_MAX = np.finfo(np.float32).max
BOX = 1024  # points per box of the search (csrc/ts_knn_front.h)


# ---- the front half ---------------------------------------------------------------------------------------------------------------------------
def bounding_box(points):
    """(lo, hi), float32 (3,): min / max per axis over the non-NaN values, then with 0 (the reductions are seeded with the origin)."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    zero = np.zeros(3, np.float32)
    with np.errstate(all="ignore"):
        lo = np.fmin(zero, np.fmin.reduce(p, axis=0)) if len(p) else zero
        hi = np.fmax(zero, np.fmax.reduce(p, axis=0)) if len(p) else zero
    return lo.astype(np.float32), hi.astype(np.float32)


def _quantise(v, lo, hi):
    with np.errstate(all="ignore"):
        t = ((v - lo) / (hi - lo)) * np.float32(1023)
        assert t.dtype == np.float32
        t = np.where(t >= 0, np.minimum(t, np.float32(4294967040.0)), np.float32(0))  # NaN / negative -> 0, saturated below 2^32
    return t.astype(np.uint64).astype(np.uint32)  # truncation


def _prep_morton(x):
    x = x.astype(np.uint32)
    x = (x | (x << np.uint32(16))) & np.uint32(0x030000FF)
    x = (x | (x << np.uint32(8))) & np.uint32(0x0300F00F)
    x = (x | (x << np.uint32(4))) & np.uint32(0x030C30C3)
    x = (x | (x << np.uint32(2))) & np.uint32(0x09249249)
    return x


def morton_codes(points):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    lo, hi = bounding_box(p)
    x, y, z = (_prep_morton(_quantise(p[:, a], lo[a], hi[a])) for a in range(3))
    return x | (y << np.uint32(1)) | (z << np.uint32(2))


def morton_order(points):
    """pos (P,) int64: pos[i] = position of point i in the stable sort of the Morton codes, i.e. in (code, index) order."""
    order = np.argsort(morton_codes(points), kind="stable")
    pos = np.empty(len(order), np.int64)
    pos[order] = np.arange(len(order))
    return pos


# ---- the searches -----------------------------------------------------------------------------------------------------------------------------
def search(points, group=1, exact=True, chunk=256):
    """Both searches in one pass over the rows.  Returns a dict:
        nearest (P,) int64   the candidate j (j // group != i // group, distance finite) of minimal distance that comes first in sorted order;
                             i itself where there is no candidate
        d2 (P,) float64      that distance (inf without a candidate)
        ties (P,) int64      how many candidates sit at that distance
        mean3 (P,) float32   ((b0 + b1) + b2) / 3 in float32 over the three smallest distances to the other positions j != i (duplicates count),
                             missing ones counting as FLT_MAX
    exact=True asserts that every finite squared distance is a float32 number (see the module text)."""
    p32 = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    p = p32.astype(np.float64)
    n = len(p)
    pos = morton_order(p32)
    grp = np.arange(n) // int(group)
    nearest = np.arange(n, dtype=np.int64)
    d2min = np.full(n, np.inf)
    ties = np.zeros(n, np.int64)
    mean3 = np.empty(n, np.float32)
    big = np.float64(FLT_MAX)
    for a in range(0, n, chunk):
        rows = np.arange(a, min(n, a + chunk))
        with np.errstate(all="ignore"):
            d = p[rows, None, :] - p[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            finite = np.isfinite(d2)
            if exact:
                assert np.array_equal(d2[finite].astype(np.float32).astype(np.float64), d2[finite]), "a squared distance is not exact in float32"
        usable = finite & (d2 < big)  # what can displace the kernel's initial FLT_MAX
        # nearest point of another group
        cand = usable & (grp[rows, None] != grp[None, :])
        dc = np.where(cand, d2, np.inf)
        m = dc.min(axis=1)
        tie = cand & (dc == m[:, None])
        first = np.where(tie, pos[None, :], n).argmin(axis=1)
        has = cand.any(axis=1)
        nearest[rows] = np.where(has, first, rows)
        d2min[rows] = np.where(has, m, np.inf)
        ties[rows] = tie.sum(axis=1)
        # three nearest other positions
        dk = np.where(usable, d2, big)
        dk[np.arange(len(rows)), rows] = big
        if n >= 3:
            b = np.sort(np.partition(dk, 2, axis=1)[:, :3], axis=1)
        else:
            b = np.concatenate([np.sort(dk, axis=1), np.full((len(rows), 3 - n), big)], axis=1)
        b = b.astype(np.float32)
        with np.errstate(over="ignore"):
            mean3[rows] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3)
    return {"nearest": nearest, "d2": d2min, "ties": ties, "mean3": mean3, "pos": pos}


def nearest_other(points, group, exact=True):
    r = search(points, group, exact)
    return r["nearest"], r["d2"]


def mean_dist3(points, exact=True):
    return search(points, 1, exact)["mean3"]


# ---- the inputs the CPU and GPU tests share: every coordinate a small integer times a power of two -----------------------------------------------
def _shuffled(p, seed):
    return np.ascontiguousarray(np.asarray(p, np.float64)[np.random.default_rng(seed).permutation(len(p))].astype(np.float32))


def lattice(side=14, shift=0.0, scale=1.0, seed=14, crop=3):
    """The side^3 integer lattice, moved by `shift` on every axis, then scaled, rows shuffled, cropped to a multiple of `crop` rows
    (14^3 = 2744 -> 2742: three boxes of 1024)."""
    k = np.arange(side, dtype=np.float64)
    p = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    p = _shuffled((p + shift) * scale, seed)
    return p[:len(p) - len(p) % crop]


def plane(z, side=52, seed=52):
    """side x side integer lattice in the plane of constant z (52^2 = 2704 points): with z = 0 the z extent of the origin-seeded box is zero
    (0 / 0 in the quantisation), with z = 5 it is [0, 5] and every point sits on its upper face."""
    k = np.arange(side, dtype=np.float64)
    xy = np.stack(np.meshgrid(k, k, indexing="ij"), -1).reshape(-1, 2)
    return _shuffled(np.concatenate([xy, np.full((len(xy), 1), float(z))], 1), seed)


def line(n=2700, seed=27):
    """n integer points on the x axis: two zero extents."""
    p = np.zeros((n, 3))
    p[:, 0] = np.arange(n)
    return _shuffled(p, seed)


def copies_and_lattice(copies=1100, others=1000, seed=11):
    """`copies` copies of one lattice point among `others` points of the 14^3 lattice (2100 rows)."""
    lat = lattice(14, 0.0, 1.0, seed=seed + 1)[:others].astype(np.float64)
    return _shuffled(np.concatenate([np.tile(np.array([[3.0, 4.0, 5.0]]), (copies, 1)), lat]), seed)


def doubled_lattice(seed=28):
    """The cropped 14^3 lattice with every point present twice (5484 rows)."""
    lat = lattice(14, 0.0, 1.0).astype(np.float64)
    return _shuffled(np.concatenate([lat, lat]), seed)


def twinned_mesh(side=24, seed=24):
    """The triangles of a triangulated side x side integer vertex grid in z = 0 as a soup of vertex triples (triangle order shuffled), followed by
    their back-face twins T[:, [0, 2, 1]]: with group = 3 an interior vertex has eleven candidates at distance zero (six triangles meet there,
    each twice, less its own)."""
    tris = []
    for y in range(side - 1):
        for x in range(side - 1):
            a, b, c, d = (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1)
            tris += [(a, b, d), (a, d, c)]
    t = np.array(tris, np.float64)  # (T, 3, 2)
    t = t[np.random.default_rng(seed).permutation(len(t))]
    t = np.concatenate([t, np.zeros(t.shape[:2] + (1,))], -1)
    soup = np.concatenate([t, t[:, [0, 2, 1]]], 0)
    return np.ascontiguousarray(soup.reshape(-1, 3).astype(np.float32))


def with_nans(p, share=0.05, seed=5):
    """A copy of p with a NaN in one coordinate of `share` of the rows."""
    rng = np.random.default_rng(seed)
    q = p.copy()
    rows = rng.choice(len(p), int(round(share * len(p))), replace=False)
    q[rows, rng.integers(0, 3, len(rows))] = np.nan
    return q


def with_infs(p, seed=6):
    """A copy of p with +inf as the x of one row and -inf as the y of another."""
    q = p.copy()
    a, b = np.random.default_rng(seed).choice(len(p), 2, replace=False)
    q[a, 0] = np.inf
    q[b, 1] = -np.inf
    return q


EDGE_LATTICE_SIDE = 15  # 15^3 = 3375 rows: the smallest lattice that has the 3072 rows of the largest box-edge case

INPUTS = {
    "lattice": lambda: lattice(14, 0.0),
    "lattice-6.5": lambda: lattice(14, -6.5),
    "lattice+1000": lambda: lattice(14, 1000.0),
    "plane0": lambda: plane(0.0),
    "plane5": lambda: plane(5.0),
    "line": line,
    "copies": copies_and_lattice,
    "doubled": doubled_lattice,
    "twinned": twinned_mesh,
    "nan": lambda: with_nans(lattice(14, -6.5)),
    "inf": lambda: with_infs(lattice(14, -6.5)),
    "edge": lambda: lattice(EDGE_LATTICE_SIDE, 0.0, seed=15, crop=1),
}


@functools.lru_cache(maxsize=None)
def _input(name):
    p = INPUTS[name]()
    p.setflags(write=False)
    return p


def make(name, n=None, shift=None, scale=None):
    """A named input (read-only, cached); `n` keeps the first n rows, `shift` / `scale` build the 14^3 lattice moved and scaled."""
    if shift is not None or scale is not None:
        p = lattice(14, 0.0 if shift is None else shift, 1.0 if scale is None else scale)
    else:
        p = _input(name)
    return p if n is None else p[:n]


_solved = {}


def solve(name, group, n=None, shift=None, scale=None):
    """(points, search(points, group)) of a named input, computed once per process and left unchanged."""
    key = (name, group, n, shift, scale)
    if key not in _solved:
        p = make(name, n, shift, scale)
        r = search(p, group)
        for v in r.values():
            v.setflags(write=False)
        _solved[key] = (p, r)
    return _solved[key]
