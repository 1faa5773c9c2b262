"""Brute-force reference of the triangle-overlap query (include/ts_overlap.h), in numpy float64 over ALL pairs, written from the header's
text: separate multiplies and adds in the header's order, so that the native result can be compared bit for bit.  Also the constructions
with small integer coordinates (every determinant exact, the geometric answer known) and the two generators that the CPU and the GPU
tests share."""
import numpy as np

KIND_CROSSING, KIND_COPLANAR, KIND_DUPLICATE = 1, 2, 3
STATS_KEYS = ("candidates", "adjacent", "crossing", "coplanar", "duplicate", "degenerate", "stored")


def orient(a, b, c, d):
    """(b - a) . ((c - a) x (d - a)) on (..., 3) float64 arrays, every operation rounded."""
    u, v, w = b - a, c - a, d - a
    cx = v[..., 1] * w[..., 2] - v[..., 2] * w[..., 1]
    cy = v[..., 2] * w[..., 0] - v[..., 0] * w[..., 2]
    cz = v[..., 0] * w[..., 1] - v[..., 1] * w[..., 0]
    return (u[..., 0] * cx + u[..., 1] * cy) + u[..., 2] * cz


def seg(p, q, sp, sq, t0, t1, t2):
    out = ~(((sp > 0) & (sq > 0)) | ((sp < 0) & (sq < 0)) | ((sp == 0) & (sq == 0)))
    e0, e1, e2 = orient(p, q, t0, t1), orient(p, q, t1, t2), orient(p, q, t2, t0)
    return out & (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0)))


def eligible(v, f, keep=None):
    """ts_bvh.h's rule: kept, the three indices in [0, V), the nine coordinates finite."""
    v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    if keep is not None:
        ok &= np.asarray(keep).astype(bool)
    fin = np.zeros(len(f), bool)
    if len(v):
        fin[ok] = np.isfinite(v[f[ok]]).all(axis=(1, 2))
    return ok & fin


def _side(vals, skip):
    """0 apart, 1 coplanar, 2 neither: vals (n, 3), skip (n,) the shared vertex or -1."""
    use = skip[:, None] != np.arange(3)[None, :]
    n = use.sum(axis=1)
    pos, neg, zero = ((vals > 0) & use).sum(axis=1), ((vals < 0) & use).sum(axis=1), ((vals == 0) & use).sum(axis=1)
    return np.where((pos == n) | (neg == n), 0, np.where(zero == n, 1, 2))


def pair_kinds(A, B, sa, sb):
    """The kind of n pairs: A, B (n, 3, 3) float64, sa, sb (n,) the shared vertex of each side or -1."""
    n = len(A)
    kinds = np.zeros(n, np.uint8)
    if not n:
        return kinds
    pB = np.stack([orient(A[:, 0], A[:, 1], A[:, 2], B[:, k]) for k in range(3)], axis=1)
    pA = np.stack([orient(B[:, 0], B[:, 1], B[:, 2], A[:, k]) for k in range(3)], axis=1)
    for k in range(3):
        pB[sb == k, k] = 0.0
        pA[sa == k, k] = 0.0
    sideB, sideA = _side(pB, sb), _side(pA, sa)
    apart = (sideB == 0) | (sideA == 0)
    copl = ~apart & ((sideB == 1) | (sideA == 1))
    rest = ~apart & ~copl
    hit = np.zeros(n, bool)
    free = sa < 0
    for k in range(3):  # the edges k -> k + 1 of A against B, of B against A
        k1 = (k + 1) % 3
        hit |= free & seg(A[:, k], A[:, k1], pA[:, k], pA[:, k1], B[:, 0], B[:, 1], B[:, 2])
        hit |= free & seg(B[:, k], B[:, k1], pB[:, k], pB[:, k1], A[:, 0], A[:, 1], A[:, 2])
    idx = np.arange(n)
    ia, ib = np.where(free, 0, sa), np.where(free, 0, sb)
    ap, aq, bp, bq = (ia + 1) % 3, (ia + 2) % 3, (ib + 1) % 3, (ib + 2) % 3  # the edge opposite vertex s is (s + 1, s + 2), in list direction
    hit |= ~free & seg(A[idx, ap], A[idx, aq], pA[idx, ap], pA[idx, aq], B[:, 0], B[:, 1], B[:, 2])
    hit |= ~free & seg(B[idx, bp], B[idx, bq], pB[idx, bp], pB[idx, bq], A[:, 0], A[:, 1], A[:, 2])
    kinds[copl] = KIND_COPLANAR
    kinds[rest & hit] = KIND_CROSSING
    return kinds


def _boxes(v, f, part):
    lo, hi = np.zeros((len(f), 3), np.float32), np.zeros((len(f), 3), np.float32)
    if part.any():
        tri = v[f[part]]
        lo[part], hi[part] = tri.min(axis=1), tri.max(axis=1)
    return lo, hi


def overlap(va, fa, keep_a=None, vb=None, fb=None, keep_b=None):
    """Self mode (vb is None) or cross mode.  Returns a dict: pairs (P, 2) int32 sorted by (first, second), kind (P,) uint8, count_a,
    count_b (None in self mode), stats (a dict of the seven named entries; stored = the total)."""
    self_mode = vb is None
    va, fa = np.asarray(va, np.float32).reshape(-1, 3), np.asarray(fa, np.int64).reshape(-1, 3)
    part_a = eligible(va, fa, keep_a)
    if self_mode:
        part_a &= (fa[:, 0] != fa[:, 1]) & (fa[:, 1] != fa[:, 2]) & (fa[:, 0] != fa[:, 2])
        vb, fb, part_b = va, fa, part_a
    else:
        vb, fb = np.asarray(vb, np.float32).reshape(-1, 3), np.asarray(fb, np.int64).reshape(-1, 3)
        part_b = eligible(vb, fb, keep_b)
    FA, FB = len(fa), len(fb)
    count_a, count_b = np.zeros(FA, np.int32), np.zeros(FB, np.int32)
    stats = dict.fromkeys(STATS_KEYS, 0)
    empty = {"pairs": np.zeros((0, 2), np.int32), "kind": np.zeros(0, np.uint8), "count_a": count_a, "count_b": None if self_mode else count_b,
             "stats": stats}
    if FA == 0 or FB == 0:
        return empty
    stats["degenerate"] = int((~part_a).sum()) + (0 if self_mode else int((~part_b).sum()))
    lo_a, hi_a = _boxes(va, fa, part_a)
    lo_b, hi_b = _boxes(vb, fb, part_b)
    cand = part_a[:, None] & part_b[None, :]
    for ax in range(3):  # fp32, closed
        cand &= (lo_a[:, None, ax] <= hi_b[None, :, ax]) & (lo_b[None, :, ax] <= hi_a[:, None, ax])
    if self_mode:
        cand &= np.arange(FA)[:, None] < np.arange(FB)[None, :]
    I, J = np.nonzero(cand)
    stats["candidates"] = len(I)
    sa, sb = np.full(len(I), -1), np.full(len(I), -1)
    shared = np.zeros(len(I), np.int64)
    if self_mode:
        m = np.full((len(I), 3), -1)
        for k in range(3):
            for l in range(3):
                m[:, k] = np.where(fa[I, k] == fb[J, l], l, m[:, k])
        shared = (m >= 0).sum(axis=1)
        first = np.argmax(m >= 0, axis=1)
        one = shared == 1
        sa[one], sb[one] = first[one], m[np.arange(len(I)), first][one]
    stats["adjacent"] = int((shared == 2).sum())
    kinds = np.zeros(len(I), np.uint8)
    kinds[shared == 3] = KIND_DUPLICATE
    go = shared <= 1
    A, B = va[fa[I[go]]].astype(np.float64), vb[fb[J[go]]].astype(np.float64)
    kinds[go] = pair_kinds(A, B, sa[go], sb[go])
    found = kinds != 0
    I, J, kinds = I[found], J[found], kinds[found]
    cross = kinds == KIND_CROSSING
    np.add.at(count_a, I[cross], 1)
    np.add.at(count_a if self_mode else count_b, J[cross], 1)
    stats.update(crossing=int(cross.sum()), coplanar=int((kinds == KIND_COPLANAR).sum()), duplicate=int((kinds == KIND_DUPLICATE).sum()))
    stats["stored"] = len(I)
    return {"pairs": np.stack([I, J], axis=1).astype(np.int32), "kind": kinds, "count_a": count_a, "count_b": None if self_mode else count_b,
            "stats": stats}  # np.nonzero is row-major: already ascending by (first, second)


def kind_of(va, fa, i, j):
    """The kind of the self-mode pair (i, j), 0 when it is not listed."""
    r = overlap(va, fa)
    hit = np.nonzero((r["pairs"] == [min(i, j), max(i, j)]).all(axis=1))[0]
    return int(r["kind"][hit[0]]) if len(hit) else 0


# ---- constructions: small integers, exact determinants, known answers ---------------------------------------------------------------------
def _mesh(tris):
    """Triangles given by coordinates: vertices with equal coordinates are NOT merged, every corner gets an index of its own."""
    v = np.array(tris, np.float32).reshape(-1, 3)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def constructions():
    """name -> (vertices, faces, expected kind of the pair (0, 1), expected stats entries)."""
    out = {}
    flat = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
    out["piercing"] = (*_mesh([flat, [(1, 1, -1), (1, 1, 1), (3, 3, 1)]]), 1, {"crossing": 1})
    out["parallel"] = (*_mesh([flat, [(0, 0, 1), (4, 0, 1), (0, 4, 1)]]), 0, {"crossing": 0, "coplanar": 0, "candidates": 0})
    out["parallel_close_boxes"] = (*_mesh([[(0, 0, 0), (4, 0, 1), (0, 4, 1)], [(0, 0, 1), (4, 0, 2), (0, 4, 2)]]), 0, {"candidates": 1, "crossing": 0})
    out["vertex_rests_inside"] = (*_mesh([flat, [(1, 1, 0), (1, 1, 2), (2, 1, 2)]]), 1, {"crossing": 1})
    out["edges_cross_in_a_point"] = (*_mesh([[(0, 0, 0), (4, 0, 0), (2, -3, 0)], [(2, 2, -2), (2, -2, 2), (2, 4, 4)]]), 1, {"crossing": 1})
    # one shared vertex (index 0): B's opposite edge pierces A; then the same pair opened up
    v = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0), (1, 1, -1), (1, 1, 1), (1, 1, 3), (2, 2, 3)], np.float32)
    out["shared_vertex_pierced"] = (v, np.array([(0, 1, 2), (0, 3, 4)], np.int32), 1, {"crossing": 1, "adjacent": 0})
    out["shared_vertex_open"] = (v, np.array([(0, 1, 2), (5, 0, 6)], np.int32), 0, {"crossing": 0, "candidates": 1})
    v = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0), (4, 4, 1)], np.float32)
    out["edge_adjacent"] = (v, np.array([(0, 1, 2), (2, 1, 3)], np.int32), 0, {"adjacent": 1, "crossing": 0, "coplanar": 0})
    out["same_indices_other_order"] = (v, np.array([(0, 1, 2), (2, 0, 1)], np.int32), 3, {"duplicate": 1, "adjacent": 0})
    out["overlapping_in_one_plane"] = (*_mesh([flat, [(1, 1, 0), (5, 1, 0), (1, 5, 0)]]), 2, {"coplanar": 1, "crossing": 0})
    out["degenerate_face"] = (v, np.array([(0, 1, 2), (3, 3, 1)], np.int32), 0, {"degenerate": 1, "candidates": 0})
    return out


def tetrahedron():
    v = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4)], np.float32)
    return v, np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.int32)


def cube():
    v = np.array([(x, y, z) for z in (0, 2) for y in (0, 2) for x in (0, 2)], np.float32)
    f = [(0, 2, 1), (1, 2, 3), (4, 5, 6), (5, 7, 6), (0, 1, 4), (1, 5, 4), (2, 6, 3), (3, 6, 7), (0, 4, 2), (2, 4, 6), (1, 3, 5), (3, 7, 5)]
    return v, np.array(f, np.int32)


def octahedron():
    v = np.array([(2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2)], np.float32)
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return v, np.array(f, np.int32)


# ---- generators ------------------------------------------------------------------------------------------------------------------------------
def soup(F, seed, edge=0.15, lo=0.0, hi=1.0):
    """F random triangles of edge about `edge` inside [lo, hi]^3, no shared vertices: many crossings."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(lo + edge, hi - edge, (F, 1, 3))
    v = (centre + rng.uniform(-0.5 * edge, 0.5 * edge, (F, 3, 3))).astype(np.float32).reshape(-1, 3)
    return v, np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def sheets(F, seed):
    """A welded height field with a second, tilted sheet through it, duplicates (the same indices in another order) and degenerate faces
    (a repeated index) sprinkled in; exactly F faces, in a shuffled order."""
    rng = np.random.default_rng(seed)
    n = 2
    while 4 * (n - 1) * (n - 1) < F:
        n += 1
    g = np.arange(n) / 16.0                                            # dyadic: the tilted sheet below is EXACTLY planar in fp32
    x, y = np.meshgrid(g, g, indexing="xy")
    z0 = 0.5 + 0.05 * np.sin(5.0 * x) * np.cos(4.0 * y) + 0.01 * rng.standard_normal(x.shape)
    z1 = 0.25 + 0.5 * x + 0.25 * y                                     # tilted: passes through the first sheet; its faces are coplanar
    v = np.concatenate([np.stack([x, y, z0], -1).reshape(-1, 3), np.stack([x, y, z1], -1).reshape(-1, 3)]).astype(np.float32)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="xy")
    a = (j * n + i).reshape(-1)
    quad = np.concatenate([np.stack([a, a + 1, a + n], 1), np.stack([a + 1, a + n + 1, a + n], 1)])
    f = np.concatenate([quad, quad + n * n])
    f = f[rng.permutation(len(f))][:max(F, 1)]
    extra = max(1, F // 40)
    if F >= 8:
        src = rng.integers(0, F, extra)
        f[rng.choice(F, extra, replace=False)] = f[src][:, [1, 2, 0]]   # duplicates of other faces
        bad = rng.choice(F, extra, replace=False)
        f[bad, 2] = f[bad, 0]                                            # degenerate: (v, w, v)
    return v, f[:F].astype(np.int32)
