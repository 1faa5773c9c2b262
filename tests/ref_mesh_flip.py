"""Reference of one round of edge flips (include/ts_flip.h) in numpy float64, written from the header's text operation by operation: numpy
rounds every float64 operation and fuses none, which is what the unit's -ffp-contract=off gives.  Vectorised over the edges, so that it
serves the large cases too; nothing here is shared with the package."""
import numpy as np

NO_EDGE, NOT_ELIGIBLE, DELAUNAY, GUARDED, LOST, DUPLICATE, FLIPPED = range(7)  # TSE_*


def takes_part(V, faces, keep=None):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    if keep is not None:
        ok &= np.asarray(keep).reshape(-1) != 0
    return ok


def _sub(p, q):
    return p - q


def _dot(s, t):
    return (s[:, 0] * t[:, 0] + s[:, 1] * t[:, 1]) + s[:, 2] * t[:, 2]


def _cross(s, t):
    return np.stack([s[:, 1] * t[:, 2] - s[:, 2] * t[:, 1], s[:, 2] * t[:, 0] - s[:, 0] * t[:, 2], s[:, 0] * t[:, 1] - s[:, 1] * t[:, 0]], 1)


def wants_flip(p, q, r, s):
    """W(p, q; r, s): (n, 3) float64 rows -> (n,) bool."""
    with np.errstate(all="ignore"):
        u, v = _sub(p, r), _sub(q, r)
        A, w = _dot(u, v), _cross(u, v)
        P = _dot(w, w)
        u2, v2 = _sub(p, s), _sub(q, s)
        B, w2 = _dot(u2, v2), _cross(u2, v2)
        Q = _dot(w2, w2)
        both = (A < 0) & (B < 0)
        first = (A < 0) & (B >= 0)
        second = (B < 0) & (A >= 0)
        return (both & ((P > 0) | (Q > 0))) | (first & ((A * A) * Q > (B * B) * P)) | (second & ((B * B) * P > (A * A) * Q))


def flat_and_unfolded(a, b, c, d, min_cos):
    """Guards (iii) and (iv); min_cos: the fp32 parameter widened."""
    with np.errstate(all="ignore"):
        n0, n1 = _cross(_sub(b, a), _sub(c, a)), _cross(_sub(a, b), _sub(d, b))
        D, L = _dot(n0, n1), _dot(n0, n0) * _dot(n1, n1)
        M = np.float64(min_cos) * np.float64(min_cos)
        flat = ((D >= 0) & (D * D >= M * L)) if min_cos >= 0 else ((D >= 0) | (D * D <= M * L))
        S = n0 + n1
        m0, m1 = _cross(_sub(d, a), _sub(c, a)), _cross(_sub(b, d), _sub(c, d))
        return flat & (_dot(m0, S) > 0) & (_dot(m1, S) > 0)


def priority(lo, hi, seed):
    """The header's mixer in uint32 arithmetic (held in uint64 and masked)."""
    m = np.uint64(0xFFFFFFFF)
    lo, hi = np.asarray(lo, np.uint64), np.asarray(hi, np.uint64)
    h = (np.uint64(seed & 0xFFFFFFFF) * np.uint64(0x9E3779B1) + lo) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h + hi) & m
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def _next(h):
    return np.where(h % 3 == 2, h - 2, h + 1)


def flip_round(vertices, faces, keep=None, min_cos=np.float32(1.0), seed=0):
    """One round.  Returns a dict of the outputs of tse_flip to their capacity (out_faces (F, 3) int32, face_flipped (F,) uint8, edge_vertices
    (3 F, 2) int32, edge_state (3 F,) uint8, edge_opposite (3 F, 2) int32, totals [4]) and E."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    V, F = len(v32), len(f)
    N = 3 * F
    min_cos = float(np.float32(min_cos))
    assert -1.0 <= min_cos <= 1.0
    out = {"out_faces": f.copy(), "face_flipped": np.zeros(F, np.uint8), "edge_vertices": np.full((N, 2), -1, np.int32),
           "edge_state": np.full(N, NO_EDGE, np.uint8), "edge_opposite": np.full((N, 2), -1, np.int32), "totals": [0, 0, 0, 0], "E": 0}
    part = takes_part(V, f, keep)
    if not part.any():
        return out
    flat = f.astype(np.int64).reshape(-1)
    h = (3 * np.nonzero(part)[0][:, None] + np.arange(3)[None, :]).reshape(-1)  # the half-edges of the faces that take part
    tail, head = flat[h], flat[_next(h)]
    lo, hi = np.minimum(tail, head), np.maximum(tail, head)
    order = np.lexsort((h, hi, lo))  # ascending (lo, hi, half-edge)
    h, lo, hi = h[order], lo[order], hi[order]
    is_head = np.ones(len(h), bool)
    is_head[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    start = np.nonzero(is_head)[0]
    E = len(start)
    use = np.diff(np.append(start, len(h)))
    eid = np.cumsum(is_head) - 1
    half_edge_edge = np.full(N, -1, np.int64)
    half_edge_edge[h] = eid
    elo, ehi = lo[start], hi[start]
    out["E"] = E
    out["edge_vertices"][:E, 0], out["edge_vertices"][:E, 1] = elo, ehi
    state = np.full(E, NOT_ELIGIBLE, np.uint8)

    two = np.nonzero(use == 2)[0]
    ha, hb = h[start[two]], h[start[two] + 1]
    opposite_ways = flat[ha] != flat[hb]
    two, ha, hb = two[opposite_ways], ha[opposite_ways], hb[opposite_ways]
    swap = flat[ha] != elo[two]
    h0, h1 = np.where(swap, hb, ha), np.where(swap, ha, hb)  # h0 runs lo -> hi
    c, d = flat[_next(_next(h0))], flat[_next(_next(h1))]
    v = v32.astype(np.float64)
    fin = np.isfinite(v32).all(1)
    ok = (c != d) & fin[elo[two]] & fin[ehi[two]] & fin[c] & fin[d]
    el, h0, h1, c, d = two[ok], h0[ok], h1[ok], c[ok], d[ok]  # the eligible edges
    out["edge_opposite"][el, 0], out["edge_opposite"][el, 1] = c, d
    pa, pb, pc, pd = v[elo[el]], v[ehi[el]], v[c], v[d]
    non = wants_flip(pa, pb, pc, pd)
    state[el] = np.where(non, GUARDED, DELAUNAY)

    # guard (i): the table as a set of lo * V + hi
    table = elo * V + ehi  # ascending
    want = np.minimum(c, d) * V + np.maximum(c, d)
    at = np.searchsorted(table, want)
    exists = (at < E) & (table[np.minimum(at, E - 1)] == want)
    cand = non & ~exists & ~wants_flip(pc, pd, pa, pb) & flat_and_unfolded(pa, pb, pc, pd, min_cos)
    state[el[cand]] = LOST
    out["totals"][:3] = [E, int(non.sum()), int(cand.sum())]

    # selection
    is_cand = np.zeros(E, bool)
    is_cand[el[cand]] = True
    prio = np.zeros(E, np.uint64)
    prio[el[cand]] = priority(elo[el[cand]], ehi[el[cand]], seed)
    ce, ch0, ch1 = el[cand], h0[cand], h1[cand]
    win = np.ones(len(ce), bool)
    for hh in (ch0, ch1):
        for o in (_next(hh), _next(_next(hh))):
            e2 = half_edge_edge[o]
            win &= ~(is_cand[e2] & ((prio[e2] > prio[ce]) | ((prio[e2] == prio[ce]) & (e2 < ce))))
    we, wh0, wh1, wc, wd = ce[win], ch0[win], ch1[win], c[cand][win], d[cand][win]  # ascending edge id
    key = np.minimum(wc, wd) * V + np.maximum(wc, wd)
    _, first = np.unique(key, return_index=True)  # the first occurrence: the smallest edge id
    flips = np.zeros(len(we), bool)
    flips[first] = True
    state[we] = np.where(flips, FLIPPED, DUPLICATE)
    out["totals"][3] = int(flips.sum())
    out["edge_state"][:E] = state

    # the flip: f0 = (a, b, c) -> (a, d, c), f1 = (b, a, d) -> (d, b, c)
    fe, f0, f1 = we[flips], wh0[flips] // 3, wh1[flips] // 3
    a, b, cc, dd = elo[fe], ehi[fe], wc[flips], wd[flips]
    out["out_faces"][f0] = np.stack([a, dd, cc], 1).astype(np.int32)
    out["out_faces"][f1] = np.stack([dd, b, cc], 1).astype(np.int32)
    out["face_flipped"][f0] = 1
    out["face_flipped"][f1] = 1
    return out


def delaunay_flips(vertices, faces, keep=None, min_cos=np.float32(1.0), max_rounds=64):
    """Rounds with seed = round index until one flips nothing.  Returns (faces, per-round totals, converged, the union of face_flipped)."""
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    union = np.zeros(len(f), bool)
    per_round = []
    for r in range(max_rounds):
        o = flip_round(vertices, f, keep, min_cos, r)
        if o["totals"][3] == 0:
            return f, per_round, True, union
        per_round.append(o["totals"])
        union |= o["face_flipped"] != 0
        f = o["out_faces"]
    return f, per_round, False, union


def min_cos_of(max_dihedral_deg):
    """The cosine in float64, rounded to fp32 once."""
    return np.float32(np.cos(np.deg2rad(np.float64(max_dihedral_deg))))


# ---- meshes the tests share -------------------------------------------------------------------------------------------------------------------
def sheared_grid(nx, ny, sx=6, sy=8, jitter=1, seed=1, shear=1):
    """(vertices float32, faces int32) of (ny + 1) rows of (nx + 1) points with integer coordinates in the plane z = 0: spacing sx along a
    row and sy between rows, every row shifted by `shear` more spacings than the row below, the interior points jittered by up to
    `jitter` per axis.  Every cell a b / c d (c above a) is a parallelogram cut by its LONG diagonal a-d: 2 nx ny faces, counter-clockwise.
    The outline is the parallelogram itself, its border points unjittered: convex.  At the default spacing no jitter of 1 inverts
    a face ((sx - 2)(sy - 2) > 2 (sy + 2)); the callers that need a valid triangulation at a tighter spacing check it."""
    rng = np.random.RandomState(seed)
    ii, jj = np.meshgrid(np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    x, y = (jj + shear * ii) * sx, ii * sy
    jit = rng.randint(-jitter, jitter + 1, size=(ny + 1, nx + 1, 2))
    inner = np.zeros((ny + 1, nx + 1), bool)
    inner[1:-1, 1:-1] = True
    x, y = x + jit[..., 0] * inner, y + jit[..., 1] * inner
    x, y = x - (nx + shear * ny) * sx // 2, y - ny * sy // 2
    v = np.stack([x, y, np.zeros_like(x)], -1).reshape(-1, 3).astype(np.float32)
    idx = ii * (nx + 1) + jj
    a, b, c, d = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    f = np.concatenate([np.stack([a, b, d], -1).reshape(-1, 3), np.stack([a, d, c], -1).reshape(-1, 3)]).astype(np.int32)
    return v, f


def stretched_grid(nx, ny, stretch=4.0, seed=1):
    """(vertices, faces): the converged triangulation of a heavily jittered sheared_grid, its vertices then stretched along x.  What was
    Delaunay is poor everywhere now, and non-Delaunay edges share faces: candidates that compete, which the long diagonals of sheared_grid
    never do (one per cell, each in faces of its own)."""
    v, f = sheared_grid(nx, ny, 8, 8, 3, seed)
    g = delaunay_flips(v, f)[0]
    return (v * np.array([stretch, 1.0, 1.0], np.float32)).astype(np.float32), g


# A = (-8, 0), B = (8, 0), C = (0, 2), D = (0, -2): the diagonal A-B is long, the angles at C and D are obtuse
QUAD = np.array([[-8, 0, 0], [8, 0, 0], [0, 2, 0], [0, -2, 0]], np.float32)
LONG = [[0, 1, 2], [1, 0, 3]]  # the quad cut by A-B


def hand_constructions():
    """name -> (vertices, faces, keep, max_dihedral_deg): the constructions of tests/test_mesh_flip_cpu.py, whose results are known by hand,
    for the bit comparison on the device."""
    z = np.float32(0)
    cube_v = np.array([[x, y, z] for z in (0, 2) for y in (0, 2) for x in (0, 2)], np.float32)
    cube_f = [[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]]
    two = np.concatenate([QUAD, np.array([[0, 0, -8], [0, 0, 8]], np.float32)])
    apex = np.concatenate([QUAD, np.array([[0, 0, 4]], np.float32)])
    nan_d = QUAD.copy()
    nan_d[3, 1] = np.nan
    inf_a = QUAD.copy()
    inf_a[0, 2] = -np.inf
    roof = np.array([[-8, 0, 0], [8, 0, 0], [0, 2, 0], [0, 0, -2]], np.float32)
    return {
        "long diagonal": (QUAD, LONG, None, 30.0),
        "short diagonal": (QUAD, [[2, 3, 1], [3, 2, 0]], None, 30.0),
        "long diagonal, slots swapped and rotated": (QUAD, [[0, 3, 1], [2, 0, 1]], None, 30.0),
        "square": (np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]], np.float32), [[0, 1, 2], [0, 2, 3]], None, 30.0),
        "cap": (np.array([[0, 0, 0], [8, 0, 0], [4, 0, 0], [4, -4, 0]], np.float32), LONG, None, 30.0),
        "flattened tetrahedron": (QUAD, [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], None, 180.0),
        "two quads over one vertex pair": (two, [[0, 1, 2], [1, 0, 3], [4, 5, 2], [5, 4, 3]], None, 30.0),
        "two quads, listed the other way": (two, [[4, 5, 2], [5, 4, 3], [0, 1, 2], [1, 0, 3]], None, 30.0),
        "same direction": (apex, [[0, 1, 2], [0, 1, 3]], None, 180.0),
        "use three": (apex, [[0, 1, 2], [1, 0, 3], [0, 1, 4]], None, 180.0),
        "same vertices twice": (QUAD, [[0, 1, 2], [1, 0, 2]], None, 180.0),
        "roof at 30": (roof, LONG, None, 30.0),
        "roof at 89": (roof, LONG, None, 89.0),
        "roof at 90": (roof, LONG, None, 90.0),
        "roof at 180": (roof, LONG, None, 180.0),
        "cube": (cube_v, cube_f, None, 180.0),
        "fold": (np.array([[-8, 0, 0], [8, 0, 0], [0, 2, 0], [12, 4, 0]], np.float32), LONG, None, 180.0),
        "masked": (QUAD, LONG, [1, 0], 30.0),
        "out of range": (QUAD, LONG + [[0, 1, 9], [2, 2, 3], [-1, 0, 1]], None, 30.0),
        "nan": (nan_d, LONG, None, 30.0),
        "inf": (inf_a, LONG, None, 30.0),
        "one face": (QUAD, [[0, 1, 2]], None, 30.0),
    }
