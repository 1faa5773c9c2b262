"""Reference of one round of half-edge collapses (include/ts_collapse.h) in numpy float64, written from the header's text operation by
operation: numpy rounds every float64 operation and fuses none, which is what the unit's -ffp-contract=off gives.  The front, the vertex
classes, the short test and the selection are vectorised over the edges; only the short eligible edges walk a ring, one Python step each,
so that sparse short edges keep the large cases within seconds.  Nothing here is shared with the package."""
import numpy as np

NO_EDGE, NOT_ELIGIBLE, LONG_ENOUGH, GUARDED, LOST, COLLAPSED = range(6)  # TSP_*
MARK_SHORTER, MARK_VERTEX_LIMIT = 1, 2                                   # TSP_MARK_*
GUARD_LINK, GUARD_LONG, GUARD_NORMAL, GUARD_HELD = 1, 2, 4, 8            # TSP_GUARD_*
MAX_RING = 64                                                            # TSP_MAX_RING
NAMES = ("out_faces", "out_keep", "vertex_target", "edge_vertices", "edge_state", "edge_removed", "edge_guard")


def takes_part(V, faces, keep=None):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    if keep is not None:
        ok &= np.asarray(keep).reshape(-1) != 0
    return ok


def _dot(s, t):
    return (s[:, 0] * t[:, 0] + s[:, 1] * t[:, 1]) + s[:, 2] * t[:, 2]


def _cross(s, t):
    return np.stack([s[:, 1] * t[:, 2] - s[:, 2] * t[:, 1], s[:, 2] * t[:, 0] - s[:, 0] * t[:, 2], s[:, 0] * t[:, 1] - s[:, 1] * t[:, 0]], 1)


def length2(v, i, j):
    """From the smaller index to the larger: d = p_max - p_min, (dx dx + dy dy) + dz dz."""
    d = v[np.maximum(i, j)] - v[np.minimum(i, j)]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


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


def min_cos_of(max_normal_deg):
    """The cosine in float64, rounded to fp32 once, clamped to [0, 1] (cos(90 degrees) rounds to 6e-17)."""
    return np.float32(min(1.0, max(0.0, float(np.float32(np.cos(np.deg2rad(np.float64(max_normal_deg))))))))


def collapse_round(vertices, faces, keep=None, pinned=None, min_edge=None, vertex_limit=None, max_edge=np.inf, min_cos=np.float32(1.0), seed=0):
    """One round: min_edge (TSP_MARK_SHORTER) or vertex_limit (TSP_MARK_VERTEX_LIMIT).  Returns a dict of the outputs of tsp_collapse to their
    capacity (NAMES, totals [4]), E, and for the tests vertex_free (V,) bool."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    V, F = len(v32), len(f)
    N = 3 * F
    assert (min_edge is None) != (vertex_limit is None)
    min_cos = float(np.float32(min_cos))
    assert 0.0 <= min_cos <= 1.0
    M = np.float64(min_cos) * np.float64(min_cos)
    with np.errstate(all="ignore"):
        max2 = np.float64(np.float32(max_edge)) * np.float64(np.float32(max_edge))
    kept = np.ones(F, np.uint8) if keep is None else (np.asarray(keep).reshape(-1) != 0).astype(np.uint8)
    out = {"out_faces": f.copy(), "out_keep": kept.copy(), "vertex_target": np.arange(V, dtype=np.int32),
           "edge_vertices": np.full((N, 2), -1, np.int32), "edge_state": np.full(N, NO_EDGE, np.uint8), "edge_removed": np.full(N, -1, np.int32),
           "edge_guard": np.zeros(N, np.uint8), "totals": [0, 0, 0, 0], "E": 0, "vertex_free": np.zeros(V, bool)}
    part = takes_part(V, f, keep)
    if not part.any():
        return out
    flat = f.astype(np.int64).reshape(-1)
    h = (3 * np.nonzero(part)[0][:, None] + np.arange(3)[None, :]).reshape(-1)  # the half-edges (= corners) of the faces that take part
    # rings: the corners by vertex, stable
    corner_vertex = flat[h]
    ring_order = np.argsort(corner_vertex, kind="stable")
    ring_h = h[ring_order]
    ring_bound = np.searchsorted(corner_vertex[ring_order], np.arange(V + 1))
    ring_count = np.diff(ring_bound)
    # edges
    tail, head = flat[h], flat[_next(h)]
    lo, hi = np.minimum(tail, head), np.maximum(tail, head)
    order = np.lexsort((h, hi, lo))  # ascending (lo, hi, half-edge)
    h, lo, hi = h[order], lo[order], hi[order]
    is_head = np.ones(len(h), bool)
    is_head[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    start = np.nonzero(is_head)[0]
    E = len(start)
    use = np.diff(np.append(start, len(h)))
    elo, ehi = lo[start], hi[start]
    out["E"] = E
    out["edge_vertices"][:E, 0], out["edge_vertices"][:E, 1] = elo, ehi
    state = np.full(E, NOT_ELIGIBLE, np.uint8)
    second = np.minimum(start + 1, len(h) - 1)
    clean = (use == 2) & (flat[h[start]] != flat[h[second]])
    # vertex classes
    v = v32.astype(np.float64)
    fin = np.isfinite(v32).all(1)
    unclean_at = np.bincount(elo[~clean], minlength=V) + np.bincount(ehi[~clean], minlength=V)
    free = (ring_count > 0) & (ring_count <= MAX_RING) & fin & (unclean_at == 0)
    if pinned is not None:
        free &= np.asarray(pinned).reshape(-1) == 0
    out["vertex_free"] = free
    # eligible
    two = np.nonzero(clean & (free[elo] | free[ehi]))[0]
    ha, hb = h[start[two]], h[start[two] + 1]
    swap = flat[ha] != elo[two]
    h0, h1 = np.where(swap, hb, ha), np.where(swap, ha, hb)  # h0 runs lo -> hi
    c, d = flat[_next(_next(h0))], flat[_next(_next(h1))]
    ok = (c != d) & fin[elo[two]] & fin[ehi[two]] & fin[c] & fin[d]
    el, c, d = two[ok], c[ok], d[ok]
    with np.errstate(all="ignore"):
        l2 = length2(v, elo[el], ehi[el])
        if min_edge is not None:
            L = np.float64(np.float32(min_edge))
            short = l2 < L * L
        else:
            limit = np.asarray(vertex_limit, np.float32).reshape(-1)
            la, lb = limit[elo[el]], limit[ehi[el]]
            L = np.where(lb < la, lb, la).astype(np.float64)
            short = ~np.isnan(la) & ~np.isnan(lb) & (l2 < L * L)
    state[el] = LONG_ENOUGH
    table = elo * V + ehi  # ascending

    def guards(r, k, cc, dd):
        """The mask of the guards that fail for r -> k over the whole ring of a FREE r."""
        hs = ring_h[ring_bound[r]:ring_bound[r + 1]]
        x, y = flat[_next(hs)], flat[_next(_next(hs))]
        on = x != k
        x, y = x[on], y[on]
        mask = 0
        with np.errstate(all="ignore"):
            want = np.minimum(x, k) * V + np.maximum(x, k)
            at = np.searchsorted(table, want)
            exists = (at < E) & (table[np.minimum(at, E - 1)] == want)
            if ((x != cc) & (x != dd) & exists).any():
                mask |= GUARD_LINK
            if (~(length2(v, x, np.full_like(x, k)) <= max2)).any():
                mask |= GUARD_LONG
            alive = y != k
            x, y = x[alive], y[alive]
            if (((x == cc) & (y == dd)) | ((x == dd) & (y == cc))).any():
                mask |= GUARD_LINK
            n0, n1 = _cross(v[x] - v[r], v[y] - v[r]), _cross(v[x] - v[k], v[y] - v[k])
            Q0, Q1, D = _dot(n0, n0), _dot(n1, n1), _dot(n0, n1)
            if (~((Q1 > 0) & ((Q0 == 0) | ((D > 0) & (D * D >= (M * Q0) * Q1))))).any():
                mask |= GUARD_NORMAL
        return mask

    removed = np.full(E, -1, np.int64)
    guard = np.zeros(E, np.uint8)
    for i in np.nonzero(short)[0]:
        e, a, b = el[i], int(elo[el[i]]), int(ehi[el[i]])
        mask = 0
        for r, k in ((b, a), (a, b)):  # hi first
            if not free[r]:
                mask |= GUARD_HELD
                continue
            g = guards(r, k, int(c[i]), int(d[i]))
            mask |= g
            if g == 0:
                removed[e] = r
                break
        guard[e] = mask
        state[e] = LOST if removed[e] >= 0 else GUARDED
    cand = np.nonzero(state == LOST)[0]
    out["totals"][:3] = [E, int(short.sum()), len(cand)]
    # selection: rank the candidates by (l2 ascending, priority descending, edge id ascending)
    l2_of = np.zeros(E)
    l2_of[el] = l2
    inverse_priority = np.uint64(0xFFFFFFFF) - priority(elo[cand], ehi[cand], seed)
    ranked = cand[np.lexsort((cand, inverse_priority, l2_of[cand]))]
    rank = np.full(E, E, np.int64)
    rank[ranked] = np.arange(len(ranked))
    best = np.full(V, E, np.int64)
    np.minimum.at(best, elo[cand], rank[cand])
    np.minimum.at(best, ehi[cand], rank[cand])
    best2 = best.copy()  # v itself, then every vertex adjacent to it: the edge table, both ways
    np.minimum.at(best2, elo, best[ehi])
    np.minimum.at(best2, ehi, best[elo])
    win = cand[(best2[elo[cand]] == rank[cand]) & (best2[ehi[cand]] == rank[cand])]
    state[win] = COLLAPSED
    out["totals"][3] = len(win)
    out["edge_state"][:E] = state
    out["edge_removed"][:E] = removed
    out["edge_guard"][:E] = guard
    # the collapse
    r = removed[win]
    target = np.arange(V, dtype=np.int64)
    target[r] = np.where(r == elo[win], ehi[win], elo[win])
    out["vertex_target"] = target.astype(np.int32)
    mapped = target[np.where(part[:, None], f, 0)]
    deleted = part & ((mapped[:, 0] == mapped[:, 1]) | (mapped[:, 1] == mapped[:, 2]) | (mapped[:, 0] == mapped[:, 2]))
    rewrite = part & ~deleted
    out["out_faces"][rewrite] = mapped[rewrite].astype(np.int32)
    out["out_keep"][part] = 1
    out["out_keep"][deleted] = 0
    return out


def collapse_short_edges(vertices, faces, keep=None, max_rounds=64, **rule):
    """Rounds with seed = round index until one collapses nothing, each fed the faces and the keep of the one before.  Returns (faces, keep,
    vertex_target composed over the rounds, per-round totals, converged)."""
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    V = len(np.asarray(vertices).reshape(-1, 3))
    k = None if keep is None else (np.asarray(keep).reshape(-1) != 0).astype(np.uint8)
    target = np.arange(V, dtype=np.int32)
    per_round = []
    for r in range(max_rounds):
        o = collapse_round(vertices, f, k, seed=r, **rule)
        if o["totals"][3] == 0:
            return f, k, target, per_round, True
        per_round.append(o["totals"])
        f, k = o["out_faces"], o["out_keep"]
        target = o["vertex_target"][target]
    return f, k, target, per_round, False


def apply_one(faces, keep, r, k):
    """The collapse r -> k alone, on Python's own terms: every kept face replaces r by k, a face that then names k twice is dropped."""
    f = np.array(faces, np.int32).reshape(-1, 3)
    kept = np.ones(len(f), np.uint8) if keep is None else np.array(keep, np.uint8)
    for i in range(len(f)):
        if kept[i] and r in f[i]:
            if k in f[i]:
                kept[i] = 0
            else:
                f[i] = [k if x == r else x for x in f[i]]
    return f, kept


# ---- meshes the tests share -------------------------------------------------------------------------------------------------------------------
def jittered_grid(nx, ny, jitter=0.3, seed=1, z=0.0):
    """(vertices float32, faces int32): (ny + 1) x (nx + 1) points at unit spacing, every point but the outline's moved by up to `jitter`
    per axis in the plane (and by up to z out of it); 2 nx ny faces, counter-clockwise, every cell cut by the diagonal a-d.  Below a
    jitter of 1/3 no face is inverted."""
    rng = np.random.RandomState(seed)
    ii, jj = np.meshgrid(np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    inner = np.zeros((ny + 1, nx + 1), bool)
    inner[1:-1, 1:-1] = True
    jit = rng.uniform(-1.0, 1.0, size=(ny + 1, nx + 1, 3)) * np.array([jitter, jitter, z]) * inner[..., None]
    v = (np.stack([jj, ii, np.zeros_like(ii)], -1) + jit).reshape(-1, 3).astype(np.float32)
    idx = ii * (nx + 1) + jj
    a, b, c, d = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    f = np.concatenate([np.stack([a, b, d], -1).reshape(-1, 3), np.stack([a, d, c], -1).reshape(-1, 3)]).astype(np.int32)
    return v, f


def pinched_grid(nx, ny, share=0.03, seed=1):
    """jittered_grid(jitter = 0.05) in which a random `share` of the interior points, no two of them in neighbouring cells, sits at a fifth
    of the spacing from its right-hand neighbour: sparse short edges (0.2 against ~1) in a large mesh."""
    v, f = jittered_grid(nx, ny, 0.05, seed)
    rng = np.random.RandomState(seed + 1000)
    grid = v.reshape(ny + 1, nx + 1, 3)
    pick = np.zeros((ny + 1, nx + 1), bool)
    pick[2:-2:3, 2:-3:3] = rng.uniform(size=pick[2:-2:3, 2:-3:3].shape) < share * 9
    rows, cols = np.nonzero(pick)
    grid[rows, cols] = grid[rows, cols + 1] + np.array([-0.2, 0.0, 0.0], np.float32)
    return grid.reshape(-1, 3).copy(), f


def jittered_sphere(rings=12, segments=16, jitter=0.02, seed=1, radius=1.0):
    """A closed lat-long sphere, every vertex moved by up to `jitter` per axis: short edges around the poles, longer ones at the equator."""
    th = np.linspace(0, np.pi, rings + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, segments, endpoint=False)
    pts = [[0.0, 0.0, radius]] + [[radius * np.sin(t) * np.cos(p), radius * np.sin(t) * np.sin(p), radius * np.cos(t)] for t in th for p in ph]
    pts.append([0.0, 0.0, -radius])
    ring = lambda r, s: 1 + r * segments + s % segments
    faces = [(0, ring(0, s), ring(0, s + 1)) for s in range(segments)]
    for r in range(rings - 2):
        for s in range(segments):
            faces += [(ring(r, s), ring(r + 1, s), ring(r + 1, s + 1)), (ring(r, s), ring(r + 1, s + 1), ring(r, s + 1))]
    last = len(pts) - 1
    faces += [(last, ring(rings - 2, s + 1), ring(rings - 2, s)) for s in range(segments)]
    v = np.array(pts) + np.random.RandomState(seed).uniform(-jitter, jitter, (len(pts), 3))
    return v.astype(np.float32), np.array(faces, np.int32)


def fan(n, centre=(0.0, 0.0, 0.0), radius=2.0):
    """A centre (vertex 0) and n rim points (1 .. n) on a circle around it, n faces (0, i, i + 1) counter-clockwise."""
    a = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[list(centre)], np.stack([radius * np.cos(a), radius * np.sin(a), np.zeros(n)], 1)]).astype(np.float32)
    f = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32)
    return v, f


def closed_fan(n, centre=(0.0, 0.0, 0.0), radius=2.0, depth=-1.0):
    """fan(n) closed by a second centre below the plane (vertex n + 1): 2 n faces, every vertex interior."""
    v, f = fan(n, centre, radius)
    v = np.concatenate([v, np.array([[0.0, 0.0, depth]], np.float32)])
    g = np.array([[n + 1, 1 + (i + 1) % n, 1 + i] for i in range(n)], np.int32)
    return v, np.concatenate([f, g])


TETRAHEDRON = (np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2]], np.float32), np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32))
OCTAHEDRON = (np.array([[2, 0, 0], [-2, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 2], [0, 0, -2]], np.float32),
              np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32))


def waisted_tube(n=3, rings=5):
    """An open tube of `rings` rings of n points along z; the middle ring is narrow.  With n = 3 the three edges of a ring bound no face:
    collapsing an edge along the tube next to the waist would pinch the tube there, which the link guard refuses.  The tube is closed by a
    pole at either end, so that every vertex is interior."""
    pts, faces = [], []
    for r in range(rings):
        rad = 0.25 if r == rings // 2 else 1.0
        for s in range(n):
            a = 2 * np.pi * s / n
            pts.append([rad * np.cos(a), rad * np.sin(a), float(r)])
    at = lambda r, s: r * n + s % n
    for r in range(rings - 1):
        for s in range(n):
            faces += [(at(r, s), at(r, s + 1), at(r + 1, s + 1)), (at(r, s), at(r + 1, s + 1), at(r + 1, s))]
    bottom, top = len(pts), len(pts) + 1
    pts += [[0.0, 0.0, -1.0], [0.0, 0.0, float(rings)]]
    faces += [(bottom, at(0, s + 1), at(0, s)) for s in range(n)] + [(top, at(rings - 1, s), at(rings - 1, s + 1)) for s in range(n)]
    return np.array(pts, np.float32), np.array(faces, np.int32)


def cube_with_edge_vertex():
    """A cube of side 2 whose edge from (0, 0, 0) to (2, 0, 0) carries one more vertex at (0.5, 0, 0) (vertex 8): it may slide along the
    crease, onto either end, but not off it."""
    v = np.array([[x, y, z] for z in (0, 2) for y in (0, 2) for x in (0, 2)] + [[0.5, 0, 0]], np.float32)
    f = [[0, 2, 3], [0, 3, 8], [8, 3, 1],          # bottom, z = 0 (seen from below): the edge 0-1 split at 8
         [4, 5, 7], [4, 7, 6],                      # top
         [0, 8, 4], [8, 5, 4], [8, 1, 5],           # front, y = 0
         [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]]
    return v, np.array(f, np.int32)


def square_fan():
    """Centre 0 at (1.5, 0, 0), rim 1 .. 4 at (2, 0), (0, 2), (-2, 0), (0, -2), apex 5 at (0, 0, -2), closed: the edge (0, 1) has length
    0.5, and the collapse 1 -> 0 creates the edges (0, 2), (0, 4), (0, 5) of squared length 6.25 = 2.5^2 exactly."""
    v = np.array([[1.5, 0, 0], [2, 0, 0], [0, 2, 0], [-2, 0, 0], [0, -2, 0], [0, 0, -2]], np.float32)
    f = [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [5, 2, 1], [5, 3, 2], [5, 4, 3], [5, 1, 4]]
    return v, np.array(f, np.int32)


def hand_constructions():
    """name -> (vertices, faces, keyword arguments of collapse_round): the constructions of tests/test_mesh_collapse_cpu.py, whose results
    are known by hand, for the bit comparison on the device."""
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    lean = (1.5, 0.0, 0.0)  # the centre leans towards rim point 1 at (2, 0, 0): the edge (0, 1) has length 0.5
    flat = dict(min_edge=1.0, min_cos=min_cos_of(30.0))
    concave = fan(6, lean)
    concave[0][2] = [1.4, 0.3, 0.0]  # rim point 2 pulled below the line from rim point 1 to rim point 3: the ring is concave there
    zero = closed_fan(6)
    zero[0][0] = zero[0][1]  # the centre sits on rim point 1: an edge of length zero
    nan_v, inf_v = closed_fan(6, lean), closed_fan(6, lean)
    nan_v[0][2, 1], inf_v[0][0, 2] = np.nan, -np.inf  # c of the edge (0, 1); its end
    nan_ring = closed_fan(6, lean)
    nan_ring[0][7, 0] = np.nan  # the apex: in the ring of rim point 1, not among lo, hi, c, d
    limit = np.full(8, 1.0, np.float32)
    limit[1] = np.nan
    below = np.nextafter(np.float32(2.5), np.float32(0.0))
    return {
        "one face": (quad, [[0, 1, 2]], dict(min_edge=5.0)),
        "two-face quad": (quad, [[0, 1, 2], [0, 2, 3]], dict(min_edge=5.0)),
        "tetrahedron": (*TETRAHEDRON, dict(min_edge=5.0, min_cos=0.0)),
        "octahedron": (*OCTAHEDRON, dict(min_edge=3.0, min_cos=0.0)),
        "hexagon fan": (*fan(6, lean), flat),
        "closed hexagon fan": (*closed_fan(6, lean), flat),
        "fan of 65": (*fan(65, (1.9, 0.0, 0.0)), dict(min_edge=0.15, min_cos=0.0)),
        "fan of 64": (*fan(64, (1.9, 0.0, 0.0)), dict(min_edge=0.15, min_cos=0.0)),
        "waisted tube": (*waisted_tube(), dict(min_edge=0.5, min_cos=0.0)),
        "concave ring": (*concave, flat),
        "cube edge": (*cube_with_edge_vertex(), dict(min_edge=10.0, min_cos=min_cos_of(30.0))),
        "zero length": (*zero, dict(min_edge=1e-3, min_cos=min_cos_of(30.0))),
        "max_edge at equality": (*square_fan(), dict(min_edge=1.0, max_edge=2.5, min_cos=0.0)),
        "max_edge just below": (*square_fan(), dict(min_edge=1.0, max_edge=below, min_cos=0.0)),
        "pinned centre": (*closed_fan(6, lean), dict(flat, pinned=[1, 0, 0, 0, 0, 0, 0, 0])),
        "pinned rim": (*closed_fan(6, lean), dict(flat, pinned=[0, 1, 0, 0, 0, 0, 0, 0])),
        "pinned both": (*closed_fan(6, lean), dict(flat, pinned=[1, 1, 0, 0, 0, 0, 0, 0])),
        "vertex limit": (*closed_fan(6, lean), dict(vertex_limit=np.full(8, 1.0, np.float32), min_cos=min_cos_of(30.0))),
        "vertex limit with a NaN": (*closed_fan(6, lean), dict(vertex_limit=limit, min_cos=min_cos_of(30.0))),
        "masked": (*closed_fan(6, lean), dict(flat, keep=[1] * 11 + [0])),
        "out of range": (closed_fan(6, lean)[0], np.concatenate([closed_fan(6, lean)[1], [[0, 1, 9], [2, 2, 3], [-1, 0, 1]]]), flat),
        "nan": (*nan_v, flat),
        "inf": (*inf_v, flat),
        "nan in the ring": (*nan_ring, flat),
    }
