"""Reference of the quadric-error decimation (include/ts_decimate.h) in numpy float64, written from the header's text operation by operation:
numpy rounds every float64 operation and fuses none, which is what the unit's -ffp-contract=off gives.  What the header takes from
ts_collapse.h -- taking part, the edge numbering, length2, clean edges, rings, the vertex classes, eligibility, the three guards, the
priority -- is written here once more over all directions at once (every eligible edge walks its rings, so one Python step per edge would
not do), with the helpers of ref_mesh_collapse.  Nothing here is shared with the package."""
import numpy as np

import ref_mesh_collapse as rc
from ref_mesh_collapse import GUARD_HELD, GUARD_LINK, GUARD_LONG, GUARD_NORMAL, MAX_RING, min_cos_of, priority, takes_part  # noqa: F401

NO_EDGE, NOT_ELIGIBLE, TOO_COSTLY, GUARDED, LOST, COLLAPSED, DEFERRED = range(7)  # TSZ_*
NAMES = ("out_faces", "out_keep", "vertex_target", "out_quadrics", "edge_vertices", "edge_state", "edge_removed", "edge_guard", "edge_cost")
TOTALS = ("edges", "candidates", "in_budget", "collapsed", "too_costly")
_next = rc._next


def _front(v32, f, keep):
    """The corners by vertex (stable) and the numbered edges of the faces that take part; None if none does."""
    V = len(v32)
    part = takes_part(V, f, keep)
    if not part.any():
        return None
    flat = f.astype(np.int64).reshape(-1)
    h = (3 * np.nonzero(part)[0][:, None] + np.arange(3)[None, :]).reshape(-1)
    corner_vertex = flat[h]
    ring_order = np.argsort(corner_vertex, kind="stable")
    ring_h = h[ring_order]  # per vertex in ascending corner index
    ring_bound = np.searchsorted(corner_vertex[ring_order], np.arange(V + 1))
    tail, head = flat[h], flat[_next(h)]
    lo, hi = np.minimum(tail, head), np.maximum(tail, head)
    order = np.lexsort((h, hi, lo))
    h, lo, hi = h[order], lo[order], hi[order]
    is_head = np.ones(len(h), bool)
    is_head[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    start = np.nonzero(is_head)[0]
    use = np.diff(np.append(start, len(h)))
    return dict(part=part, flat=flat, ring_h=ring_h, ring_bound=ring_bound, h=h, start=start, use=use, elo=lo[start], ehi=hi[start])


def vertex_quadrics(vertices, faces, keep=None):
    """(V, 10) float64: a00 a01 a02 a11 a12 a22 b0 b1 b2 c.  The i-th ring face of every vertex is added in the i-th step, so each
    accumulator sees its terms in ascending corner index, one rounded product and one rounded sum per term."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    V = len(v32)
    q = np.zeros((V, 10))
    front = _front(v32, f, keep)
    if front is None:
        return q
    v, fin = v32.astype(np.float64), np.isfinite(v32).all(1)
    flat, ring_h, bound = front["flat"], front["ring_h"], front["ring_bound"]
    count = np.diff(bound)
    with np.errstate(all="ignore"):
        for i in range(int(count.max())):
            at = np.nonzero((count > i) & fin)[0]
            hs = ring_h[bound[at] + i]
            x, y = flat[_next(hs)], flat[_next(_next(hs))]
            ok = fin[x] & fin[y]
            at, x, y = at[ok], x[ok], y[ok]
            n = rc._cross(v[x] - v[at], v[y] - v[at])
            for col, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                q[at, col] = q[at, col] + n[:, a] * n[:, b]
    return q


def _cost_of_removed(q, d):
    """(A d (n, 3), cost_r (n,)) of the quadric rows q (n, 10) at the offsets d (n, 3): per row (a_i0 dx + a_i1 dy) + a_i2 dz, then
    (dot(d, A d) + (dot(b, d) + dot(b, d))) + c."""
    rows = ((0, 1, 2), (1, 3, 4), (2, 4, 5))
    Ad = np.stack([(q[:, a] * d[:, 0] + q[:, b] * d[:, 1]) + q[:, c] * d[:, 2] for a, b, c in rows], 1)
    bd = rc._dot(q[:, 6:9], d)
    return Ad, (rc._dot(d, Ad) + (bd + bd)) + q[:, 9]


def decimate_round(vertices, faces, quadrics, max_collapses, keep=None, pinned=None, max_cost=np.inf, max_edge=np.inf, min_cos=np.float32(1.0),
                   seed=0):
    """One round.  Returns a dict of the outputs of tsz_decimate to their capacity (NAMES, totals [5]), E, and for the tests vertex_free
    (V,) bool and rank (E,) int64: the rank of a candidate (deferred ones included), -1 otherwise."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    V, F = len(v32), len(f)
    N = 3 * F
    Q = np.array(quadrics, np.float64).reshape(V, 10)
    max_collapses = int(max_collapses)
    assert max_collapses >= 0
    min_cos = float(np.float32(min_cos))
    assert 0.0 <= min_cos <= 1.0
    M = np.float64(min_cos) * np.float64(min_cos)
    limit = np.float64(np.float32(max_cost))
    assert limit >= 0
    with np.errstate(all="ignore"):
        max2 = np.float64(np.float32(max_edge)) * np.float64(np.float32(max_edge))
    kept = np.ones(F, np.uint8) if keep is None else (np.asarray(keep).reshape(-1) != 0).astype(np.uint8)
    out = {"out_faces": f.copy(), "out_keep": kept.copy(), "vertex_target": np.arange(V, dtype=np.int32), "out_quadrics": Q.copy(),
           "edge_vertices": np.full((N, 2), -1, np.int32), "edge_state": np.full(N, NO_EDGE, np.uint8), "edge_removed": np.full(N, -1, np.int32),
           "edge_guard": np.zeros(N, np.uint8), "edge_cost": np.full(N, np.inf), "totals": [0, 0, 0, 0, 0], "E": 0,
           "vertex_free": np.zeros(V, bool), "rank": np.zeros(0, np.int64)}
    front = _front(v32, f, keep)
    if front is None:
        return out
    part, flat, ring_h, ring_bound, h, start, use, elo, ehi = (front[k] for k in ("part", "flat", "ring_h", "ring_bound", "h", "start", "use", "elo", "ehi"))
    ring_count = np.diff(ring_bound)
    E = len(start)
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
    n_el = len(el)
    table = elo * V + ehi  # ascending
    # the directions: 0 = hi -> lo, 1 = lo -> hi; walked where r is FREE
    r_all = np.stack([ehi[el], elo[el]], 1)
    k_all = np.stack([elo[el], ehi[el]], 1)
    walked = free[r_all]
    guard = np.where(walked, 0, GUARD_HELD).astype(np.uint8)  # (n_el, 2)
    di, dj = np.nonzero(walked)
    r, k, cc, dd = r_all[di, dj], k_all[di, dj], c[di], d[di]
    D = len(r)
    if D:
        cnt = ring_count[r]
        owner = np.repeat(np.arange(D), cnt)
        offs = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        hs = ring_h[ring_bound[r][owner] + offs]
        x, y = flat[_next(hs)], flat[_next(_next(hs))]
        R, K, C_, D_ = r[owner], k[owner], cc[owner], dd[owner]
        with np.errstate(all="ignore"):
            on = x != K  # the face on the edge where k follows r is skipped; the other one has y == k
            want = np.minimum(x, K) * V + np.maximum(x, K)
            at = np.searchsorted(table, want)
            exists = (at < E) & (table[np.minimum(at, E - 1)] == want)
            link = on & (x != C_) & (x != D_) & exists
            too_long = on & ~(rc.length2(v, x, K) <= max2)
            alive = on & (y != K)
            link |= alive & (((x == C_) & (y == D_)) | ((x == D_) & (y == C_)))
            n0, n1 = rc._cross(v[x] - v[R], v[y] - v[R]), rc._cross(v[x] - v[K], v[y] - v[K])
            Q0, Q1, Dn = rc._dot(n0, n0), rc._dot(n1, n1), rc._dot(n0, n1)
            turned = alive & ~((Q1 > 0) & ((Q0 == 0) | ((Dn > 0) & (Dn * Dn >= (M * Q0) * Q1))))
        bits = np.zeros(D, np.uint8)
        for flag, bit in ((link, GUARD_LINK), (too_long, GUARD_LONG), (turned, GUARD_NORMAL)):
            bits |= np.where(np.bincount(owner, weights=flag, minlength=D) > 0, bit, 0).astype(np.uint8)
        guard[di, dj] = bits
    # costs of the directions that passed their guards
    cost = np.full((n_el, 2), np.inf)
    has = np.zeros((n_el, 2), bool)
    passed = walked & (guard == 0)
    pi, pj = np.nonzero(passed)
    with np.errstate(all="ignore"):
        pr, pk = r_all[pi, pj], k_all[pi, pj]
        _, cost_r = _cost_of_removed(Q[pr], v[pk] - v[pr])
        total = cost_r + Q[pk, 9]
        finite = np.isfinite(total)
        total = np.where(total > 0, total, 0.0)  # a negative cost and -0 become +0
    has[pi, pj] = finite
    cost[pi[finite], pj[finite]] = total[finite]
    passes = has & (cost <= limit)
    take_lo = passes[:, 1] & (~passes[:, 0] | (cost[:, 1] < cost[:, 0]))  # a tie goes to r = hi
    is_cand = passes.any(1)
    removed_el = np.where(is_cand, np.where(take_lo, r_all[:, 1], r_all[:, 0]), -1)
    cost_el = np.where(is_cand, np.where(take_lo, cost[:, 1], cost[:, 0]), np.where(passed.any(1), cost.min(1), np.inf))
    state[el] = np.where(is_cand, LOST, np.where(passed.any(1), TOO_COSTLY, GUARDED))
    removed = np.full(E, -1, np.int64)
    removed[el] = removed_el
    edge_cost = np.full(E, np.inf)
    edge_cost[el] = cost_el
    mask = np.zeros(E, np.uint8)
    mask[el] = guard[:, 0] | guard[:, 1]
    out["directions"] = {"edge": el, "guard": guard, "has_cost": has, "cost": cost}  # per eligible edge; column 0 is hi -> lo, 1 is lo -> hi
    # the ranking and the budget
    cand = np.nonzero(state == LOST)[0]
    inverse_priority = np.uint64(0xFFFFFFFF) - priority(elo[cand], ehi[cand], seed)
    ranked = cand[np.lexsort((cand, inverse_priority, edge_cost[cand]))]
    rank = np.full(E, -1, np.int64)
    rank[ranked] = np.arange(len(ranked))
    out["rank"] = rank
    state[ranked[max_collapses:]] = DEFERRED
    live = ranked[:max_collapses]
    out["totals"] = [E, len(cand), len(live), 0, int((state == TOO_COSTLY).sum())]
    # selection over the candidates in budget, by rank
    key = np.where(state == LOST, rank, E)
    best = np.full(V, E, np.int64)
    np.minimum.at(best, elo[live], key[live])
    np.minimum.at(best, ehi[live], key[live])
    best2 = best.copy()
    np.minimum.at(best2, elo, best[ehi])
    np.minimum.at(best2, ehi, best[elo])
    win = live[(best2[elo[live]] == key[live]) & (best2[ehi[live]] == key[live])]
    state[win] = COLLAPSED
    out["totals"][3] = len(win)
    out["edge_state"][:E] = state
    out["edge_removed"][:E] = removed
    out["edge_guard"][:E] = mask
    out["edge_cost"][:E] = edge_cost
    # the collapse
    wr = removed[win]
    wk = np.where(wr == elo[win], ehi[win], elo[win])
    target = np.arange(V, dtype=np.int64)
    target[wr] = wk
    out["vertex_target"] = target.astype(np.int32)
    mapped = target[np.where(part[:, None], f, 0)]
    deleted = part & ((mapped[:, 0] == mapped[:, 1]) | (mapped[:, 1] == mapped[:, 2]) | (mapped[:, 0] == mapped[:, 2]))
    rewrite = part & ~deleted
    out["out_faces"][rewrite] = mapped[rewrite].astype(np.int32)
    out["out_keep"][part] = 1
    out["out_keep"][deleted] = 0
    # the quadrics follow
    with np.errstate(all="ignore"):
        Ad, cost_r = _cost_of_removed(Q[wr], v[wk] - v[wr])
        merged = np.empty((len(win), 10))
        merged[:, :6] = Q[wk, :6] + Q[wr, :6]
        merged[:, 6:9] = Q[wk, 6:9] + (Ad + Q[wr, 6:9])
        merged[:, 9] = Q[wk, 9] + cost_r
    out["out_quadrics"][wk] = merged
    return out


def decimate_mesh(vertices, faces, target_faces, keep=None, quadrics="carried", max_rounds=256, **rule):
    """Rounds with seed = round index and max_collapses = ceil((participating faces - target) / 2), until the count is at most the target,
    a round collapses nothing, or max_rounds.  Returns (faces, keep, vertex_target composed, quadrics, per-round totals, reached)."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    V = len(v32)
    k = None if keep is None else (np.asarray(keep).reshape(-1) != 0).astype(np.uint8)
    count = int(takes_part(V, f, k).sum())
    target = np.arange(V, dtype=np.int32)
    q = vertex_quadrics(v32, f, k) if isinstance(quadrics, str) else np.array(quadrics, np.float64)
    per_round = []
    for r in range(max_rounds):
        if count <= target_faces:
            break
        if quadrics == "memoryless" and r > 0:
            q = vertex_quadrics(v32, f, k)
        o = decimate_round(v32, f, q, -((target_faces - count) // 2), keep=k, seed=r, **rule)
        if o["totals"][3] == 0:
            break
        per_round.append(o["totals"])
        f, k, q = o["out_faces"], o["out_keep"], o["out_quadrics"]
        target = o["vertex_target"][target]
        count -= 2 * o["totals"][3]
    return f, k, target, q, per_round, count <= target_faces


# ---- meshes the tests share -------------------------------------------------------------------------------------------------------------------
def integer_grid(n=6, raised=None, height=3):
    """(n + 1)^2 points at integer positions, 2 n^2 faces (jittered_grid without jitter); `raised` = (row, column) of one vertex lifted by
    `height`."""
    v, f = rc.jittered_grid(n, n, 0.0)
    if raised is not None:
        v[raised[0] * (n + 1) + raised[1], 2] = height
    return v, f


def subdivided_cube(n=8):
    """A cube of side n with integer vertices, every side cut into n x n cells of two faces: 12 n^2 faces (768 at n = 8), closed, outward."""
    index, pts, faces = {}, [], []

    def at(p):
        if p not in index:
            index[p] = len(pts)
            pts.append(p)
        return index[p]

    for axis in range(3):
        for side in (0, n):
            u, w = [a for a in range(3) if a != axis]
            for i in range(n):
                for j in range(n):
                    def corner(di, dj):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        return at(tuple(p))
                    a, b, c, d = corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)
                    quad = [(a, b, c), (a, c, d)]
                    # (u, w, axis) is an even permutation of (0, 1, 2) for axis 2 and 0, odd for axis 1: outward on the far side where even
                    outward = (side == n) == (axis != 1)
                    faces += quad if outward else [(t[0], t[2], t[1]) for t in quad]
    return np.array(pts, np.float32), np.array(faces, np.int32)


def signed_volume6(vertices, faces, keep=None):
    """Six times the signed volume of the kept faces in Python integers (integer coordinates)."""
    v = [[int(x) for x in p] for p in np.asarray(vertices).tolist()]
    total = 0
    for i, (a, b, c) in enumerate(np.asarray(faces).tolist()):
        if keep is not None and not keep[i]:
            continue
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = v[a], v[b], v[c]
        total += ax * (by * cz - bz * cy) - ay * (bx * cz - bz * cx) + az * (bx * cy - by * cx)
    return total
