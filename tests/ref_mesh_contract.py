"""Reference of the quadric-error edge contraction (include/ts_contract.h) in numpy float64, written from the header's text operation by
operation: numpy rounds every float64 operation and fuses none, which is what the unit's -ffp-contract=off gives.  What the header takes
from ts_collapse.h and ts_decimate.h -- the front, the classes, eligibility, the LINK guard, the priority, the quadric of a removed vertex,
the ranking, the budget and the selection -- is written here over all edges at once with the helpers of ref_mesh_collapse and
ref_mesh_decimate; the edge quadric, the solve, the clamp, the rounding, the cost and the guards at p*, the merge in the new frame and the
blend are written out below.  Nothing here is shared with the package."""
import numpy as np

import ref_mesh_collapse as rc
import ref_mesh_decimate as rd
from ref_mesh_collapse import GUARD_HELD, GUARD_LINK, GUARD_LONG, GUARD_NORMAL, MAX_RING, min_cos_of, priority, takes_part  # noqa: F401
from ref_mesh_decimate import vertex_quadrics  # noqa: F401  (the initial quadrics are ts_decimate.h's)

NO_EDGE, NOT_ELIGIBLE, TOO_COSTLY, GUARDED, LOST, COLLAPSED, DEFERRED = range(7)  # TSU_*
NAMES = ("out_faces", "out_keep", "vertex_target", "out_vertices", "out_quadrics", "vertex_blend", "edge_vertices", "edge_state", "edge_removed",
         "edge_guard", "edge_cost", "edge_position")
FACE_SIDE = NAMES[:6]
TOTALS = ("edges", "candidates", "in_budget", "collapsed", "too_costly")
_next = rc._next


def quadric_at(q, y):
    """(A y (n, 3), (dot(y, A y) + (dot(b, y) + dot(b, y))) + c (n,)) of the quadric rows q (n, 10) at y (n, 3)."""
    return rd._cost_of_removed(q, y)


def edge_quadric(qr, qk, d):
    """The quadric of the edge in the frame of k: A = A_k + A_r, b = b_k + (A_r d + b_r), c = c_k + cost_r."""
    Ad, cost_r = quadric_at(qr, d)
    out = np.empty_like(qk)
    out[:, :6] = qk[:, :6] + qr[:, :6]
    out[:, 6:9] = qk[:, 6:9] + (Ad + qr[:, 6:9])
    out[:, 9] = qk[:, 9] + cost_r
    return out


def solve(q, m, lam):
    """ts_simplify.h's quadric placement towards m: (y (n, 3), solved (n,) bool); y = m where a test fails."""
    a00, a01, a02, a11, a12, a22 = (q[:, i] for i in range(6))
    with np.errstate(all="ignore"):
        tr = (a00 + a11) + a22
        ok = np.isfinite(tr) & (tr > 0)
        mu = np.float64(lam) * tr
        a00, a11, a22 = a00 + mu, a11 + mu, a22 + mu
        r0, r1, r2 = mu * m[:, 0] - q[:, 6], mu * m[:, 1] - q[:, 7], mu * m[:, 2] - q[:, 8]
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        ok &= np.isfinite(det) & (det > 0)
        y = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                      ((c02 * r0 + c12 * r1) + c22 * r2) / det], 1)
        ok &= np.isfinite(y).all(1)
    return np.where(ok[:, None], y, m), ok


def place(q, d, lam, reach):
    """y of the placement (n, 3): the solve around m = -0.5 d, each axis within h = reach max|d_i| of m; y = m where h is 0."""
    m = -0.5 * d
    y, _ = solve(q, m, lam)
    h = (np.float64(reach) * np.maximum(np.maximum(np.abs(d[:, 0]), np.abs(d[:, 1])), np.abs(d[:, 2])))[:, None]
    with np.errstate(all="ignore"):
        t = y - m
        y = np.where(t > h, m + h, np.where(t < -h, m - h, y))
    return np.where(h > 0, y, m)


def rounded(pk, y):
    """(p* (n, 3) float32, y' (n, 3) float64): the position that is written and the offset everything after it uses."""
    with np.errstate(all="ignore"):
        star = (pk + y).astype(np.float32)
        return star, star.astype(np.float64) - pk


def blend_of(y, d):
    """t = dot(y', -d) / dot(d, d), not > 0 -> +0, above 1 -> 1; dot(d, d) == 0 -> 0."""
    with np.errstate(all="ignore"):
        den = rc._dot(d, d)
        t = rc._dot(y, -d) / den
        t = np.where(t > 0, t, 0.0)
        t = np.where(t > 1, 1.0, t)
    return np.where(den != 0, t, 0.0)


def _walk(front, v, V, table, centre, other, k, cc, dd, new, link, max2, M):
    """The guard bits (n,) of n ring walks: the ring of centre[i], faces (centre, x, y); `other` is the edge's other end, k the survivor the
    LINK test searches beside, new[i] (3,) the position that replaces centre[i]'s.  link: which walks evaluate LINK."""
    flat, ring_h, ring_bound = front["flat"], front["ring_h"], front["ring_bound"]
    n = len(centre)
    bits = np.zeros(n, np.uint8)
    if not n:
        return bits
    E = len(table)
    cnt = np.diff(ring_bound)[centre]
    owner = np.repeat(np.arange(n), cnt)
    offs = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    hs = ring_h[ring_bound[centre][owner] + offs]
    x, y = flat[_next(hs)], flat[_next(_next(hs))]
    R, O, K, C_, D_, P, L = centre[owner], other[owner], k[owner], cc[owner], dd[owner], new[owner], link[owner]
    with np.errstate(all="ignore"):
        on = x != O
        want = np.minimum(x, K) * V + np.maximum(x, K)
        at = np.searchsorted(table, want)
        exists = (at < E) & (table[np.minimum(at, E - 1)] == want)
        is_link = L & on & (x != C_) & (x != D_) & exists
        e = v[x] - P
        too_long = on & ~(((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) <= max2)
        alive = on & (y != O)
        is_link |= L & alive & (((x == C_) & (y == D_)) | ((x == D_) & (y == C_)))
        n0, n1 = rc._cross(v[x] - v[R], v[y] - v[R]), rc._cross(v[x] - P, v[y] - P)
        Q0, Q1, Dn = rc._dot(n0, n0), rc._dot(n1, n1), rc._dot(n0, n1)
        turned = alive & ~((Q1 > 0) & ((Q0 == 0) | ((Dn > 0) & (Dn * Dn >= (M * Q0) * Q1))))
    for flag, bit in ((is_link, GUARD_LINK), (too_long, GUARD_LONG), (turned, GUARD_NORMAL)):
        bits |= np.where(np.bincount(owner, weights=flag, minlength=n) > 0, bit, 0).astype(np.uint8)
    return bits


def contract_round(vertices, faces, quadrics, max_collapses, keep=None, pinned=None, max_cost=np.inf, max_edge=np.inf, min_cos=np.float32(1.0),
                   regularization=1e-3, reach=1.0, seed=0):
    """One round.  Returns a dict of the outputs of tsu_contract to their capacity (NAMES, totals [5]), E, and for the tests vertex_free
    (V,) bool, rank (E,) int64 (the rank of a candidate, deferred ones included, -1 otherwise), placed (E,) bool (an eligible edge with
    two FREE ends) and unrounded (E, 3) float64 (the offset y before the rounding, NaN where the edge is not placed)."""
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
    lam, span = np.float64(np.float32(regularization)), np.float64(np.float32(reach))
    assert np.isfinite(lam) and lam >= 0 and np.isfinite(span) and span >= 0
    with np.errstate(all="ignore"):
        max2 = np.float64(np.float32(max_edge)) * np.float64(np.float32(max_edge))
    kept = np.ones(F, np.uint8) if keep is None else (np.asarray(keep).reshape(-1) != 0).astype(np.uint8)
    out = {"out_faces": f.copy(), "out_keep": kept.copy(), "vertex_target": np.arange(V, dtype=np.int32), "out_vertices": v32.copy(),
           "out_quadrics": Q.copy(), "vertex_blend": np.zeros(V), "edge_vertices": np.full((N, 2), -1, np.int32),
           "edge_state": np.full(N, NO_EDGE, np.uint8), "edge_removed": np.full(N, -1, np.int32), "edge_guard": np.zeros(N, np.uint8),
           "edge_cost": np.full(N, np.inf), "edge_position": np.full((N, 3), np.nan, np.float32), "totals": [0, 0, 0, 0, 0], "E": 0,
           "vertex_free": np.zeros(V, bool), "rank": np.zeros(0, np.int64), "placed": np.zeros(0, bool), "unrounded": np.zeros((0, 3))}
    front = rd._front(v32, f, keep)
    if front is None:
        return out
    part, flat, ring_bound, h, start, use, elo, ehi = (front[k] for k in ("part", "flat", "ring_bound", "h", "start", "use", "elo", "ehi"))
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
    # ends: r = hi unless hi is HELD; the survivor is placed where both are FREE
    both = free[elo[el]] & free[ehi[el]]
    r = np.where(free[ehi[el]], ehi[el], elo[el])
    k = np.where(free[ehi[el]], elo[el], ehi[el])
    pk = v[k]
    dk = pk - v[r]
    # placement, rounding first
    with np.errstate(all="ignore"):
        edge_q = edge_quadric(Q[r], Q[k], dk)
        y = np.where(both[:, None], place(edge_q, dk, lam, span), 0.0)
        star, y1 = rounded(pk, y)
        star = np.where(both[:, None], star, v32[k])  # a survivor that stays: its own row, bit for bit
        new = star.astype(np.float64)
        # cost: the edge quadric at y' where placed; cost_r + c_k where the survivor stays
        _, placed_cost = quadric_at(edge_q, y1)
        _, cost_r = quadric_at(Q[r], dk)
        total = np.where(both, placed_cost, cost_r + Q[k, 9])
        has = np.isfinite(total)
        cost = np.where(total > 0, total, 0.0)  # a negative cost and -0 become +0
    # guards: the ring of r for every eligible edge, the ring of k besides where the survivor moves
    guard = _walk(front, v, V, table, r, k, k, c, d, new, np.ones(n_el, bool), max2, M)
    at = np.nonzero(both)[0]
    side_k = np.zeros(n_el, np.uint8)
    side_k[at] = _walk(front, v, V, table, k[at], r[at], k[at], c[at], d[at], new[at], np.zeros(len(at), bool), max2, M)
    out["sides"] = {"edge": el, "r": r, "k": k, "ring_of_r": guard.copy(), "ring_of_k": side_k}  # per eligible edge, for the tests
    guard |= side_k
    clear = guard == 0
    guard |= np.where(both, 0, GUARD_HELD).astype(np.uint8)
    is_cand = clear & has & (cost <= limit)
    state[el] = np.where(is_cand, LOST, np.where(clear, TOO_COSTLY, GUARDED))
    removed = np.full(E, -1, np.int64)
    removed[el] = np.where(is_cand, r, -1)
    edge_cost = np.full(E, np.inf)
    edge_cost[el] = np.where(clear & has, cost, np.inf)
    mask = np.zeros(E, np.uint8)
    mask[el] = guard
    position = np.full((E, 3), np.nan, np.float32)
    position[el[is_cand]] = star[is_cand]
    placed = np.zeros(E, bool)
    placed[el] = both
    unrounded = np.full((E, 3), np.nan)
    unrounded[el[both]] = y[both]
    out["placed"], out["unrounded"] = placed, unrounded
    # the ranking and the budget (ts_decimate.h's)
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
    out["edge_position"][:E] = position
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
    # what follows a winner: the moved vertex, the quadric in the new frame, the blend
    moved = placed[win]
    with np.errstate(all="ignore"):
        dw = v[wk] - v[wr]
        merged = edge_quadric(Q[wr], Q[wk], dw)
        yw = position[win].astype(np.float64) - v[wk]
        Ay, unclamped = quadric_at(merged, yw)
        merged[moved, 6:9] = (merged[:, 6:9] + Ay)[moved]
        merged[moved, 9] = unclamped[moved]
    out["out_quadrics"][wk] = merged
    out["out_vertices"][wk[moved]] = position[win][moved]
    out["vertex_blend"][wk[moved]] = blend_of(yw, dw)[moved]
    return out


def blend_attributes(attr, out):
    """(1 - t) attr_k + t attr_r in float64 rounded to fp32, for the placed survivors of a round; every other row is copied."""
    a = np.asarray(attr, np.float32)
    res = a.copy()
    t = out["vertex_blend"]
    gone = np.nonzero(out["vertex_target"] != np.arange(len(t)))[0]
    k = out["vertex_target"][gone]
    moved = t[k] > 0
    gone, k = gone[moved], k[moved]
    tk = t[k].reshape((-1,) + (1,) * (a.ndim - 1))
    res[k] = ((1.0 - tk) * a[k].astype(np.float64) + tk * a[gone].astype(np.float64)).astype(np.float32)
    return res


def contract_mesh(vertices, faces, target_faces, keep=None, quadrics="carried", max_rounds=256, **rule):
    """Rounds with seed = round index and max_collapses = ceil((participating faces - target) / 2), until the count is at most the target,
    a round contracts nothing, or max_rounds.  Returns (vertices, faces, keep, vertex_target composed, quadrics, per-round totals, reached)."""
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
        o = contract_round(v32, f, q, -((target_faces - count) // 2), keep=k, seed=r, **rule)
        if o["totals"][3] == 0:
            break
        per_round.append(o["totals"])
        v32, f, k, q = o["out_vertices"], o["out_faces"], o["out_keep"], o["out_quadrics"]
        target = o["vertex_target"][target]
        count -= 2 * o["totals"][3]
    return v32, f, k, target, q, per_round, count <= target_faces


def signed_volume(vertices, faces, keep=None):
    """The signed volume of the kept faces in float64: the sum of det(a, b, c) / 6."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    if keep is not None:
        f = f[np.asarray(keep) != 0]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(rc._dot(a, rc._cross(b, c)).sum() / 6.0)
