"""numpy reference of include/ts_holes.h: boundary half-edges, simple vertices, successors, the boundary loops -- twice over: by pointer
doubling, as the header states it, and by a plain walk along the successors -- and the centroid fans, written operation by operation.
The sums of the fill are Python floats (float64) added one by one in member order; the division and the rounding to fp32 are the correctly
rounded IEEE operations.  The adjacency table is ref_mesh_smooth.adjacency's.
"""
import numpy as np

import ref_mesh_smooth

FILLED, TOO_LONG, LONE_FACE, DEAD = 0, 1, 2, 3
STATUS = {"filled": FILLED, "too_long": TOO_LONG, "lone_face": LONE_FACE, "dead": DEAD}
UNBOUNDED = 2 ** 31 - 1


def _faces(faces):
    return np.asarray(faces, np.int64).reshape(-1, 3)


def table_of(V, faces, keep=None):
    """(offsets, neighbors, edge_faces, num_entries): tss_adjacency's table as vertex_adjacency hands it on."""
    adj = ref_mesh_smooth.adjacency(V, faces, keep)
    return adj["offsets"], adj["neighbors"], adj["edge_faces"], adj["counts"][0]


# ---- boundary half-edges, simple vertices, successors ------------------------------------------------------------------------------------------
def boundary_half_edges(V, faces, keep, table):
    """(boundary (3 F,) bool, tail (3 F,), head (3 F,)): the lower-bound search of the header in the tail's row, cut at num_entries."""
    f = _faces(faces)
    F = len(f)
    tail, head = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    if V <= 0 or F == 0:
        return np.zeros(3 * F, bool), tail, head
    offsets, neighbors, edge_faces, num_entries = table
    offsets = np.asarray(offsets, np.int64)
    nb = np.concatenate([np.asarray(neighbors, np.int64)[:num_entries], [0]])  # the pad is never compared: a search stays below its hi
    ef = np.concatenate([np.asarray(edge_faces, np.int64)[:num_entries], [0]])
    kept = np.ones(F, bool) if keep is None else np.asarray(keep).reshape(F) != 0
    part = kept & ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    part = np.repeat(part, 3)
    t = np.where(part, tail, 0)
    end = np.minimum(offsets[t + 1], num_entries)
    lo, hi = np.maximum(offsets[t], 0), end.copy()
    for _ in range(33):
        active = lo < hi
        m = np.where(active, lo + (hi - lo) // 2, 0)
        below = active & (nb[m] < head)
        lo = np.where(below, m + 1, lo)
        hi = np.where(active & ~below, m, hi)
    assert not (lo < hi).any()
    at = np.where(lo < end, lo, num_entries)
    found = (lo < end) & (nb[at] == head)
    return part & found & (ef[at] == 1), tail, head


def successors(V, faces, keep, table):
    """dict: boundary (3 F,) bool, succ (3 F,) int64 (-1: none; only boundary half-edges have one), nonsimple (the count), tail."""
    boundary, tail, head = boundary_half_edges(V, faces, keep, table)
    N = len(boundary)
    h = np.nonzero(boundary)[0]
    out_count, in_count = np.bincount(tail[h], minlength=max(V, 0)), np.bincount(head[h], minlength=max(V, 0))
    out_min = np.full(max(V, 0), N, np.int64)
    np.minimum.at(out_min, tail[h], h)
    simple = (out_count == 1) & (in_count == 1)
    succ = np.full(N, -1, np.int64)
    succ[h] = np.where(simple[head[h]], out_min[head[h]], -1)
    nonsimple = int((((out_count > 0) | (in_count > 0)) & ~simple).sum())
    return {"boundary": boundary, "succ": succ, "nonsimple": nonsimple, "tail": tail}


# ---- the loops, twice over ---------------------------------------------------------------------------------------------------------------------
def loops_by_doubling(boundary, succ):
    """(lab (3 F,) int64: the head of every half-edge's loop or -1, rank (3 F,) int64: its position in the loop, length (3 F,): at heads).
    Two doubling passes of ceil(log2(max(B, 2))) rounds, every read from the previous round."""
    N = len(boundary)
    B = int(boundary.sum())
    rounds = max(1, int(np.ceil(np.log2(max(B, 2)))))
    assert 2 ** rounds >= B
    idx = np.arange(N)
    jump, label, opened = succ.copy(), idx.copy(), succ < 0  # a half-edge that is not boundary has no successor: open, never on a loop
    for _ in range(rounds):
        go = jump >= 0
        j = np.where(go, jump, 0)
        label = np.where(go, np.minimum(label, label[j]), label)
        opened = np.where(go, opened | opened[j], opened)
        jump = np.where(go, jump[j], jump)
    on_loop = boundary & ~opened
    lab = np.where(on_loop, label, -1)
    # Wyllie: the hops to the member in front of the head, the cycle cut there
    last = ~on_loop | (succ == lab)
    jump, dist = np.where(last, -1, succ), np.where(last, 0, 1)
    for _ in range(rounds):
        go = jump >= 0
        j = np.where(go, jump, 0)
        dist = np.where(go, dist + dist[j], dist)
        jump = np.where(go, jump[j], jump)
    assert not (jump >= 0).any()
    head = np.where(on_loop, lab, 0)
    rank = np.where(on_loop, dist[head] - dist, -1)
    length = np.where(on_loop & (lab == idx), dist + 1, 0)
    return lab, rank, length


def loops_by_walking(boundary, succ):
    """The same three arrays by a plain walk: from every boundary half-edge along the successors until it comes back (a loop) or ends."""
    N = len(boundary)
    lab, rank, length = np.full(N, -1, np.int64), np.full(N, -1, np.int64), np.zeros(N, np.int64)
    seen = np.zeros(N, bool)
    for h in np.nonzero(boundary)[0]:
        if seen[h]:
            continue
        chain, g = [], int(h)
        while g >= 0 and not seen[g]:
            seen[g] = True
            chain.append(g)
            g = int(succ[g])
        if g != h:
            continue  # it ended, or ran into a chain walked before (which then was no cycle either: successors are injective)
        first = chain.index(min(chain))
        chain = chain[first:] + chain[:first]
        lab[chain], rank[chain], length[chain[0]] = chain[0], np.arange(len(chain)), len(chain)
    # a chain that ran into an earlier one: the earlier one ended (a cycle would have contained it), so neither is a loop
    return lab, rank, length


def loops(V, faces, keep=None, table=None, walk=False):
    """dict of tsh_loops' outputs to their capacity: half_edge_loop (3 F,) int32, loop_offsets (F + 1,) int32, loop_half_edges (3 F,) int32,
    counts [boundary, members, loops, nonsimple]; and num_loops, num_members, tail (the tail of every half-edge)."""
    f = _faces(faces)
    F = len(f)
    if table is None:
        table = table_of(V, f, keep) if V > 0 else None
    s = successors(V, f, keep, table)
    lab, rank, length = (loops_by_walking if walk else loops_by_doubling)(s["boundary"], s["succ"])
    heads = np.nonzero(length > 0)[0]  # ascending
    n, lens = len(heads), length[heads]
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(starts[-1])
    index_of = np.full(3 * F, -1, np.int64)
    index_of[heads] = np.arange(n)
    on = lab >= 0
    half_edge_loop = np.where(on, index_of[np.where(on, lab, 0)], -1).astype(np.int32)
    loop_half_edges = np.full(3 * F, -1, np.int32)
    hs = np.nonzero(on)[0]
    loop_half_edges[starts[half_edge_loop[hs]] + rank[hs]] = hs
    loop_offsets = np.full(F + 1, total, np.int32)
    loop_offsets[:n] = starts[:n]
    return {"half_edge_loop": half_edge_loop, "loop_offsets": loop_offsets, "loop_half_edges": loop_half_edges,
            "counts": [int(s["boundary"].sum()), total, n, s["nonsimple"]], "num_loops": n, "num_members": total, "tail": s["tail"]}


def loop_lengths(lp):
    return np.diff(lp["loop_offsets"][:lp["num_loops"] + 1].astype(np.int64))


# ---- the fill ----------------------------------------------------------------------------------------------------------------------------------
def fill(vertices, faces, lp, max_loop_edges=UNBOUNDED, attributes=None, attr_valid=None):
    """dict of tsh_fill's outputs to their capacity: loop_status (loops,) uint8, new_vertices (loops, 3) float32, new_attributes (loops, C)
    float32 and new_attr_valid (loops,) uint8 (None without attributes), new_faces (members, 3) int32, new_face_loop (members,) int32,
    totals [filled, new vertices, new faces]."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    V = len(v)
    f = _faces(faces)
    flat = f.reshape(-1)
    n, members = lp["num_loops"], lp["num_members"]
    off, lhe = lp["loop_offsets"].astype(np.int64), lp["loop_half_edges"].astype(np.int64)
    a = None if attributes is None else np.ascontiguousarray(attributes, np.float32).reshape(V, -1)
    C = 0 if a is None else a.shape[1]
    use = np.ones(V, bool) if attr_valid is None else np.asarray(attr_valid).reshape(V) != 0
    status = np.zeros(n, np.uint8)
    new_vertices = np.zeros((n, 3), np.float32)
    new_attributes = np.zeros((n, C), np.float32) if C else None
    new_attr_valid = np.zeros(n, np.uint8) if C else None
    new_faces = np.full((members, 3), -1, np.int32)
    new_face_loop = np.full(members, -1, np.int32)
    filled = nv = nf = 0
    finite = np.isfinite(v).all(1)
    for i in range(n):
        start = min(max(int(off[i]), 0), members)
        end = min(max(int(off[i + 1]), start), members)
        L = end - start
        if L > max_loop_edges:
            status[i] = TOO_LONG
            continue
        hs = lhe[start:end]
        in_range = bool(((hs >= 0) & (hs < len(flat))).all())
        if L == 3 and in_range and hs[0] // 3 == hs[1] // 3 == hs[2] // 3:
            status[i] = LONE_FACE
            continue
        tails = flat[hs] if in_range else None
        if L < 3 or tails is None or not ((tails >= 0) & (tails < V)).all() or not finite[tails].all():
            status[i] = DEAD
            continue
        status[i] = FILLED
        filled += 1
        if L == 3:
            new_faces[nf], new_face_loop[nf] = (tails[0], tails[2], tails[1]), i
            nf += 1
            continue
        with np.errstate(all="ignore"):
            for axis in range(3):
                s = 0.0
                for t in tails:
                    s = s + float(v[t, axis])
                new_vertices[nv, axis] = np.float32(s / float(L))
            if C:
                who = [t for t in tails if use[t]]
                new_attr_valid[nv] = 1 if who else 0
                for c in range(C):
                    s = 0.0
                    for t in who:
                        s = s + float(a[t, c])
                    new_attributes[nv, c] = np.float32(s / float(len(who))) if who else np.float32(0.0)
        for k in range(L):
            new_faces[nf + k] = (tails[(k + 1) % L], tails[k], V + nv)
        new_face_loop[nf:nf + L] = i
        nf += L
        nv += 1
    return {"loop_status": status, "new_vertices": new_vertices, "new_attributes": new_attributes, "new_attr_valid": new_attr_valid,
            "new_faces": new_faces, "new_face_loop": new_face_loop, "totals": [filled, nv, nf]}


def filled_mesh(vertices, faces, lp, fl):
    """(vertices, faces) of the closed mesh: the input's first, then the new ones."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    _, nv, nf = fl["totals"]
    return np.concatenate([v, fl["new_vertices"][:nv]]), np.concatenate([_faces(faces), fl["new_faces"][:nf].astype(np.int64)])


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------------
def punched_sphere():
    """(vertices, faces): the sphere fixture with 8 vertex fans, 4 one-ring neighbourhoods and 5 single faces removed (17 holes)."""
    import ref_mesh_simplify as fixtures
    v, f = fixtures.sphere_mesh()
    V, F = len(v), len(f)
    rng = np.random.default_rng(11)
    picks = rng.choice(V, 12, replace=False)
    keep = ~np.isin(f, picks[:8]).any(1)                      # the faces incident to the first 8
    ring = np.unique(f[np.isin(f, picks[8:]).any(1)])         # the one-ring of the last 4 (themselves included)
    keep &= ~np.isin(f, ring).any(1)                          # the faces touching it
    keep[rng.choice(F, 5, replace=False)] = False             # 5 faces of the sphere's own numbering
    return v, f[keep]


def capped_sphere():
    """The sphere fixture with every face that has a vertex above mean(z) + 5 removed: one hole."""
    import ref_mesh_simplify as fixtures
    v, f = fixtures.sphere_mesh()
    high = v[:, 2].astype(np.float64) > v[:, 2].astype(np.float64).mean() + 5.0
    return v, f[~high[f].any(1)]


def fused_sphere():
    """fuse_sphere(carve=False), extracted and welded: the level set ends where no view saw the volume."""
    import ref_volume
    s, w, dims, origin, h = ref_volume.fuse_sphere(carve=False)
    tri, _ = ref_volume.extract(ref_volume.field(s, w), dims, origin, h)
    return ref_volume.weld_exact(tri)


def nan_block_sphere():
    """A 24^3 sphere field with two blocks of NaN samples: two holes."""
    import ref_volume
    fld = ref_volume.sphere_field((24, 24, 24), (11.3, 11.6, 11.4), 8.2).reshape(24, 24, 24).copy()
    fld[15:, 9:14, 9:14] = np.nan
    fld[3:8, 3:8, 2:9] = np.nan
    tri, _ = ref_volume.extract(fld.reshape(-1), (24, 24, 24), (0, 0, 0), 1.0)
    return ref_volume.weld_exact(tri)


def open_bands(sizes, seed=0):
    """(vertices, faces): per n of `sizes` two rings of n vertices joined by 2 n faces -- two boundary loops of length n each -- in one mesh,
    the face order permuted with `seed` so that heads and ranks are scattered."""
    verts, faces, base = [], [], 0
    for b, n in enumerate(sizes):
        ang = 2.0 * np.pi * np.arange(n) / n
        for z in (0.0, 1.0):
            verts.append(np.stack([(1.0 + b) * np.cos(ang), (1.0 + b) * np.sin(ang), np.full(n, z + 3.0 * b)], 1))
        i = np.arange(n)
        j = (i + 1) % n
        faces.append(np.stack([base + i, base + j, base + n + i], 1))
        faces.append(np.stack([base + j, base + n + j, base + n + i], 1))
        base += 2 * n
    v, f = np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int64)
    return v, f[np.random.default_rng(seed).permutation(len(f))]
