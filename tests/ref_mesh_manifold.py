"""numpy reference of include/ts_manifold.h: participation, corners, edge use, links, the fans -- twice over: by a union-find over the links,
as the header states it, and by a plain walk around every vertex -- the six counts, the split and the promises, written operation by
operation.  There is no floating-point arithmetic: everything is integers.  Fixture builders: books, hubs, cones, the kissing spheres.
"""
import numpy as np

COUNT_NAMES = ("corners", "fans", "fan_vertices", "split_vertices", "nonmanifold_edges", "same_direction_edges")


def _faces(faces):
    return np.asarray(faces, np.int64).reshape(-1, 3)


def participation(V, faces, keep=None):
    """(F,) bool: kept, the three indices in [0, V) and pairwise distinct (ts_smooth.h's rule)."""
    f = _faces(faces)
    kept = np.ones(len(f), bool) if keep is None else np.asarray(keep).reshape(len(f)) != 0
    return kept & ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def edge_runs(V, faces, keep=None):
    """The participating half-edges in (min, max, half-edge) order and their runs: (order, starts, lengths, tail, head)."""
    f = _faces(faces)
    tail, head = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    h = np.nonzero(np.repeat(participation(V, f, keep), 3))[0]
    lo, hi = np.minimum(tail[h], head[h]), np.maximum(tail[h], head[h])
    order = h[np.lexsort((h, hi, lo))]
    key = np.minimum(tail[order], head[order]) * max(V, 1) + np.maximum(tail[order], head[order])
    starts = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0] if len(order) else np.zeros(0, np.int64)
    lengths = np.diff(np.concatenate([starts, [len(order)]]))
    return order, starts, lengths, tail, head


def _next(c):
    return np.where(c % 3 == 2, c - 2, c + 1)


def links(V, faces, keep=None):
    """(pairs (L, 2): the linked corners, nonmanifold_edges, same_direction_edges).  An edge used exactly twice by half-edges h0 < h1 links
    the two corners at either end: h0 with h1 and next(h0) with next(h1) when both leave the same vertex, h0 with next(h1) and next(h0)
    with h1 otherwise."""
    order, starts, lengths, tail, _ = edge_runs(V, faces, keep)
    two = starts[lengths == 2]
    h0, h1 = order[two], order[two + 1]
    same = tail[h0] == tail[h1]
    a = np.stack([h0, np.where(same, h1, _next(h1))], 1)
    b = np.stack([_next(h0), np.where(same, _next(h1), h1)], 1)
    return np.concatenate([a, b]).reshape(-1, 2), int((lengths >= 3).sum()), int(same.sum())


def fans_by_union_find(N, pairs):
    """root (N,): the smallest member of every component; the larger root is hooked under the smaller, paths halved."""
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in pairs.tolist():
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(N)], np.int64).reshape(N)


def fans_by_walking(V, faces, keep=None):
    """root (3 F,), -1 for a corner that does not take part: around every vertex, from every corner not yet seen, across the edges at that
    vertex that exactly two participating faces use, to the other face's corner there; the component's label is its smallest corner."""
    f = _faces(faces)
    part = participation(V, f, keep)
    use, at = {}, {}
    for face in np.nonzero(part)[0].tolist():
        for k in range(3):
            a, b = int(f[face, k]), int(f[face, (k + 1) % 3])
            use.setdefault((min(a, b), max(a, b)), []).append(face)
            at[(face, a)] = 3 * face + k
    root = np.full(3 * len(f), -1, np.int64)
    for face in np.nonzero(part)[0].tolist():
        for k in range(3):
            c = 3 * face + k
            if root[c] >= 0:
                continue
            v = int(f[face, k])
            seen, stack = {c}, [c]
            while stack:
                d = stack.pop()
                g = d // 3
                for w in (int(f[g, (d + 1) % 3]), int(f[g, (d + 2) % 3])):  # the two edges of face g at v
                    faces_here = use[(min(v, w), max(v, w))]
                    if len(faces_here) != 2:
                        continue
                    other = faces_here[0] if faces_here[1] == g else faces_here[1]
                    e = at[(other, v)]
                    if e not in seen:
                        seen.add(e)
                        stack.append(e)
            root[list(seen)] = min(seen)
    return root


def fans(V, faces, keep=None, walk=False):
    """tsf_fans: dict corner_fan (3 F,) int32, vertex_fans (V,) int32, counts (six ints), new_vertices."""
    f = _faces(faces)
    N = 3 * len(f)
    V = max(int(V), 0)
    part = np.repeat(participation(V, f, keep), 3)
    pairs, nonmanifold, same = links(V, f, keep)
    if walk:
        root = fans_by_walking(V, f, keep)
    else:
        root = np.where(part, fans_by_union_find(N, pairs), -1)
    is_root = part & (root == np.arange(N))
    tail = f.reshape(-1)
    per_vertex = np.bincount(tail[is_root], minlength=V).astype(np.int32) if V else np.zeros(0, np.int32)
    counts = [int(part.sum()), int(is_root.sum()), int((per_vertex >= 1).sum()), int((per_vertex >= 2).sum()), nonmanifold, same]
    return {"corner_fan": root.astype(np.int32), "vertex_fans": per_vertex, "counts": counts, "new_vertices": counts[1] - counts[2]}


def split(V, faces, corner_fan, keep=None, capacity=None):
    """tsf_split: dict out_faces (F, 3) int32, new_vertex_source / new_vertex_fan (capacity,) int32, totals [new vertices, corners rewritten].
    An entry of corner_fan counts iff its corner takes part and it lies in [0, 3 F), on a face that takes part, on the corner's vertex."""
    f = _faces(faces)
    N = 3 * len(f)
    V = max(int(V), 0)
    tail = f.reshape(-1)
    part = np.repeat(participation(V, f, keep), 3)
    e = np.asarray(corner_fan, np.int64).reshape(N)
    if V == 0 or N == 0:  # nothing takes part
        capacity = 0 if capacity is None else int(capacity)
        return {"out_faces": f.astype(np.int32), "new_vertex_source": np.full(capacity, -1, np.int32),
                "new_vertex_fan": np.full(capacity, -1, np.int32), "totals": [0, 0]}
    inside = part & (e >= 0) & (e < N)
    at = np.where(inside, e, 0)
    ok = inside & part[at] & (tail[at] == tail) if N else inside
    lab = np.where(ok, e, -1)
    keeper = np.full(V, N, np.int64)
    np.minimum.at(keeper, tail[ok], lab[ok])
    used = np.zeros(N, bool)
    used[lab[ok]] = True
    flag = used & (keeper[np.where(used, tail, 0)] != np.arange(N)) if N else used
    index = np.cumsum(flag) - flag  # exclusive: the new vertices in ascending label
    new = int(flag.sum())
    moved = ok & (keeper[np.where(ok, tail, 0)] != lab) if N else ok
    out = np.where(moved, V + index[np.where(moved, lab, 0)], tail) if N else tail
    capacity = new if capacity is None else int(capacity)
    source, label = np.full(capacity, -1, np.int32), np.full(capacity, -1, np.int32)
    which = np.nonzero(flag)[0][:capacity]
    source[:len(which)], label[:len(which)] = tail[which], which
    return {"out_faces": out.astype(np.int32).reshape(-1, 3), "new_vertex_source": source, "new_vertex_fan": label,
            "totals": [new, int(moved.sum())]}


def split_mesh(vertices, faces, keep=None):
    """(vertices', faces', fans, split): the mesh split_nonmanifold returns, the copies gathered from their sources."""
    v = np.asarray(vertices)
    fn = fans(len(v), faces, keep)
    sp = split(len(v), faces, fn["corner_fan"], keep)
    return np.concatenate([v, v[sp["new_vertex_source"]]]), sp["out_faces"], fn, sp


def uses_of_edges(V, faces, keep=None):
    """{(min, max): sorted faces} over the participating faces."""
    order, starts, lengths, tail, head = edge_runs(V, faces, keep)
    return {(int(min(tail[order[s]], head[order[s]])), int(max(tail[order[s]], head[order[s]]))): sorted((order[s:s + n] // 3).tolist())
            for s, n in zip(starts.tolist(), lengths.tolist())}


def check_promises(V, faces, keep=None):
    """The promises of the header on one input; returns (fans, split, fans of the output)."""
    f = _faces(faces)
    before = fans(V, f, keep)
    sp = split(V, f, before["corner_fan"], keep)
    g, W = sp["out_faces"], V + sp["totals"][0]
    assert sp["totals"][0] == before["new_vertices"]
    part = participation(V, f, keep)
    # a row that does not take part is copied bit for bit; one that names an index in [V, W) would take part in the OUTPUT, so the second
    # pass is told who took part (the header: "the caller passes the participation as keep")
    keep2 = part.astype(np.uint8)
    assert np.array_equal(g[~part], f[~part].astype(np.int32)) and np.array_equal(participation(W, g, keep2), part)
    after = fans(W, g, keep2)
    assert after["counts"][3] == 0 and after["vertex_fans"].max(initial=0) <= 1   # every vertex has at most one fan
    assert after["counts"][4] == 0                                                   # no edge is used three times or more
    assert after["counts"][0] == before["counts"][0] and after["counts"][1] == before["counts"][1]
    old, new = uses_of_edges(V, f, keep), uses_of_edges(W, g, keep2)
    pairs_before = sorted(tuple(u) for u in old.values() if len(u) == 2)
    pairs_after = sorted(tuple(u) for u in new.values() if len(u) == 2)
    assert set(pairs_before) <= set(pairs_after)                                     # the edges used twice, by the same two faces
    again = split(W, g, after["corner_fan"], keep2)
    assert again["totals"] == [0, 0] and np.array_equal(again["out_faces"], g)      # idempotent, bit for bit
    if before["counts"][3] == 0:
        assert np.array_equal(g, f.astype(np.int32)) and sp["totals"] == [0, 0]     # a manifold input comes back bit for bit
    assert (np.diff(sp["new_vertex_fan"]) > 0).all()
    return before, sp, after


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------------
def book(k):
    """k faces on the edge (0, 1): V = k + 2.  The edge's two ends get k fans each."""
    f = np.array([[0, 1, 2 + i] for i in range(k)], np.int64)
    return k + 2, f


def hub(n):
    """n lone triangles that share vertex 0 and nothing else: V = 2 n + 1."""
    f = np.array([[0, 1 + 2 * i, 2 + 2 * i] for i in range(n)], np.int64)
    return 2 * n + 1, f


def cone(n, closed, apex, first):
    """n faces (apex, r_i, r_{i+1}) around `apex`, the rim vertices from `first`: closed uses n rim vertices, open n + 1."""
    rim = first + (np.arange(n + 1) % n if closed else np.arange(n + 1))
    return np.stack([np.full(n, apex), rim[:-1], rim[1:]], 1).astype(np.int64)


def cones(sizes, seed=0):
    """Closed and open cones of the given sizes, each around an apex of its own, and two more that share only their apex; the face order is
    permuted.  Returns (V, faces, apexes: [(apex, fans there)])."""
    rows, apexes, at = [], [], 0
    for n in sizes:
        for closed in (True, False):
            rows.append(cone(n, closed, at, at + 1))
            apexes.append((at, 1))
            at += 1 + (n if closed else n + 1)
    n = sizes[0]
    rows.append(cone(n, True, at, at + 1))
    rows.append(cone(n, False, at, at + 1 + n))
    apexes.append((at, 2))
    at += 1 + n + n + 1
    f = np.concatenate(rows)
    return at, f[np.random.default_rng(seed).permutation(len(f))], apexes


def kissing(vertices, faces, shared=7):
    """Two copies of a closed mesh that share vertex `shared` of the first."""
    v, f = np.asarray(vertices), _faces(faces)
    g = f + len(v)
    g[g == shared + len(v)] = shared
    w = v + np.array([[3.0 * np.abs(v).max(), 0, 0]], v.dtype)
    return np.concatenate([v, w]), np.concatenate([f, g])


def two_tetrahedra():
    """Two tetrahedra that share the edge (0, 1): 6 vertices, 8 faces, the edge used four times."""
    t = lambda a, b, c, d: [[a, b, c], [a, c, d], [a, d, b], [b, d, c]]
    return 6, np.array(t(0, 1, 2, 3) + t(0, 1, 4, 5), np.int64)


SOUP_SIZES = (1, 2, 63, 257, 1025)


def soups(sizes=SOUP_SIZES, seed=3):
    """{V: faces (2 V, 3)}: random soups drawn one after the other, in the order of `sizes`, from ONE default_rng(seed) as
    integers(0, V, (2 V, 3)) -- the sequence the figures of DESIGN.md 16l were taken on."""
    rng = np.random.default_rng(seed)
    return {V: rng.integers(0, V, (2 * V, 3)) for V in sizes}
