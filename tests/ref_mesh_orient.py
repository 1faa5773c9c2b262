"""numpy reference of include/ts_orient.h: the links between faces and their parity, the pieces and the consistency flips -- twice over: by a
union-find over the doubled graph, as the header states it, and by a breadth-first walk that carries a parity -- the outward rules, the
quantised signed volume S_p with its sums as Python integers, the ten counts, the written faces and the promises, operation by operation.
Participation and the sorted edge runs are ref_mesh_manifold's.  Fixture builders: strips and Moebius strips, torus and Klein-bottle grids,
the scrambler.
"""
import numpy as np

import ref_mesh_manifold as manifold

COUNT_NAMES = ("faces", "pieces", "nonorientable_pieces", "nonorientable_faces", "linking_edges", "same_direction_before",
               "same_direction_after", "faces_flipped", "pieces_inverted", "nonfinite_terms")
MODES = {"anchor": 0, "majority": 1, "volume": 2}


def _faces(faces):
    return np.asarray(faces, np.int64).reshape(-1, 3)


def face_links(V, faces, keep=None):
    """(f (L,), g (L,), odd (L,) bool): an edge used exactly twice, by half-edges h0 < h1, links faces h0 // 3 and h1 // 3; the link is odd
    when both half-edges leave the same vertex."""
    order, starts, lengths, tail, _ = manifold.edge_runs(V, faces, keep)
    two = starts[lengths == 2]
    h0, h1 = order[two], order[two + 1]
    return h0 // 3, h1 // 3, tail[h0] == tail[h1]


def pieces_by_doubled_union_find(F, f, g, odd):
    """(piece (F,), flip (F,), nonorientable (F,) bool) for ALL faces (a face without a link is a piece of its own): node 2 f is f as given,
    2 f + 1 f reversed; an even link unites (2 f, 2 g) and (2 f + 1, 2 g + 1), an odd one (2 f, 2 g + 1) and (2 f + 1, 2 g)."""
    o = odd.astype(np.int64)
    pairs = np.concatenate([np.stack([2 * f, 2 * g + o], 1), np.stack([2 * f + 1, 2 * g + 1 - o], 1)]).reshape(-1, 2)
    root = manifold.fans_by_union_find(2 * F, pairs)
    r0, r1 = root[0::2], root[1::2]
    non = r0 == r1
    return np.minimum(r0, r1) >> 1, np.where(non, 0, r0 & 1), non


def pieces_by_walking(F, f, g, odd):
    """The same three arrays by a breadth-first walk from every face not yet seen, in ascending order, that carries the parity of the path: a
    face reached with both parities makes its piece non-orientable."""
    near = [[] for _ in range(F)]
    for a, b, o in zip(f.tolist(), g.tolist(), odd.tolist()):
        near[a].append((b, int(o)))
        near[b].append((a, int(o)))
    piece, parity, non = np.full(F, -1, np.int64), np.zeros(F, np.int64), np.zeros(F, bool)
    for start in range(F):
        if piece[start] >= 0:
            continue
        piece[start] = start
        members, queue, twisted = [start], [start], False
        while queue:
            a = queue.pop(0)
            for b, o in near[a]:
                if piece[b] < 0:
                    piece[b], parity[b] = start, parity[a] ^ o
                    members.append(b)
                    queue.append(b)
                elif parity[b] != parity[a] ^ o:
                    twisted = True
        if twisted:
            non[members], parity[members] = True, 0
    return piece, parity, non


def volume_terms(vertices, faces, part, piece, flip):
    """(S {anchor: Python int}, nonfinite faces): the quantised signed volume of every piece (the header's S_p), float64 on widened fp32, every
    operation rounded once, the sums exact."""
    f = _faces(faces)
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    who = np.nonzero(part)[0]
    S = {int(p): 0 for p in np.unique(piece[who])}
    if not len(who):
        return S, 0
    with np.errstate(invalid="ignore", over="ignore"):
        o = v[f[piece[who], 0]]
        a, b, c = v[f[who, 0]] - o, v[f[who, 1]] - o, v[f[who, 2]] - o
        X = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]
        Y = b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]
        Z = b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
        t = (a[:, 0] * X + a[:, 1] * Y) + a[:, 2] * Z
        d = np.abs(np.concatenate([a, b, c], 1))
    finite = np.isfinite(d).all(1)
    good = finite & np.isfinite(t)
    largest = np.where(finite, np.where(finite[:, None], d, 0.0).max(1), 0.0)
    for p in S:
        mine = piece[who] == p
        m = largest[mine].max()
        e = 0 if m == 0 else int(np.frexp(m)[1])
        n = int(mine.sum())
        k = 56 - n.bit_length() - 3 * e
        for i in np.nonzero(mine & good)[0].tolist():
            q = int(np.rint(np.ldexp(t[i], k)))
            assert n * abs(q) < 2 ** 59
            S[p] += -q if flip[who[i]] else q
    return S, int((~good).sum())


def orient(V, faces, keep=None, mode=1, vertices=None, walk=False):
    """tsw_orient: dict face_piece (F,) int32, face_flip (F,) uint8, out_faces (F, 3) int32, counts (ten ints), and S (mode 2: {anchor: S_p})."""
    f = _faces(faces)
    F, V = len(f), max(int(V), 0)
    mode = MODES.get(mode, mode)
    assert mode in (0, 1, 2)
    part = manifold.participation(V, f, keep)
    lf, lg, odd = face_links(V, f, keep)
    piece, flip, non = (pieces_by_walking if walk else pieces_by_doubled_union_find)(F, lf, lg, odd)
    piece, flip, non = np.where(part, piece, -1), np.where(part, flip, 0), non & part
    anchors = np.nonzero(part & (piece == np.arange(F)))[0]
    invert, S, nonfinite = np.zeros(F, bool), None, 0
    if mode == 1:
        n, c = np.bincount(piece[part], minlength=F), np.bincount(piece[part], weights=flip[part], minlength=F).astype(np.int64)
        invert[anchors] = 2 * c[anchors] > n[anchors]
    elif mode == 2:
        S, nonfinite = volume_terms(vertices, f, part, piece, flip)
        invert[anchors] = [S[int(p)] < 0 for p in anchors]
    invert[anchors] &= ~non[anchors]
    final = np.where(part & ~non, flip ^ invert[np.where(part, piece, 0)], 0).astype(np.uint8)
    out = np.where(final[:, None] != 0, f[:, [0, 2, 1]], f).astype(np.int32)
    after = odd ^ (final[lf] != 0) ^ (final[lg] != 0)
    counts = [int(part.sum()), len(anchors), int(non[anchors].sum()), int(non.sum()), len(lf), int(odd.sum()), int(after.sum()),
              int(final.sum()), int(invert.sum()), nonfinite]
    return {"face_piece": piece.astype(np.int32), "face_flip": final, "out_faces": out, "counts": counts, "S": S, "nonorientable": non}


def check_promises(V, faces, keep=None, mode=1, vertices=None):
    """The promises of the header on one input; returns (first call, second call)."""
    f = _faces(faces)
    first = orient(V, f, keep, mode, vertices)
    walked = orient(V, f, keep, mode, vertices, walk=True)
    for key in ("face_piece", "face_flip", "out_faces"):
        assert np.array_equal(first[key], walked[key]), key
    assert first["counts"] == walked["counts"] and first["S"] == walked["S"]
    part = manifold.participation(V, f, keep)
    g = first["out_faces"]
    assert np.array_equal(manifold.participation(V, g, keep), part) and np.array_equal(g[~part], f[~part].astype(np.int32))
    second = orient(V, g, keep, mode, vertices)
    c1, c2 = first["counts"], second["counts"]
    assert c1[6] == c2[5] and c2[6] == c2[5]                                  # what is left is what the second call finds, and leaves
    assert c1[2] > 0 or c1[6] == 0                                          # every conflict that remains lies in a non-orientable piece
    piece, flip = first["face_piece"], first["face_flip"]
    lf, lg, odd = face_links(V, g, keep)
    bad = np.nonzero(odd)[0]
    non = first["nonorientable"]
    assert np.array_equal(non, walked["nonorientable"]) and np.array_equal(non, second["nonorientable"])
    assert non[lf[bad]].all() and non[lg[bad]].all()
    assert c2[7] == 0 and c2[8] == 0 and np.array_equal(second["out_faces"], g)   # a second call flips nothing, bit for bit
    assert np.array_equal(second["face_piece"], piece) and c2[:5] == c1[:5]       # the pieces do not depend on the winding
    assert np.array_equal(g[non], f[non].astype(np.int32)) and not flip[non].any()  # a non-orientable piece comes back bit for bit
    assert (flip[~part] == 0).all() and (piece[~part] == -1).all() and c1[7] == int(flip.sum())
    if mode == 2:
        assert all(s >= 0 for p, s in second["S"].items() if not non[p])      # an orientable piece's volume is |S_p| now
    return first, second


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------------
def strip(n, twist=False):
    """n quads (2 n faces) in a ring, consistently wound: 2 n vertices, vertex 2 i on one rim and 2 i + 1 on the other.  With `twist` the last
    quad joins the rims crosswise: a Moebius strip, one non-orientable piece.  n >= 3.  Returns (vertices (2 n, 3) fp32, faces (2 n, 3))."""
    ang = 2 * np.pi * np.arange(n) / n
    half = ang / 2 if twist else np.zeros(n)
    pts = []
    for a, h in zip(ang, half):
        for s in (-0.3, 0.3):
            r = 1.0 + s * np.cos(h)
            pts.append([r * np.cos(a), r * np.sin(a), s * np.sin(h)])
    rows = []
    for i in range(n):
        a, b = 2 * i, 2 * i + 1
        c, d = (2 * ((i + 1) % n), 2 * ((i + 1) % n) + 1)
        if twist and i == n - 1:
            c, d = d, c
        rows += [[a, c, b], [b, c, d]]
    return np.array(pts, np.float32), np.array(rows, np.int64)


def grid(nu, nv, klein=False):
    """A torus grid of nu x nv quads, consistently wound; with `klein` the seam in u is glued with v reversed: a Klein bottle, closed and
    non-orientable.  nu, nv >= 3.  Returns (vertices (nu nv, 3) fp32, faces (2 nu nv, 3))."""
    at = lambda i, j: (i % nu) * nv + ((-j) % nv if klein and (i // nu) % 2 else j % nv)
    rows = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            rows += [[a, b, c], [a, c, d]]
    u, w = np.meshgrid(2 * np.pi * np.arange(nu) / nu, 2 * np.pi * np.arange(nv) / nv, indexing="ij")
    pts = np.stack([(2 + np.cos(w)) * np.cos(u), (2 + np.cos(w)) * np.sin(u), np.sin(w)], -1).reshape(-1, 3)
    return pts.astype(np.float32), np.array(rows, np.int64)


def scramble(faces, seed, fraction=0.5, permute=True):
    """(faces', mask, order): a seeded mask of about `fraction` of the faces reversed as (a, c, b), then a seeded permutation of the faces:
    faces' = reversed[order]."""
    f = _faces(faces)
    rng = np.random.default_rng(seed)
    mask = rng.random(len(f)) < fraction
    order = rng.permutation(len(f)) if permute else np.arange(len(f))
    return np.where(mask[:, None], f[:, [0, 2, 1]], f)[order], mask[order], order


def latlong_sphere(radius=0.6, rings=14, segments=20, centre=(0.0, 0.0, 0.0)):
    """The lat-long sphere of tests/test_mesh_smooth_gpu.py (the same vertices and faces at its defaults), outward; float64 arithmetic,
    rounded to fp32 once."""
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
    return (np.array(pts, np.float64) + np.array(centre, np.float64)).astype(np.float32), np.array(faces, np.int64)


def signed_volume(vertices, faces):
    v, f = np.asarray(vertices, np.float64), _faces(faces)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6)


def mixed_mesh(seed=5):
    """One mesh of several pieces: a scrambled sphere; a 2 mm sphere 50 units away with its faces inward; a torus; a Klein bottle; a Moebius
    strip; a book of 257 faces (257 one-face pieces: its spine links nothing); a hub of 257; lone triangles; rows with the indices -1 and
    V and with repeated indices.  The faces are permuted.  Returns (vertices, faces, keep, parts {name: (first vertex, rows in the result)})."""
    rng = np.random.default_rng(seed)
    blocks, rows, names = [], [], []

    def add(name, v, f):
        first = sum(len(b) for b in blocks)
        blocks.append(np.asarray(v, np.float32))
        rows.append(_faces(f) + first)
        names.append((name, first, len(f)))

    v, f = latlong_sphere()
    add("sphere", v, scramble(f, seed + 1, permute=False)[0])
    v, f = latlong_sphere(radius=0.002, rings=6, segments=8, centre=(50.0, 0.0, 0.0))
    add("small", v, f[:, [0, 2, 1]])
    v, f = grid(9, 7)
    add("torus", v + np.float32(5), scramble(f, seed + 2, 0.3, permute=False)[0])
    v, f = grid(8, 6, klein=True)
    add("klein", v - np.float32(7), scramble(f, seed + 3, permute=False)[0])
    v, f = strip(37, twist=True)
    add("moebius", v * np.float32(2), scramble(f, seed + 4, permute=False)[0])
    V, f = manifold.book(257)
    add("book", rng.uniform(-1, 1, (V, 3)), f)
    V, f = manifold.hub(257)
    add("hub", rng.uniform(-1, 1, (V, 3)), scramble(f, seed + 5, permute=False)[0])
    add("lone", rng.uniform(-1, 1, (30, 3)), np.arange(30).reshape(10, 3))
    vertices, faces = np.concatenate(blocks), np.concatenate(rows)
    V = len(vertices)
    faces = np.concatenate([faces, [[-1, 0, 1], [0, V, 2], [3, 3, 0], [V, V, -1], [5, 6, 5]]])
    source = np.concatenate([np.full(n, i) for i, (_, _, n) in enumerate(names)] + [np.full(5, len(names))])
    order = rng.permutation(len(faces))
    faces, source = faces[order], source[order]
    keep = (rng.integers(0, 6, len(faces)) != 0).astype(np.uint8)
    parts = {name: (first, np.nonzero(source == i)[0]) for i, (name, first, _) in enumerate(names)}
    return vertices, faces, keep, parts
