"""numpy float64 reference of include/ts_subdivide.h, written from the header's text operation by operation: the edge table of an indexed mesh
and the conforming 1-to-2/3/4 split at the midpoints of marked edges.  Every array has the device's dtype and capacity, fill values included,
so that tests compare bit for bit.  Also the small constructions the CPU and GPU tests share."""
import numpy as np

MARK_ALL, MARK_LONGER, MARK_VERTEX_LIMIT = 0, 1, 2
COUNT_NAMES = ("edges", "boundary", "manifold", "nonmanifold")
TOTAL_NAMES = ("edges", "marked", "out_faces", "faces_split")
QNAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


def participation(V, faces, keep=None):
    """(F,) bool: kept, the three indices in [0, V) and pairwise distinct."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    if keep is not None:
        ok &= np.asarray(keep).reshape(-1) != 0
    return ok


def squared_length(p, q):
    """(dx dx + dy dy) + dz dz with d = q - p, float64 rows (..., 3)."""
    with np.errstate(all="ignore"):
        d = np.asarray(q, np.float64) - np.asarray(p, np.float64)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def edges(V, faces, keep=None, vertices=None):
    """tsd_edges: edge_vertices (3 F, 2) int32, edge_use (3 F,) int32, edge_length2 (3 F,) float64 or None, half_edge_edge (3 F,) int32,
    counts (a list of four), and `finite` (E,) bool where vertices are given."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    N = 3 * F
    ok = participation(V, f, keep)
    tail, head = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    part = np.repeat(ok, 3)
    lo, hi = np.minimum(tail, head)[part], np.maximum(tail, head)[part]
    which = np.nonzero(part)[0]
    ev = np.full((N, 2), -1, np.int32)
    use = np.zeros(N, np.int32)
    hee = np.full(N, -1, np.int32)
    E = 0
    if len(which):
        pairs, inverse, count = np.unique(np.stack([lo, hi], 1), axis=0, return_inverse=True, return_counts=True)  # ascending (lo, hi)
        E = len(pairs)
        ev[:E], use[:E], hee[which] = pairs, count, inverse.reshape(-1)
    out = {"E": E, "edge_vertices": ev, "edge_use": use, "half_edge_edge": hee, "edge_length2": None,
           "counts": [E, int((use[:E] == 1).sum()), int((use[:E] == 2).sum()), int((use[:E] >= 3).sum())]}
    if vertices is not None:
        p = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
        l2 = np.zeros(N, np.float64)
        a, b = p[ev[:E, 0]], p[ev[:E, 1]]
        fin = np.isfinite(a).all(1) & np.isfinite(b).all(1)
        l2[:E] = np.where(fin, squared_length(a, b), QNAN)
        out["edge_length2"], out["finite"] = l2, fin
    return out


def marks(table, mode, max_edge=0.0, vertex_limit=None):
    """(E,) bool from edges()' table with vertices."""
    E = table["E"]
    l2, fin, ev = table["edge_length2"][:E], table["finite"], table["edge_vertices"][:E]
    if mode == MARK_ALL:
        return fin.copy()
    with np.errstate(all="ignore"):
        if mode == MARK_LONGER:
            m = np.float64(np.float32(max_edge))
            return fin & (l2 > m * m)
        lim = np.asarray(vertex_limit, np.float32)
        la, lb = lim[ev[:, 0]], lim[ev[:, 1]]
        L = np.where(lb < la, lb, la).astype(np.float64)
        return fin & ~np.isnan(la) & ~np.isnan(lb) & (l2 > L * L)


def split(vertices, faces, keep=None, mode=MARK_ALL, max_edge=0.0, vertex_limit=None, attributes=None, attr_valid=None):
    """tsd_split, every output to its capacity: new_vertices (3 F, 3), new_attributes (3 F, C) / new_attr_valid (3 F,) uint8 (None without
    channels), new_vertex_edge (3 F, 2), out_faces (4 F, 3), out_face_parent (4 F,), totals (a list of four)."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    V = len(v32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    N = 3 * F
    table = edges(V, f, keep, v32)
    E = table["E"]
    marked = marks(table, mode, max_edge, vertex_limit)
    which = np.nonzero(marked)[0]  # ascending edge id: rank r
    n = len(which)
    ends = table["edge_vertices"][which].astype(np.int64)
    p = v32.astype(np.float64)
    new_vertices = np.zeros((N, 3), np.float32)
    new_vertices[:n] = ((p[ends[:, 0]] + p[ends[:, 1]]) * 0.5).astype(np.float32)
    new_vertex_edge = np.full((N, 2), -1, np.int32)
    new_vertex_edge[:n] = ends
    channels = 0 if attributes is None else np.asarray(attributes).shape[1]
    new_attributes = new_attr_valid = None
    if channels:
        a32 = np.asarray(attributes, np.float32)
        a = a32.astype(np.float64)
        ok = np.ones(V, bool) if attr_valid is None else np.asarray(attr_valid).reshape(-1) != 0
        vl, vh = ok[ends[:, 0]], ok[ends[:, 1]]
        with np.errstate(all="ignore"):
            mean = ((a[ends[:, 0]] + a[ends[:, 1]]) * 0.5).astype(np.float32)
        rows = np.where((vl & vh)[:, None], mean, np.where(vl[:, None], a32[ends[:, 0]], np.where(vh[:, None], a32[ends[:, 1]], np.float32(0))))
        new_attributes = np.zeros((N, channels), np.float32)
        new_attributes[:n] = rows
        new_attr_valid = np.zeros(N, np.uint8)
        new_attr_valid[:n] = vl | vh
    edge_mid = np.full(E, -1, np.int64)
    edge_mid[which] = V + np.arange(n)
    hee = table["half_edge_edge"]
    half_edge_mid = np.where(hee >= 0, edge_mid[np.maximum(hee, 0)] if E else -1, -1).reshape(F, 3)
    position = np.concatenate([v32, new_vertices[:n]]).astype(np.float64)  # the fp32 positions as written
    out_faces = np.full((4 * F, 3), -1, np.int32)
    parent = np.full(4 * F, -1, np.int32)
    at = faces_split = 0
    for i in range(F):
        v, m = f[i], half_edge_mid[i]
        k_marked = [k for k in range(3) if m[k] >= 0]
        if len(k_marked) == 0:
            pieces = [tuple(v)]
        elif len(k_marked) == 1:
            k = k_marked[0]
            a, b, c = v[k], v[(k + 1) % 3], v[(k + 2) % 3]
            pieces = [(a, m[k], c), (m[k], b, c)]
        elif len(k_marked) == 2:
            k = next(k for k in range(3) if m[k] < 0)
            a, b, c, m1, m2 = v[k], v[(k + 1) % 3], v[(k + 2) % 3], m[(k + 1) % 3], m[(k + 2) % 3]
            d1, d2 = squared_length(position[a], position[m1]), squared_length(position[b], position[m2])
            if d1 < d2 or (d1 == d2 and a < b):
                pieces = [(m1, c, m2), (a, b, m1), (a, m1, m2)]
            else:
                pieces = [(m1, c, m2), (a, b, m2), (b, m1, m2)]
        else:
            pieces = [(v[0], m[0], m[2]), (m[0], v[1], m[1]), (m[2], m[1], v[2]), (m[0], m[1], m[2])]
        faces_split += len(pieces) > 1
        for piece in pieces:
            out_faces[at], parent[at] = piece, i
            at += 1
    return {"new_vertices": new_vertices, "new_attributes": new_attributes, "new_attr_valid": new_attr_valid, "new_vertex_edge": new_vertex_edge,
            "out_faces": out_faces, "out_face_parent": parent, "totals": [E, n, at, int(faces_split)], "marked": marked, "table": table}


def split_mesh(vertices, faces, keep=None, mode=MARK_ALL, max_edge=0.0, vertex_limit=None, attributes=None, attr_valid=None):
    """One round joined to its input, as split_edges returns it: (vertices, faces, attributes, valid (bool), vertex_edge of the new rows,
    face_parent, totals)."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    s = split(v32, faces, keep, mode, max_edge, vertex_limit, attributes, attr_valid)
    n, nf = s["totals"][1], s["totals"][2]
    out_a = out_valid = None
    if attributes is not None:
        a32 = np.asarray(attributes, np.float32)
        was = np.ones(len(v32), bool) if attr_valid is None else np.asarray(attr_valid).reshape(-1) != 0
        ends = s["new_vertex_edge"][:n]
        if a32.shape[1]:
            out_a, out_valid = np.concatenate([a32, s["new_attributes"][:n]]), np.concatenate([was, s["new_attr_valid"][:n] != 0])
        else:
            out_a, out_valid = np.zeros((len(v32) + n, 0), np.float32), np.concatenate([was, was[ends[:, 0]] | was[ends[:, 1]]])
    return np.concatenate([v32, s["new_vertices"][:n]]), s["out_faces"][:nf], out_a, out_valid, s["new_vertex_edge"][:n], s["out_face_parent"][:nf], s["totals"]


def split_rounds(vertices, faces, calls, max_edge=None, vertex_limit=None, attributes=None, attr_valid=None, keep=None):
    """split_long_edges / subdivide_mesh: at most `calls` rounds of split_mesh, until one marks nothing.  A new vertex's limit is
    (float)((l_lo + l_hi) 0.5); pieces inherit keep; face_parent is composed back to the input's faces.  Returns a dict."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    V0 = len(v)
    mode = MARK_LONGER if max_edge is not None else MARK_VERTEX_LIMIT if vertex_limit is not None else MARK_ALL
    limit = None if vertex_limit is None else np.asarray(vertex_limit, np.float32)
    a = None if attributes is None else np.asarray(attributes, np.float32)
    valid = None if attr_valid is None else np.asarray(attr_valid).reshape(-1) != 0
    k = None if keep is None else np.asarray(keep).reshape(-1) != 0
    parent = np.arange(len(f), dtype=np.int32)
    edge_rows, per_round, converged = [], [], False
    for _ in range(calls):
        v2, f2, a2, valid2, e, p, totals = split_mesh(v, f, k, mode, 0.0 if max_edge is None else max_edge, limit, a, valid)
        if totals[1] == 0:
            converged = True
            break
        per_round.append(totals)
        edge_rows.append(e)
        if limit is not None:
            limit = np.concatenate([limit, ((limit[e[:, 0]].astype(np.float64) + limit[e[:, 1]].astype(np.float64)) * 0.5).astype(np.float32)])
        parent = parent[p]
        if k is not None:
            k = k[p]
        if valid is not None:
            valid = valid2
        v, f, a = v2, f2, a2
    vertex_edge = np.concatenate([np.full((V0, 2), -1, np.int32)] + edge_rows)
    return {"vertices": v, "faces": f, "attributes": a, "valid": (np.ones(len(v), bool) if valid is None else valid) if a is not None else None,
            "vertex_edge": vertex_edge, "face_parent": parent, "rounds": len(per_round), "converged": converged, "per_round": per_round,
            "keep": k, "limit": limit}


def view_edge_limit(vertices, camera_centers, focal_pixels, max_pixels):
    v, c = np.asarray(vertices, np.float64), np.asarray(camera_centers, np.float64)
    focal = np.broadcast_to(np.asarray(focal_pixels, np.float64).reshape(-1), (len(c),))
    d = np.sqrt(((v[:, None, :] - c[None]) ** 2).sum(-1)) / focal[None]
    return max_pixels * d.min(1)


# ---- constructions: small even-integer coordinates, so midpoints, squared lengths and doubled areas are exact -------------------------------------
def cube_grid(n=2, step=4):
    """The closed surface of a cube of n x n x n cells of side `step`: vertices on the surface grid, two triangles per cell face, all outward.
    (V, 3) float32, (12 n^2, 3) int32."""
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append([step * x for x in p])
        return index[p]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def at(di, dj):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        return vid(tuple(p))
                    a, b, c, d = at(0, 0), at(1, 0), at(1, 1), at(0, 1)
                    quad = [(a, b, c), (a, c, d)] if side == n else [(a, c, b), (a, d, c)]  # u x w = +axis
                    faces += quad
    return np.array(verts, np.float32), np.array(faces, np.int32)


def doubled_area_vectors(vertices, faces):
    """(F, 3) float64: the cross product of two edge vectors of every face; exact on small integer coordinates."""
    p = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])


def euler(V_used, faces):
    f = np.asarray(faces, np.int64)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    return V_used - len(e) + len(f)
