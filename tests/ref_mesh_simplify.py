"""numpy float64 reference of include/ts_simplify.h: vertex clustering on a uniform grid, quadric error placement and the duplicate-face
sweep, written operation by operation.  Every elementwise numpy operation below rounds once, like the kernel built with -ffp-contract=off;
the sequential sums are np.add.at, which applies its updates one by one in index order.  The numbering between the steps is
ref_mesh_weld.compact / remap_faces, as the product reuses compact_labels / remap_faces.
"""
import numpy as np

import ref_mesh_weld

MEAN, QUADRIC = 0, 1
MODES = {"mean": MEAN, "quadric": QUADRIC}
CELL_LIMIT = 2097152.0  # 2^21 cells per axis


def _f64(x):
    return np.float64(np.float32(x))


def cell_indices(vertices, origin, cell):
    """(c (V, 3) int64, valid (V,) bool): c = floor(((double)x - (double)o) / (double)cell); valid iff finite and 0 <= c < 2^21 per axis."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    o = np.array([_f64(a) for a in origin])
    with np.errstate(all="ignore"):
        g = (v.astype(np.float64) - o[None, :]) / _f64(cell)
        fl = np.floor(g)
        ok = np.isfinite(v) & (fl >= 0.0) & (fl < CELL_LIMIT)
    valid = ok.all(1)
    c = np.where(ok, fl, 0.0).astype(np.int64)
    return c, valid


def cluster_labels(vertices, origin, cell):
    """label (V,) int64: the smallest index among the valid vertices with the same key; an invalid vertex is its own label."""
    c, valid = cell_indices(vertices, origin, cell)
    key = (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]
    label = np.arange(len(c), dtype=np.int64)
    first = {}
    for i in np.nonzero(valid)[0]:
        label[i] = first.setdefault(int(key[i]), int(i))
    return label


def place(vertices, faces, remap, origin, cell, lam=1e-3, mode=QUADRIC, attributes=None, attr_valid=None):
    """dict: vertices (V', 3) float32, attributes (V', C) float32 / valid (V',) uint8 (None without attributes), member_count (V',) int64."""
    v32 = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    V = len(v32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    remap = np.asarray(remap, np.int64)
    n = int(remap.max()) + 1 if V else 0
    out = {"vertices": np.zeros((n, 3), np.float32), "attributes": None, "valid": None, "member_count": np.bincount(remap, minlength=n)}
    if V == 0:
        return out
    v = v32.astype(np.float64)
    c, valid = cell_indices(v32, origin, cell)
    head = np.full(n, V, np.int64)
    np.minimum.at(head, remap, np.arange(V))  # the first member of every cluster
    o = np.array([_f64(a) for a in origin])
    cw = _f64(cell)
    count = out["member_count"].astype(np.float64)
    with np.errstate(all="ignore"):
        cc = o[None, :] + cw * (c[head].astype(np.float64) + 0.5)  # (n, 3): the clusters' frames
        s = np.zeros((n, 3))
        np.add.at(s, remap, v - cc[remap])  # members in ascending index order
        m = s / count[:, None]
        x = m.copy()
        if mode == QUADRIC:
            ok = ((f >= 0) & (f < V)).all(1)
            fs = np.where(ok[:, None], f, 0)
            ok &= np.isfinite(v[fs]).all((1, 2))
            # incidence records (cluster, face) in ascending face order: vertex k unless an earlier valid vertex of the face named its cluster
            q, val = remap[fs], valid[fs]
            take = [ok & val[:, 0],
                    ok & val[:, 1] & ~(val[:, 0] & (q[:, 0] == q[:, 1])),
                    ok & val[:, 2] & ~(val[:, 0] & (q[:, 0] == q[:, 2])) & ~(val[:, 1] & (q[:, 1] == q[:, 2]))]
            rec_face = np.concatenate([np.nonzero(t)[0] for t in take])
            rec_cluster = np.concatenate([q[t, k] for k, t in enumerate(take)])
            order = np.argsort(rec_face, kind="stable")  # a cluster is named once per face, so face order is all that matters
            rec_face, rec_cluster = rec_face[order], rec_cluster[order]
            p = v[fs[rec_face]] - cc[rec_cluster][:, None, :]  # (R, 3, 3) in the cluster's frame
            p0, e1, e2 = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
            nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            d = -((nx * p0[:, 0] + ny * p0[:, 1]) + nz * p0[:, 2])
            acc = np.zeros((9, n))
            for row, term in enumerate((nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * d, ny * d, nz * d)):
                np.add.at(acc[row], rec_cluster, term)
            a00, a01, a02, a11, a12, a22, b0, b1, b2 = acc
            tr = (a00 + a11) + a22
            mu = _f64(lam) * tr
            a00, a11, a22 = a00 + mu, a11 + mu, a22 + mu
            r0, r1, r2 = mu * m[:, 0] - b0, mu * m[:, 1] - b1, mu * m[:, 2] - b2
            c00 = a11 * a22 - a12 * a12
            c01 = a02 * a12 - a01 * a22
            c02 = a01 * a12 - a02 * a11
            c11 = a00 * a22 - a02 * a02
            c12 = a01 * a02 - a00 * a12
            c22 = a00 * a11 - a01 * a01
            det = (a00 * c00 + a01 * c01) + a02 * c02
            y = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det,
                          ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                          ((c02 * r0 + c12 * r1) + c22 * r2) / det], 1)
            solved = np.isfinite(tr) & (tr > 0.0) & np.isfinite(det) & (det > 0.0) & np.isfinite(y).all(1)
            x = np.where(solved[:, None], y, m)
        half = 0.5 * cw
        x = np.minimum(np.maximum(x, -half), half)
        placed = (cc + x).astype(np.float32)
    out["vertices"] = np.where(valid[head][:, None], placed.view(np.uint32), v32[head].view(np.uint32)).view(np.float32)  # invalid: bit for bit
    if attributes is not None:
        a = np.ascontiguousarray(attributes, np.float32).reshape(V, -1).astype(np.float64)
        use = np.ones(V, bool) if attr_valid is None else np.asarray(attr_valid).reshape(V) != 0
        sums, cnt = np.zeros((n, a.shape[1])), np.zeros(n, np.int64)
        with np.errstate(all="ignore"):
            np.add.at(sums, remap[use], a[use])
            np.add.at(cnt, remap[use], 1)
            mean = (sums / cnt.astype(np.float64)[:, None]).astype(np.float32)
        out["attributes"] = np.where((cnt > 0)[:, None], mean.view(np.uint32), np.uint32(0)).view(np.float32)
        out["valid"] = (cnt > 0).astype(np.uint8)
    return out


def rotate_smallest_first(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    k = np.argmin(f, axis=1)  # distinct indices: one minimum
    rows = np.arange(len(f))
    return np.stack([f[rows, k], f[rows, (k + 1) % 3], f[rows, (k + 2) % 3]], 1)


def unique_faces(V, faces, keep):
    """(keep_out (F,) bool, duplicates, flaps)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    part = np.asarray(keep, bool) & ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    rot = rotate_smallest_first(np.where(part[:, None], f, np.array([0, 1, 2])))
    seen, keep_out = {}, np.zeros(len(f), bool)
    for i in np.nonzero(part)[0]:
        t = tuple(rot[i])
        if t not in seen:
            seen[t] = i
            keep_out[i] = True
    flaps = sum(1 for (a, b, c) in seen if (a, c, b) in seen)
    return keep_out, int(part.sum() - keep_out.sum()), int(flaps)


def simplify(vertices, faces, cell, origin, mode="quadric", lam=1e-3, attributes=None, attr_valid=None):
    """The whole pipeline, as diff_recon_hip.simplify_mesh chains it: dict of label, remap, num_vertices, vertices, attributes, valid,
    member_count, new_faces (F, 3), keep (after the sweep), keep_remap (before it), duplicates, flaps, faces (the kept ones)."""
    v32 = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    V = len(v32)
    label = cluster_labels(v32, origin, cell)
    remap, _, n = ref_mesh_weld.compact(label, v32, "first")
    placed = place(v32, faces, remap, origin, cell, lam, MODES[mode], attributes, attr_valid)
    new, keep_remap = ref_mesh_weld.remap_faces(V, faces, remap)
    keep, dup, flaps = unique_faces(n, new, keep_remap)
    return {"label": label, "remap": remap, "num_vertices": n, **placed, "new_faces": new, "keep_remap": keep_remap, "keep": keep,
            "duplicates": dup, "flaps": flaps, "faces": new[keep]}


# ---- what the tests measure and their fixtures ---------------------------------------------------------------------------------------------
def sphere_mesh():
    """The marching-tetrahedra sphere of the fixtures: (vertices (4834, 3) float32, faces (9664, 3) int64), closed."""
    import ref_volume
    tri, _ = ref_volume.extract(ref_volume.sphere_field((28, 28, 28), (13.63, 13.29, 13.57), 9.3), (28, 28, 28), (0, 0, 0), 1.0)
    return ref_volume.weld_exact(tri)


def cube_mesh(n=12, lo=0.37, hi=7.61):
    """A cube [lo, hi]^3 tessellated n x n per side with outward normals, vertices shared along the edges: (vertices float32, faces int64)."""
    t = (np.float64(lo) + (np.float64(hi) - np.float64(lo)) * np.arange(n + 1) / n).astype(np.float32)
    verts, index, faces = [], {}, []

    def vid(p):
        key = tuple(np.float32(x).tobytes() for x in p)
        if key not in index:
            index[key] = len(verts)
            verts.append(p)
        return index[key]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side, value in ((0, t[0]), (1, t[-1])):
            for i in range(n):
                for j in range(n):
                    def corner(a, b):
                        p = [0.0, 0.0, 0.0]
                        p[axis], p[u], p[w] = value, t[a], t[b]
                        return vid(tuple(p))
                    q = [corner(i, j), corner(i + 1, j), corner(i + 1, j + 1), corner(i, j + 1)]  # counter-clockwise seen from +axis
                    if side == 0:
                        q.reverse()
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return np.array(verts, np.float32), np.array(faces, np.int64)


def plane_grid(n=24, seed=5):
    """An n x n grid on the plane through (0.3, -0.2, 0.5) with unit normal nrm, rounded to fp32: (vertices, faces, point, normal)."""
    nrm = np.array([0.31, -0.52, 0.79])
    nrm /= np.linalg.norm(nrm)
    e1 = np.cross(nrm, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    p0 = np.array([0.3, -0.2, 0.5])
    a, b = np.meshgrid(np.arange(n + 1) * 0.37, np.arange(n + 1) * 0.41, indexing="ij")
    v = (p0[None, :] + a.reshape(-1, 1) * e1[None, :] + b.reshape(-1, 1) * e2[None, :]).astype(np.float32)
    idx = np.arange((n + 1) ** 2).reshape(n + 1, n + 1)
    q = np.stack([idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]], -1).reshape(-1, 4)
    f = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]]).astype(np.int64)
    return v, f, p0, nrm


def signed_volume(vertices, faces):
    import ref_volume
    return ref_volume.signed_volume(np.asarray(vertices, np.float32)[np.asarray(faces, np.int64)])


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)
