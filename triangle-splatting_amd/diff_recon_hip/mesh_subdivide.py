"""Making an indexed mesh finer, on the device: the table of its edges, and the conforming split of its faces at the midpoints of marked edges.

    mesh_edges(num_vertices, faces, keep=None, vertices=None) -> MeshEdges        the unique edges, their use counts and lengths
    split_edges(vertices, faces, max_edge=None, vertex_limit=None, ...) -> SplitMesh    one round
    split_long_edges(vertices, faces, max_edge=None, vertex_limit=None, ..., max_rounds=16) -> SplitMesh    rounds until nothing is marked
    subdivide_mesh(vertices, faces, levels=1, ...) -> SplitMesh                   `levels` rounds over all edges: F 4^levels faces
    view_edge_limit(vertices, camera_centers, focal_pixels, max_pixels)           the per-vertex limit that spans max_pixels pixels
    split_fused(mesh, max_edge)                                                   the pass behind a weld or a fusion

weld_mesh, simplify_mesh and fill_holes leave triangles of very different sizes: bake_face_colors gives a face that covers thousands of pixels
one flat colour, vertex colours are interpolated linearly across a long edge, and a Taubin step takes its largest moves there.  This is the
pass that bounds the edge length of a mesh.  The result is a pure function of the input (include/ts_subdivide.h), bit-equal
to a numpy reference (tests/ref_mesh_subdivide.py):

    edge     the undirected edges (lo, hi) of the faces that take part (kept, indices in range and pairwise distinct), numbered in ascending
             (lo, hi); length2 = (dx dx + dy dy) + dz dz in float64, taken from lo to hi once, so both neighbours see one value
    mark     every edge / length2 > max_edge^2 / length2 > min(limit[lo], limit[hi])^2; never an edge with a coordinate that is not finite
    vertex   one per marked edge, numbered from V in ascending edge: (float)((p_lo + p_hi) 0.5); attributes likewise where both ends have
             one, the valid end's where one has, invalid where neither has
    faces    0, 1, 2 or 3 marked edges give 1, 2, 3 or 4 pieces in the parent's orientation and in a fixed order; with 2 the remaining quad
             is cut by its shorter diagonal (on a tie by the smaller index).  Marks belong to edges, so neighbours agree: no T-junction
             between faces that take part.  A face that does not take part is copied, and keeps its long edge beside a split neighbour

Native code: libts_subdivide.so beside this file (include/ts_subdivide.h, csrc/mesh_subdivide.hip), a sixteenth library because the export
lists of the other fifteen are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, NamedTuple, Optional

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_subdivide

from .mesh_weld import _device_of, _faces_arg, _keep_arg, _vertices_arg

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_subdivide.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The edge-table and edge-split kernels have no CPU fallback."
    )
_lib = bind_subdivide(C.CDLL(_LIB_PATH))

MARK_ALL, MARK_LONGER, MARK_VERTEX_LIMIT = 0, 1, 2          # TSD_MARK_*
COUNT_NAMES = ("edges", "boundary", "manifold", "nonmanifold")  # tsd_edges' four words
TOTAL_NAMES = ("edges", "marked", "out_faces", "faces_split")   # tsd_split's four words


class MeshEdges(NamedTuple):
    edge_vertices: torch.Tensor     # (E, 2) int32: (lo, hi), ascending
    edge_use: torch.Tensor          # (E,) int32: the number of participating faces on the edge
    length: Optional[torch.Tensor]  # (E,) float64: sqrt(length2); NaN where an end is not finite; None without vertices
    half_edge_edge: torch.Tensor    # (3 F,) int32: the edge of half-edge 3 f + k, or -1
    stats: Dict[str, int]           # COUNT_NAMES


class SplitMesh(NamedTuple):
    vertices: torch.Tensor                     # (V + new, 3) float32: the input's vertices bit for bit, then the midpoints
    faces: torch.Tensor                        # (F', 3) int32
    vertex_attributes: Optional[torch.Tensor]  # (V + new, C) float32, or None
    attribute_valid: Optional[torch.Tensor]    # (V + new,) bool, or None
    new_vertex: torch.Tensor                   # (V + new,) bool
    vertex_edge: torch.Tensor                  # (V + new, 2) int32: the (lo, hi) a new vertex halves (indices of this mesh), -1 on the input's
    face_parent: torch.Tensor                  # (F',) int32: the input face every face is a piece of
    face_attributes: Optional[torch.Tensor]    # (F', ...) the input's rows through face_parent, or None
    stats: Dict[str, object]


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsd_last_error().decode()} (ts2d error {rc})")


def _workspace(V: int, F: int, device) -> torch.Tensor:
    return torch.empty((_lib.tsd_workspace_bytes(V, F),), device=device, dtype=torch.uint8)


def _edges_arrays(V: int, f: torch.Tensor, k: Optional[torch.Tensor], v: Optional[torch.Tensor], device):
    """(edge_vertices (3 F, 2), edge_use (3 F,), edge_length2 (3 F,) float64 or None, half_edge_edge (3 F,), counts (4,) int64) as tsd_edges
    writes them, to their capacity.  Nothing is read back."""
    F = f.shape[0]
    with torch.cuda.device(device):
        ev = torch.empty((3 * F, 2), device=device, dtype=torch.int32)
        use = torch.empty((3 * F,), device=device, dtype=torch.int32)
        length2 = torch.empty((3 * F,), device=device, dtype=torch.float64) if v is not None else None
        hee = torch.empty((3 * F,), device=device, dtype=torch.int32)
        counts = torch.empty((4,), device=device, dtype=torch.int64)
        ws = _workspace(V, F, device) if F else None
        ptr = (lambda t: t.data_ptr() if t is not None and t.numel() else None)
        _check(_lib.tsd_edges(V, F, ptr(v), ptr(f), _native._ptr(k), ptr(ev), ptr(use), ptr(length2), ptr(hee), counts.data_ptr(),
                              _native._ptr(ws), ws.numel() if ws is not None else 0, _native.stream()), "mesh_edges")
    return ev, use, length2, hee, counts


def _split_arrays(v: torch.Tensor, f: torch.Tensor, k: Optional[torch.Tensor], mode: int, max_edge: float, limit: Optional[torch.Tensor],
                  attrs: Optional[torch.Tensor], valid: Optional[torch.Tensor], device):
    """(new_vertices (3 F, 3), new_attributes (3 F, C) or None, new_attr_valid (3 F,) uint8 or None, new_vertex_edge (3 F, 2), out_faces
    (4 F, 3), out_face_parent (4 F,), totals (4,) int64) as tsd_split writes them, to their capacity.  Nothing is read back."""
    V, F = v.shape[0], f.shape[0]
    channels = attrs.shape[1] if attrs is not None else 0
    with torch.cuda.device(device):
        nv = torch.empty((3 * F, 3), device=device, dtype=torch.float32)
        na = torch.empty((3 * F, channels), device=device, dtype=torch.float32) if channels else None
        nvalid = torch.empty((3 * F,), device=device, dtype=torch.uint8) if channels else None
        nedge = torch.empty((3 * F, 2), device=device, dtype=torch.int32)
        out_faces = torch.empty((4 * F, 3), device=device, dtype=torch.int32)
        parent = torch.empty((4 * F,), device=device, dtype=torch.int32)
        totals = torch.empty((4,), device=device, dtype=torch.int64)
        ws = _workspace(V, F, device) if F else None
        ptr = (lambda t: t.data_ptr() if t is not None and t.numel() else None)
        _check(_lib.tsd_split(V, F, ptr(v), ptr(f), _native._ptr(k), mode, max_edge, ptr(limit), ptr(attrs) if channels else None,
                              _native._ptr(valid) if channels else None, channels, ptr(nv), ptr(na), ptr(nvalid), ptr(nedge), ptr(out_faces),
                              ptr(parent), totals.data_ptr(), _native._ptr(ws), ws.numel() if ws is not None else 0, _native.stream()),
               "split_edges")
    return nv, na, nvalid, nedge, out_faces, parent, totals


def mesh_edges(num_vertices: int, faces: torch.Tensor, keep: Optional[torch.Tensor] = None, vertices: Optional[torch.Tensor] = None) -> MeshEdges:
    """The edge table of an indexed mesh (module text).  vertices (V, 3): the lengths are formed as well.  stats: the four counts of tsd_edges
    under COUNT_NAMES, half of vertex_adjacency's entry counts on the same faces; one host read."""
    V = int(num_vertices)
    if V < 0:
        raise ValueError("num_vertices must be >= 0")
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    v = None
    if vertices is not None:
        v = _vertices_arg(vertices)
        if v.shape[0] != V:
            raise RuntimeError("vertices must have dimensions (num_vertices, 3)")
    device = _device_of("mesh_edges", f, k, v)
    ev, use, length2, hee, counts = _edges_arrays(V, f, k, v, device)
    stats = dict(zip(COUNT_NAMES, (int(x) for x in counts.tolist())))
    E = stats["edges"]
    return MeshEdges(ev[:E], use[:E], length2[:E].sqrt() if length2 is not None else None, hee, stats)


def _attribute_args(V: int, vertex_attributes, attribute_valid):
    attrs = valid = None
    if vertex_attributes is not None:
        if vertex_attributes.dim() != 2 or vertex_attributes.shape[0] != V:
            raise RuntimeError("vertex_attributes must have dimensions (num_vertices, C)")
        attrs = vertex_attributes.detach().to(torch.float32).contiguous()
        if attribute_valid is not None:
            if attribute_valid.shape != (V,) or attribute_valid.dtype not in (torch.bool, torch.uint8):
                raise RuntimeError("attribute_valid must be a bool or uint8 tensor with dimensions (num_vertices,)")
            valid = attribute_valid.contiguous()
    elif attribute_valid is not None:
        raise RuntimeError("attribute_valid needs vertex_attributes")
    return attrs, valid


def _limit_args(V: int, max_edge, vertex_limit):
    """(mode, max_edge as float, vertex_limit (V,) float32 or None)."""
    if max_edge is not None and vertex_limit is not None:
        raise ValueError("give max_edge or vertex_limit, not both")
    if max_edge is not None:
        max_edge = float(max_edge)
        if not max_edge >= 0.0:
            raise ValueError("max_edge must be >= 0")
        return MARK_LONGER, max_edge, None
    if vertex_limit is not None:
        if vertex_limit.shape != (V,):
            raise RuntimeError("vertex_limit must have dimensions (num_vertices,)")
        return MARK_VERTEX_LIMIT, 0.0, vertex_limit.detach().to(torch.float32).contiguous()
    return MARK_ALL, 0.0, None


def _round(v, f, k, mode, max_edge, limit, attrs, valid, device):
    """One call of tsd_split and ONE host read (its totals); the outputs cut to the numbers written and joined to the input's vertices.
    Returns (vertices, faces, attributes, valid as bool, vertex_edge of the new rows, face_parent, totals as a dict)."""
    V = v.shape[0]
    nv, na, nvalid, nedge, out_faces, parent, totals = _split_arrays(v, f, k, mode, max_edge, limit, attrs, valid, device)
    t = dict(zip(TOTAL_NAMES, (int(x) for x in totals.tolist())))
    n, nf = t["marked"], t["out_faces"]
    with torch.cuda.device(device):
        out_v = torch.cat([v, nv[:n]])
        out_a = out_valid = None
        if attrs is not None:
            was = valid != 0 if valid is not None else torch.ones((V,), device=device, dtype=torch.bool)
            if attrs.shape[1]:
                out_a, out_valid = torch.cat([attrs, na[:n]]), torch.cat([was, nvalid[:n] != 0])
            else:  # no channel: nothing to interpolate, a new vertex is valid iff an end is
                ends = nedge[:n].to(torch.int64)
                out_a, out_valid = attrs.new_zeros((V + n, 0)), torch.cat([was, was[ends[:, 0]] | was[ends[:, 1]]])
    return out_v, out_faces[:nf], out_a, out_valid, nedge[:n], parent[:nf], t


def _result(V0, v, f, a, valid, edges, parent, face_attributes, stats, device) -> SplitMesh:
    with torch.cuda.device(device):
        new_vertex = torch.zeros((v.shape[0],), device=device, dtype=torch.bool)
        new_vertex[V0:] = True
        vertex_edge = torch.cat([torch.full((V0, 2), -1, device=device, dtype=torch.int32)] + edges)
        fa = face_attributes[parent.to(torch.int64)] if face_attributes is not None else None
    return SplitMesh(v, f, a, valid, new_vertex, vertex_edge, parent, fa, stats)


def _face_attributes_arg(face_attributes, F: int):
    if face_attributes is not None and (face_attributes.dim() < 1 or face_attributes.shape[0] != F):
        raise RuntimeError("face_attributes must have num_faces rows")
    return face_attributes


def split_edges(vertices: torch.Tensor, faces: torch.Tensor, max_edge: Optional[float] = None, vertex_limit: Optional[torch.Tensor] = None,
                vertex_attributes: Optional[torch.Tensor] = None, attribute_valid: Optional[torch.Tensor] = None,
                keep: Optional[torch.Tensor] = None, face_attributes: Optional[torch.Tensor] = None) -> SplitMesh:
    """One round of the split (module text).  max_edge: the edges longer than it are marked; vertex_limit (V,): the edges longer than the
    smaller limit of their ends; neither: all edges.  The input's vertices come first, bit for bit; `keep` only says which faces take part, all
    faces are returned; face_attributes (F, ...) are carried by face_parent.  stats: tsd_split's totals under TOTAL_NAMES; one host read."""
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    V = v.shape[0]
    attrs, valid = _attribute_args(V, vertex_attributes, attribute_valid)
    mode, max_edge, limit = _limit_args(V, max_edge, vertex_limit)
    face_attributes = _face_attributes_arg(face_attributes, f.shape[0])
    device = _device_of("split_edges", v, f, k, limit, attrs, valid, face_attributes)
    out_v, out_f, out_a, out_valid, edges, parent, t = _round(v, f, k, mode, max_edge, limit, attrs, valid, device)
    return _result(V, out_v, out_f, out_a, out_valid, [edges], parent, face_attributes, dict(t, new_vertices=t["marked"]), device)


def _rounds(what, vertices, faces, max_edge, vertex_limit, vertex_attributes, attribute_valid, keep, face_attributes, calls) -> SplitMesh:
    """At most `calls` rounds, until one marks nothing; the state of a round is (vertices, faces, keep, attributes, valid, limit)."""
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    V0, F0 = v.shape[0], f.shape[0]
    attrs, valid = _attribute_args(V0, vertex_attributes, attribute_valid)
    mode, max_edge, limit = _limit_args(V0, max_edge, vertex_limit)
    face_attributes = _face_attributes_arg(face_attributes, F0)
    device = _device_of(what, v, f, k, limit, attrs, valid, face_attributes)
    C0 = attrs.shape[1] if attrs is not None else 0
    # the limit rides as one more interpolated attribute column where every vertex is valid; beside a validity mask, where a column would
    # take the one-end rule, the same expression is formed from the round's vertex_edge instead
    ride = limit is not None and valid is None
    work = attrs
    if ride:
        work = torch.cat([attrs, limit[:, None]], dim=1) if attrs is not None else limit[:, None].contiguous()
    with torch.cuda.device(device):
        parent = torch.arange(F0, device=device, dtype=torch.int32)
    edges, per_round, converged = [], [], False
    for _ in range(calls):
        v2, f2, work2, valid2, e, p, t = _round(v, f, k, mode, max_edge, limit, work, valid, device)
        if t["marked"] == 0:  # the round copied its input
            converged = True
            break
        per_round.append(t)
        edges.append(e)
        if ride:
            limit = work2[:, -1].contiguous()
        elif limit is not None:
            ends = e.to(torch.int64)
            limit = torch.cat([limit, ((limit[ends[:, 0]].double() + limit[ends[:, 1]].double()) * 0.5).float()])
        at = p.to(torch.int64)
        parent = parent[at]
        if k is not None:
            k = k[at].contiguous()
        if valid is not None:
            valid = valid2
        v, f, work = v2, f2, work2
    out_a = out_valid = None
    if attrs is not None:
        out_a = work[:, :C0].contiguous() if ride else work
        out_valid = valid != 0 if valid is not None else torch.ones((v.shape[0],), device=device, dtype=torch.bool)
    stats = {"rounds": len(per_round), "converged": converged, "new_vertices": int(v.shape[0]) - V0, "faces": int(f.shape[0]),
             "faces_split": sum(t["faces_split"] for t in per_round), "per_round": per_round}
    return _result(V0, v, f, out_a, out_valid, edges, parent, face_attributes, stats, device)


def split_long_edges(vertices: torch.Tensor, faces: torch.Tensor, max_edge: Optional[float] = None, vertex_limit: Optional[torch.Tensor] = None,
                     vertex_attributes: Optional[torch.Tensor] = None, attribute_valid: Optional[torch.Tensor] = None,
                     keep: Optional[torch.Tensor] = None, face_attributes: Optional[torch.Tensor] = None, max_rounds: int = 16) -> SplitMesh:
    """Rounds of split_edges until a round marks nothing, at most max_rounds of them: once converged no finite edge of a face that takes
    part is longer than max_edge (than the smaller limit of its ends).  A midpoint halves an edge, so an edge of length l is done after
    ceil(log2(l / max_edge)) rounds.  A new vertex takes the mean of its ends' limits (as one more attribute column); pieces inherit their
    parent's keep; face_parent and vertex_edge are composed over the rounds, face_parent back to the input's faces.  stats: rounds,
    converged (the last round marked nothing), new_vertices, faces, faces_split, per_round (TOTAL_NAMES each); one host read per round."""
    if max_edge is None and vertex_limit is None:
        raise ValueError("split_long_edges needs max_edge or vertex_limit")
    if int(max_rounds) < 1:
        raise ValueError("max_rounds must be >= 1")
    return _rounds("split_long_edges", vertices, faces, max_edge, vertex_limit, vertex_attributes, attribute_valid, keep, face_attributes,
                   int(max_rounds))


def subdivide_mesh(vertices: torch.Tensor, faces: torch.Tensor, levels: int = 1, vertex_attributes: Optional[torch.Tensor] = None,
                   attribute_valid: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                   face_attributes: Optional[torch.Tensor] = None) -> SplitMesh:
    """`levels` rounds of all-edge splits: every face that takes part and has finite vertices becomes 4^levels faces, midpoints only (no
    smoothing rule: the vertices of the input do not move).  Returns what split_long_edges returns."""
    if int(levels) < 0:
        raise ValueError("levels must be >= 0")
    return _rounds("subdivide_mesh", vertices, faces, None, None, vertex_attributes, attribute_valid, keep, face_attributes, int(levels))


def view_edge_limit(vertices: torch.Tensor, camera_centers: torch.Tensor, focal_pixels, max_pixels: float) -> torch.Tensor:
    """(V,) float32: max_pixels * min_c |v - c| / focal_c, the world length that spans max_pixels pixels in the nearest view, for split_edges'
    vertex_limit.  camera_centers (C, 3); focal_pixels: a number or (C,) values.  Plain torch, on the vertices' device; one camera at a time."""
    if vertices.dim() != 2 or vertices.shape[1] != 3 or camera_centers.dim() != 2 or camera_centers.shape[1] != 3 or camera_centers.shape[0] < 1:
        raise RuntimeError("vertices must have dimensions (V, 3) and camera_centers (C, 3) with C >= 1")
    max_pixels = float(max_pixels)
    if not (math.isfinite(max_pixels) and max_pixels > 0.0):
        raise ValueError("max_pixels must be finite and > 0")
    v = vertices.detach().to(torch.float32)
    c = camera_centers.detach().to(device=v.device, dtype=torch.float32)
    focal = torch.as_tensor(focal_pixels, dtype=torch.float32, device=v.device).reshape(-1).expand(c.shape[0]) if not isinstance(focal_pixels, (int, float)) \
        else torch.full((c.shape[0],), float(focal_pixels), device=v.device)
    if not bool((focal > 0).all()):
        raise ValueError("focal_pixels must be > 0")
    best = torch.full((v.shape[0],), float("inf"), device=v.device)
    for i in range(c.shape[0]):
        best = torch.minimum(best, (v - c[i]).square().sum(1).sqrt() / focal[i])
    return best * max_pixels


def split_fused(mesh, max_edge: float):
    """The pass behind a weld or a fusion: `mesh` is a WeldedMesh or a ColoredMesh (weld_mesh, volume.extract(), fuse_mesh, fuse_colored_mesh,
    simplify_fused, fill_fused ...); split_long_edges with max_edge.  Returns the same kind of mesh: a ColoredMesh carries vertex_color /
    color_valid through as attributes (a midpoint takes the mean colour of its ends, the colour of the one end that has one, 0.5 where
    neither has); a WeldedMesh keeps vertex_map / face_keep (they speak of the soup, whose vertices keep their indices) and faces_color
    follows face_parent.  stats keeps the mesh's entries, updates num_vertices / num_faces and gains split_long_edges' under "split"
    with face_parent beside them."""
    coloured = hasattr(mesh, "vertex_color")
    color, valid = (mesh.vertex_color, mesh.color_valid) if coloured else (None, None)
    r = split_long_edges(mesh.vertices, mesh.faces, max_edge=max_edge, vertex_attributes=color, attribute_valid=valid,
                         face_attributes=None if coloured else mesh.faces_color)
    stats = dict(mesh.stats)
    stats["split"] = dict(r.stats, face_parent=r.face_parent)
    stats.update(num_vertices=int(r.vertices.shape[0]), num_faces=int(r.faces.shape[0]))
    if coloured:
        color = torch.where(r.attribute_valid[:, None], r.vertex_attributes, torch.full_like(r.vertex_attributes, 0.5))
        return mesh._replace(vertices=r.vertices, faces=r.faces, vertex_color=color, color_valid=r.attribute_valid, stats=stats)
    return mesh._replace(vertices=r.vertices, faces=r.faces, faces_color=r.face_attributes, stats=stats)


__all__ = ["MeshEdges", "SplitMesh", "mesh_edges", "split_edges", "split_long_edges", "subdivide_mesh", "view_edge_limit", "split_fused",
           "MARK_ALL", "MARK_LONGER", "MARK_VERTEX_LIMIT", "COUNT_NAMES", "TOTAL_NAMES"]
