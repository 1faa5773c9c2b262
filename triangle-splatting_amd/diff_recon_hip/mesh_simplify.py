"""Making an indexed mesh smaller, on the device: vertex clustering on a uniform grid with quadric error placement (Lindstrom), the sweep
that removes the duplicate faces clustering leaves behind, and a small-piece filter.

    simplify_mesh(vertices, faces, cell, origin=None, placement="quadric", regularization=1e-3, vertex_attributes=None,
                  attribute_valid=None, faces_color=None) -> SimplifiedMesh
    drop_small_pieces(vertices, faces, min_faces) -> (vertices, faces, face_keep)
    simplify_fused(mesh, volume, simplify_cell=None, min_piece_faces=0)   both, on the grid of the volume a mesh was fused in (voxels); a
                                                                   ColoredMesh keeps its colours.  fuse_mesh(simplify_cell=...) calls it
    cluster_labels / place_clusters / unique_faces                 the three native steps, one call each

A marching-tetrahedra mesh (volume.py) has as many faces as the voxel grid cuts, whatever the shape; this is the pass that follows
extraction.  The result is a pure function of the input (include/ts_simplify.h), bit-equal to a numpy float64 reference:

    cells      c = floor(((double)x - (double)origin) / (double)cell) per axis; a vertex is valid iff it is finite and 0 <= c < 2^21
    clusters   the valid vertices of one cell; label = the smallest index; an invalid vertex is its own cluster and keeps its position
    numbering  weld_mesh's: clusters ranked by ascending label (compact_labels is reused)
    position   "mean": the float64 mean of the members in the cell's frame; "quadric": the minimiser of the summed squared distances to
               the planes of the faces that touch the cluster (area^2 weights), regularised towards the mean by `regularization` times the
               trace, solved by cofactors in float64; either way clamped to the cell, so a vertex never leaves its cell
    attributes the float64 mean of the members whose `attribute_valid` is set, per channel
    faces      remap_faces' rule (a face is dropped iff an index is out of range or two new indices are equal), then duplicates: among the
               kept faces with the same rotated triple only the smallest face index survives.  Opposite-oriented twins are both kept and
               counted in stats["flaps"].  Kept faces stay in their order.

Native code: libts_simplify.so beside this file (include/ts_simplify.h, csrc/mesh_simplify.hip), a seventh library because the export lists
of the other six are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError.  A cluster is one thread's
work (its sums are sequential by definition): `cell` is meant to be far below the mesh's extent."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, NamedTuple, Optional

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_simplify

from .mesh_weld import _device_of, _faces_arg, _vertices_arg, compact_labels, face_components, remap_faces

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_simplify.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The mesh simplification kernels have no CPU fallback."
    )
_lib = bind_simplify(C.CDLL(_LIB_PATH))

PLACEMENT_MODES = {"mean": 0, "quadric": 1}  # TSQ_PLACE_MEAN / TSQ_PLACE_QUADRIC
MAX_CHANNELS = 8                             # TSQ_MAX_CHANNELS


class SimplifiedMesh(NamedTuple):
    vertices: torch.Tensor                     # (V', 3) float32
    faces: torch.Tensor                        # (F', 3) int32: the kept faces, in their original order
    vertex_attributes: Optional[torch.Tensor]  # (V', C) float32, or None
    attribute_valid: Optional[torch.Tensor]    # (V',) bool, or None
    faces_color: Optional[torch.Tensor]        # (F', C): the kept faces' rows of the input colours, or None
    vertex_map: torch.Tensor                   # (V,) int32: old vertex -> new vertex
    face_keep: torch.Tensor                    # (F,) bool
    stats: Dict[str, object]


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsq_last_error().decode()} (ts2d error {rc})")


def _workspace(V: int, F: int, device) -> torch.Tensor:
    return torch.empty((_lib.tsq_workspace_bytes(V, F),), device=device, dtype=torch.uint8)


def _grid_args(origin, cell):
    o = tuple(float(x) for x in (origin.tolist() if isinstance(origin, torch.Tensor) else origin))
    cell = float(cell)
    if len(o) != 3 or not all(math.isfinite(x) for x in o):
        raise ValueError(f"origin must be three finite values, not {origin!r}")
    if not (math.isfinite(cell) and cell > 0.0):
        raise ValueError(f"cell must be finite and > 0, not {cell}")
    return o, cell


def cluster_labels(vertices: torch.Tensor, origin, cell: float) -> torch.Tensor:
    """(V,) int32: the smallest index among the valid vertices in the same grid cell; an invalid vertex (non-finite, or outside the 2^21
    cells per axis from `origin`) is its own label."""
    o, cell = _grid_args(origin, cell)
    v = _vertices_arg(vertices)
    device = _device_of("cluster_labels", v)
    V = v.shape[0]
    with torch.cuda.device(device):
        label = torch.empty((V,), device=device, dtype=torch.int32)
        if V:
            ws = _workspace(V, 0, device)
            _check(_lib.tsq_cluster_labels(V, v.data_ptr(), *o, cell, label.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream()),
                   "cluster_labels")
    return label


def place_clusters(vertices: torch.Tensor, faces: torch.Tensor, remap: torch.Tensor, origin, cell: float, placement: str = "quadric",
                   regularization: float = 1e-3, vertex_attributes: Optional[torch.Tensor] = None,
                   attribute_valid: Optional[torch.Tensor] = None):
    """One position per cluster of `remap` (the numbering of compact_labels): (vertices (V, 3) float32, attributes (V, C) float32 or None,
    valid (V,) bool or None, member_count (V,) int32), all with V rows of which the rows from the number of clusters on are zero.
    Nothing is read back."""
    if placement not in PLACEMENT_MODES:
        raise ValueError(f"placement must be one of {sorted(PLACEMENT_MODES)}, not {placement!r}")
    o, cell = _grid_args(origin, cell)
    lam = float(regularization)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError("regularization must be finite and >= 0")
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    device = _device_of("place_clusters", v, f, remap, vertex_attributes, attribute_valid)
    V, F = v.shape[0], f.shape[0]
    if remap.shape != (V,) or remap.dtype != torch.int32:
        raise RuntimeError("remap must be an int32 tensor with dimensions (num_vertices,)")
    attrs = mask = None
    channels = 0
    if vertex_attributes is not None:
        if vertex_attributes.dim() != 2 or vertex_attributes.shape[0] != V or not 1 <= vertex_attributes.shape[1] <= MAX_CHANNELS:
            raise RuntimeError(f"vertex_attributes must have dimensions (num_vertices, C) with 1 <= C <= {MAX_CHANNELS}")
        attrs = vertex_attributes.detach().to(torch.float32).contiguous()
        channels = attrs.shape[1]
        if attribute_valid is not None:
            if attribute_valid.shape != (V,):
                raise RuntimeError("attribute_valid must have dimensions (num_vertices,)")
            mask = (attribute_valid.detach() != 0).to(torch.uint8).contiguous()
    elif attribute_valid is not None:
        raise RuntimeError("attribute_valid needs vertex_attributes")
    with torch.cuda.device(device):
        remap = remap.contiguous()
        out = torch.empty((V, 3), device=device, dtype=torch.float32)
        out_attrs = torch.empty((V, channels), device=device, dtype=torch.float32) if attrs is not None else None
        out_valid = torch.empty((V,), device=device, dtype=torch.uint8) if attrs is not None else None
        members = torch.empty((V,), device=device, dtype=torch.int32)
        if V:
            ws = _workspace(V, F, device)
            _check(_lib.tsq_place(V, F, v.data_ptr(), f.data_ptr() if F else None, remap.data_ptr(), *o, cell, lam, PLACEMENT_MODES[placement],
                                  _native._ptr(attrs), _native._ptr(mask), channels, out.data_ptr(), _native._ptr(out_attrs),
                                  _native._ptr(out_valid), members.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream()), "place_clusters")
    return out, out_attrs, (out_valid != 0) if out_valid is not None else None, members


def unique_faces(num_vertices: int, faces: torch.Tensor, keep: torch.Tensor):
    """(keep (F,) bool, counts (2,) int64 on the device = {duplicates, flaps}): of the faces with `keep` set, indices in [0, num_vertices)
    and three distinct indices, the ones that survive the duplicate sweep.  Nothing is read back."""
    f = _faces_arg(faces)
    device = _device_of("unique_faces", f, keep)
    V, F = int(num_vertices), f.shape[0]
    if V < 0:
        raise ValueError("num_vertices must be >= 0")
    if keep.shape != (F,) or keep.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError("keep must be a bool or uint8 tensor with dimensions (num_faces,)")
    with torch.cuda.device(device):
        keep = keep.contiguous()
        out = torch.empty((F,), device=device, dtype=torch.bool)
        counts = torch.empty((2,), device=device, dtype=torch.int64)
        ws = _workspace(V, F, device) if F else None
        _check(_lib.tsq_unique_faces(V, F, f.data_ptr() if F else None, keep.data_ptr() if F else None, out.data_ptr() if F else None,
                                     counts.data_ptr(), _native._ptr(ws), ws.numel() if F else 0, _native.stream()), "unique_faces")
    return out, counts


def default_origin(vertices: torch.Tensor):
    """The per-axis minimum of the finite vertices (0 when there is none): the grid origin simplify_mesh takes when it is given none."""
    v = vertices.detach().to(torch.float32)
    finite = v[torch.isfinite(v).all(dim=1)]
    return tuple(finite.min(dim=0).values.tolist()) if finite.shape[0] else (0.0, 0.0, 0.0)


def simplify_mesh(vertices: torch.Tensor, faces: torch.Tensor, cell: float, origin=None, placement: str = "quadric",
                  regularization: float = 1e-3, vertex_attributes: Optional[torch.Tensor] = None,
                  attribute_valid: Optional[torch.Tensor] = None, faces_color: Optional[torch.Tensor] = None) -> SimplifiedMesh:
    """Simplifies an indexed mesh (module text).  origin=None: the per-axis minimum of the finite vertices.  stats: num_vertices_in,
    num_vertices, num_faces_in, num_faces, collapsed (faces dropped because two of their vertices fell into one cluster, or an index was out
    of range), duplicates, flaps, largest_cluster and max_displacement (the largest distance between a finite vertex and its cluster's
    position; float)."""
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    device = _device_of("simplify_mesh", v, f, vertex_attributes, attribute_valid, faces_color)
    V, F = v.shape[0], f.shape[0]
    if faces_color is not None and (faces_color.dim() != 2 or faces_color.shape[0] != F):
        raise RuntimeError("faces_color must have dimensions (num_faces, C)")
    if origin is None:
        origin = default_origin(v)
    with torch.cuda.device(device):
        label = cluster_labels(v, origin, cell)
        remap, _, n = compact_labels(label, v, "first")  # the numbering and V'; the positions come from place_clusters
        placed, attrs, valid, members = place_clusters(v, f, remap, origin, cell, placement, regularization, vertex_attributes, attribute_valid)
        new_faces, keep_remap = remap_faces(V, f, remap)
        keep, counts = unique_faces(n, new_faces, keep_remap)
        duplicates, flaps = (int(x) for x in counts.tolist())
        placed = placed[:n].contiguous()
        largest, displacement = 0, 0.0
        if V:
            largest = int(members[:n].max().item())
            d = (v.to(torch.float64) - placed[remap.to(torch.int64)].to(torch.float64)).norm(dim=1)
            d = d[torch.isfinite(d)]
            displacement = float(d.max().item()) if d.numel() else 0.0
        kept = new_faces[keep].contiguous()
        color = faces_color[keep].contiguous() if faces_color is not None else None
        collapsed = F - int(keep_remap.sum().item())
    stats = {"num_vertices_in": V, "num_vertices": n, "num_faces_in": F, "num_faces": int(kept.shape[0]), "collapsed": collapsed,
             "duplicates": duplicates, "flaps": flaps, "largest_cluster": largest, "max_displacement": displacement}
    return SimplifiedMesh(placed, kept, attrs[:n].contiguous() if attrs is not None else None,
                          valid[:n].contiguous() if valid is not None else None, color, remap, keep, stats)


def drop_small_pieces(vertices: torch.Tensor, faces: torch.Tensor, min_faces: int):
    """(vertices (V', 3), faces (F', 3) int32, face_keep (F,) bool): the faces of the connected pieces (face_components: joined along face
    edges) with at least `min_faces` faces, in their order, and the vertices they name, in theirs.  A face with an index outside [0, V) is
    dropped.  min_faces <= 1 keeps every piece."""
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    device = _device_of("drop_small_pieces", v, f)
    V, F = v.shape[0], f.shape[0]
    with torch.cuda.device(device):
        valid = ((f >= 0) & (f < V)).all(dim=1) if F else torch.zeros((0,), device=device, dtype=torch.bool)
        keep = valid.clone()
        if F and V:
            label = face_components(V, f).to(torch.int64)
            piece = label[f[:, 0].clamp(0, V - 1).to(torch.int64)]  # every vertex of a valid face has the same label
            size = torch.bincount(piece[valid], minlength=V)
            keep = valid & (size[piece] >= int(min_faces))
        used = torch.zeros((V,), device=device, dtype=torch.bool)
        kept = f[keep].to(torch.int64)
        used[kept.reshape(-1)] = True
        new_index = torch.cumsum(used.to(torch.int64), 0) - 1
        out_faces = new_index[kept].to(torch.int32).reshape(-1, 3).contiguous()
        out_vertices = v[used].contiguous()
    return out_vertices, out_faces, keep


def simplify_fused(mesh, volume, simplify_cell: Optional[float] = None, min_piece_faces: int = 0):
    """The pass behind a fusion: `mesh` is what volume.extract() / fuse_mesh / fuse_colored_mesh returned for `volume` (a WeldedMesh or a
    ColoredMesh), simplify_cell the cell size in voxels on the volume's own grid (None: no clustering), min_piece_faces the piece filter
    (0: none): simplify_mesh, then drop_small_pieces.  Returns the same kind of mesh: a ColoredMesh carries vertex_color / color_valid
    through as attributes (a cluster takes the mean colour of its members that have one, 0.5 where none has); a WeldedMesh gets vertex_map
    (-1 for a vertex whose piece was dropped) and face_keep from the level set to the result.  stats keeps the fusion's entries, updates
    num_vertices / num_faces and gains simplify_mesh's under "simplify" and the faces the piece filter removed under "small_piece_faces"."""
    if simplify_cell is None and int(min_piece_faces) <= 0:
        return mesh
    v, f = mesh.vertices, mesh.faces
    device = _device_of("simplify_fused", v, f)
    coloured = hasattr(mesh, "vertex_color")
    color, valid = (mesh.vertex_color, mesh.color_valid) if coloured else (None, None)
    vertex_map = torch.arange(v.shape[0], device=device, dtype=torch.int32)
    face_keep = torch.ones((f.shape[0],), device=device, dtype=torch.bool)
    stats = dict(mesh.stats)
    if simplify_cell is not None:
        s = simplify_mesh(v, f, float(simplify_cell) * volume.voxel_size, volume.origin, vertex_attributes=color, attribute_valid=valid)
        v, f, color, valid, vertex_map, face_keep = s.vertices, s.faces, s.vertex_attributes, s.attribute_valid, s.vertex_map, s.face_keep
        stats["simplify"] = s.stats
    if int(min_piece_faces) > 0:
        V = v.shape[0]
        v2, f2, keep2 = drop_small_pieces(v, f, min_piece_faces)
        used = torch.zeros((V,), device=device, dtype=torch.bool)
        used[f[keep2].to(torch.int64).reshape(-1)] = True
        new_index = torch.where(used, torch.cumsum(used.to(torch.int64), 0) - 1, torch.full((V,), -1, device=device, dtype=torch.int64))
        vertex_map = new_index[vertex_map.to(torch.int64)].to(torch.int32) if V else vertex_map
        face_keep = face_keep.clone()
        face_keep[face_keep.clone()] = keep2
        stats["small_piece_faces"] = int(f.shape[0] - f2.shape[0])
        if coloured:
            color, valid = color[used].contiguous(), valid[used].contiguous()
        v, f = v2, f2
    stats.update(num_vertices=int(v.shape[0]), num_faces=int(f.shape[0]))
    if coloured:
        color = torch.where(valid[:, None], color, torch.full_like(color, 0.5))
        return mesh._replace(vertices=v, faces=f, vertex_color=color, color_valid=valid, stats=stats)
    return mesh._replace(vertices=v, faces=f, faces_color=None, vertex_map=vertex_map, face_keep=face_keep, stats=stats)


__all__ = ["SimplifiedMesh", "simplify_mesh", "drop_small_pieces", "simplify_fused", "cluster_labels", "place_clusters", "unique_faces", "default_origin",
           "PLACEMENT_MODES"]
