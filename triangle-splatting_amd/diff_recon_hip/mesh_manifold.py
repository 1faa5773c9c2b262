"""Making an indexed mesh manifold, on the device: the fans of every vertex found and numbered, and every extra fan given a vertex of its own.

    vertex_fans(num_vertices, faces, keep=None) -> VertexFans                     the fan of every corner, the number of fans per vertex
    split_nonmanifold(vertices, faces, vertex_attributes=None, attribute_valid=None, keep=None, fans=None) -> ManifoldMesh
    manifold_fused(mesh)                                                          the pass behind simplify_fused, before fill_fused

simplify_mesh's pinched cells leave edges that three faces share and vertices where two sheets touch; smooth_mesh pulls such sheets together
and fill_holes leaves every hole that touches a pinch open.  This is the pass that turns such a mesh into an edge-manifold and
vertex-manifold one.  The result is a pure function of the input (include/ts_manifold.h), bit-equal to a numpy reference;
there is no floating-point arithmetic in it, positions and attributes are copied bit for bit:

    corner   face f, slot k, is corner 3 f + k at vertex faces[f][k], and half-edge 3 f + k from there to faces[f][(k + 1) % 3]
    link     an edge used by exactly two participating half-edges (in either direction) links the corners of its two faces at each of its
             ends; an edge used once or three times and more links nothing
    fan      a connected component of the links: a path or a cycle of faces around one vertex, labelled by its smallest corner
    split    at every vertex the fan with the smallest label keeps the vertex, every other fan gets a new vertex, numbered from V in
             ascending label; faces that do not take part (not kept, an index out of range or repeated) come back bit for bit

A pinch where two holes meet becomes ONE boundary loop over both copies of the vertex (two 3-loops become one 6-loop): the holes are merged,
not paired.  Edges used twice in the same direction (an orientation conflict) are counted and still linked, not fixed.

Native code: libts_manifold.so beside this file (include/ts_manifold.h, csrc/mesh_manifold.hip), a tenth library because the export lists
of the other nine are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, NamedTuple, Optional

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_manifold

from .mesh_weld import _device_of, _faces_arg, _keep_arg, _vertices_arg

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_manifold.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The vertex-fan and non-manifold split kernels have no CPU fallback."
    )
_lib = bind_manifold(C.CDLL(_LIB_PATH))

COUNT_NAMES = ("corners", "fans", "fan_vertices", "split_vertices", "nonmanifold_edges", "same_direction_edges")  # tsf_fans' six words


class VertexFans(NamedTuple):
    corner_fan: torch.Tensor   # (3 F,) int32: the smallest corner of every corner's fan, or -1
    vertex_fans: torch.Tensor  # (V,) int32: the number of fans at every vertex
    stats: Dict[str, int]      # COUNT_NAMES and new_vertices = fans - fan_vertices


class ManifoldMesh(NamedTuple):
    vertices: torch.Tensor                     # (V + new, 3) float32: the input's vertices, then the copies
    faces: torch.Tensor                        # (F, 3) int32
    vertex_attributes: Optional[torch.Tensor]  # (V + new, C) float32, or None
    attribute_valid: Optional[torch.Tensor]    # (V + new,) bool, or None
    source_vertex: torch.Tensor                # (V + new,) int32: the input vertex every vertex copies; the identity on the first V
    new_vertex: torch.Tensor                   # (V + new,) bool
    fans: VertexFans
    stats: Dict[str, int]


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsf_last_error().decode()} (ts2d error {rc})")


def _workspace(V: int, F: int, device) -> torch.Tensor:
    return torch.empty((_lib.tsf_workspace_bytes(V, F),), device=device, dtype=torch.uint8)


def _fans_arrays(V: int, f: torch.Tensor, k: Optional[torch.Tensor], device):
    """(corner_fan (3 F,), vertex_fans (V,), counts (6,) int64) as tsf_fans writes them.  Nothing is read back."""
    F = f.shape[0]
    with torch.cuda.device(device):
        corner_fan = torch.empty((3 * F,), device=device, dtype=torch.int32)
        fans = torch.empty((V,), device=device, dtype=torch.int32)
        counts = torch.empty((6,), device=device, dtype=torch.int64)
        ws = _workspace(V, F, device) if V and F else None
        _check(_lib.tsf_fans(V, F, f.data_ptr() if F else None, _native._ptr(k), corner_fan.data_ptr() if F else None,
                             fans.data_ptr() if V else None, counts.data_ptr(), _native._ptr(ws), ws.numel() if ws is not None else 0,
                             _native.stream()), "vertex_fans")
    return corner_fan, fans, counts


def _split_arrays(V: int, f: torch.Tensor, k: Optional[torch.Tensor], corner_fan: torch.Tensor, capacity: int, device):
    """(out_faces (F, 3), new_vertex_source (capacity,), new_vertex_fan (capacity,), totals (2,) int64) as tsf_split writes them."""
    F = f.shape[0]
    with torch.cuda.device(device):
        out_faces = torch.empty((F, 3), device=device, dtype=torch.int32)
        source = torch.empty((capacity,), device=device, dtype=torch.int32)
        label = torch.empty((capacity,), device=device, dtype=torch.int32)
        totals = torch.empty((2,), device=device, dtype=torch.int64)
        ws = _workspace(V, F, device) if V and F else None
        _check(_lib.tsf_split(V, F, f.data_ptr() if F else None, _native._ptr(k), corner_fan.data_ptr() if F else None, capacity,
                              out_faces.data_ptr() if F else None, source.data_ptr() if capacity else None,
                              label.data_ptr() if capacity else None, totals.data_ptr(), _native._ptr(ws),
                              ws.numel() if ws is not None else 0, _native.stream()), "split_nonmanifold")
    return out_faces, source, label, totals


def vertex_fans(num_vertices: int, faces: torch.Tensor, keep: Optional[torch.Tensor] = None) -> VertexFans:
    """The fans of an indexed mesh (module text).  stats: the six counts of tsf_fans under COUNT_NAMES and new_vertices, the number of
    vertices split_nonmanifold would add; one host read."""
    V = int(num_vertices)
    if V < 0:
        raise ValueError("num_vertices must be >= 0")
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    device = _device_of("vertex_fans", f, k)
    corner_fan, fans, counts = _fans_arrays(V, f, k, device)
    stats = dict(zip(COUNT_NAMES, (int(x) for x in counts.tolist())))
    stats["new_vertices"] = stats["fans"] - stats["fan_vertices"]
    return VertexFans(corner_fan, fans, stats)


def split_nonmanifold(vertices: torch.Tensor, faces: torch.Tensor, vertex_attributes: Optional[torch.Tensor] = None,
                      attribute_valid: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                      fans: Optional[VertexFans] = None) -> ManifoldMesh:
    """Gives every fan but the first of every vertex a vertex of its own (module text).  The input's vertices come first, bit for bit; the new
    rows of vertices, vertex_attributes (V, C) float32 and attribute_valid (V,) bool / uint8 are gathers through source_vertex.  `keep` only
    says which faces take part; all F faces are returned.  fans: vertex_fans' result for these faces and this keep, when it is at hand.
    stats: the fans' and corners_rewritten."""
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    device = _device_of("split_nonmanifold", v, f, k, vertex_attributes, attribute_valid)
    V, F = v.shape[0], f.shape[0]
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
    if fans is None:
        fans = vertex_fans(V, f, k)
    if fans.corner_fan.shape != (3 * F,) or fans.vertex_fans.shape != (V,):
        raise RuntimeError("fans were found for another mesh")
    _device_of("split_nonmanifold", f, fans.corner_fan)
    new = int(fans.stats["new_vertices"])
    out_faces, source, _, totals = _split_arrays(V, f, k, fans.corner_fan.contiguous(), new, device)
    with torch.cuda.device(device):
        src = source.to(torch.int64)
        source_vertex = torch.cat([torch.arange(V, device=device, dtype=torch.int32), source])
        out_v = torch.cat([v, v[src]])
        new_vertex = torch.zeros((V + new,), device=device, dtype=torch.bool)
        new_vertex[V:] = True
        out_a = out_valid = None
        if attrs is not None:
            out_a = torch.cat([attrs, attrs[src]])
            was = valid != 0 if valid is not None else torch.ones((V,), device=device, dtype=torch.bool)
            out_valid = torch.cat([was, was[src]])
    stats = dict(fans.stats)
    stats["corners_rewritten"] = int(totals[1].item()) if new else 0
    return ManifoldMesh(out_v, out_faces, out_a, out_valid, source_vertex, new_vertex, fans, stats)


def manifold_fused(mesh):
    """The pass behind a fusion: `mesh` is what volume.extract() / fuse_mesh / fuse_colored_mesh / simplify_fused returned (a WeldedMesh or a
    ColoredMesh); split_nonmanifold.  Returns the same kind of mesh: a ColoredMesh carries vertex_color / color_valid through as attributes
    (a copy has its source's); a WeldedMesh keeps face_keep, and vertex_map composed with the split -- the input's vertices keep their
    indices and positions, so every soup vertex still lands on a vertex with its position (the copy that kept the index) -- and faces_color
    becomes None.  stats keeps the fusion's entries, updates num_vertices / num_faces and gains split_nonmanifold's under "manifold"."""
    coloured = hasattr(mesh, "vertex_color")
    color, valid = (mesh.vertex_color, mesh.color_valid) if coloured else (None, None)
    r = split_nonmanifold(mesh.vertices, mesh.faces, vertex_attributes=color, attribute_valid=valid)
    stats = dict(mesh.stats)
    stats["manifold"] = r.stats
    stats.update(num_vertices=int(r.vertices.shape[0]), num_faces=int(r.faces.shape[0]))
    if coloured:
        return mesh._replace(vertices=r.vertices, faces=r.faces, vertex_color=r.vertex_attributes, color_valid=r.attribute_valid, stats=stats)
    # source_vertex is the identity on the input's vertices: the composed map is vertex_map itself
    return mesh._replace(vertices=r.vertices, faces=r.faces, faces_color=None, vertex_map=mesh.vertex_map, face_keep=mesh.face_keep, stats=stats)


__all__ = ["VertexFans", "ManifoldMesh", "vertex_fans", "split_nonmanifold", "manifold_fused", "COUNT_NAMES"]
