"""Vertex welding and topology of an exported triangle mesh, on the device:

    weld_mesh(vertices, faces, faces_color=None, eps=0.0, position="first")   merges all vertices within `eps` of each other, transitively,
                                                                              renumbers them, remaps the faces and drops the ones that collapse
    mesh_topology(num_vertices, faces, keep=None)                             boundary / manifold / non-manifold edges, connected pieces, Euler
    weld_labels / face_components / compact_labels / remap_faces / edge_census  the five native steps, one call each

`mesh_from_triangles` and `RawTriangle.saveGLB` give every triangle three private vertices; the trainer's `vertex_reg` pulls neighbouring
triangles' vertices together, and this module answers whether they closed up into a surface.  It is the counterpart of the reference's
saveGLB(..., process=True) (src/diff_recon/models/raw_triangle.py:183-207: trimesh's vertex merging), UNPINNED against trimesh like the rest
of the export path, and defined so that the result is a pure function of the input (include/ts_weld.h):

    adjacent   i != j, all six coordinates finite, (dx*dx + dy*dy) + dz*dz <= eps*eps in fp32 with every operation rounded
    clusters   the connected components of that relation (single linkage: chains merge; `stats["largest_cluster"]` and
               `stats["max_displacement"]` show when that happened); label = the smallest index of the cluster
    numbering  clusters ranked by ascending label; vertices that no face names are kept
    position   "first": the position of vertex `label`, bit for bit; "mean": float64 sum in ascending index order / count, rounded to fp32
    faces      a face is dropped iff an index lies outside [0, V) or two of its new indices are equal; kept faces stay in their order.
               Duplicate faces are NOT removed.

Native code: libts2d.so (include/ts_weld.h, csrc/mesh_weld.hip), bound with ctypes like mesh_renderer.py.  No CPU / eager fallback.  The search
is quadratic when most vertices lie within `eps` of each other (see the header): `eps` is meant to be far below the mesh's extent."""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional

import torch

from diff_triangle_rasterization_2D import _C as _native

_lib = _native._lib

POSITION_MODES = {"first": 0, "mean": 1}  # TS2D_WELD_FIRST / TS2D_WELD_MEAN


class WeldedMesh(NamedTuple):
    vertices: torch.Tensor               # (V', 3) float32
    faces: torch.Tensor                  # (F', 3) int32: the kept faces, in their original order
    faces_color: Optional[torch.Tensor]  # (F', 3): the kept faces' rows of the input colours, or None
    vertex_map: torch.Tensor             # (V,) int32: old vertex -> new vertex (`remap`)
    face_keep: torch.Tensor              # (F,) bool
    stats: Dict[str, object]


def _device_of(what: str, *tensors) -> torch.device:
    tensors = [t for t in tensors if t is not None]
    device = tensors[0].device
    if device.type != "cuda" or any(t.device != device for t in tensors):
        raise RuntimeError(f"{what} (MI355X build) needs its tensors on one HIP device; there is no CPU fallback")
    return device


def _vertices_arg(vertices: torch.Tensor) -> torch.Tensor:
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError("vertices must have dimensions (num_vertices, 3)")
    return vertices.detach().to(torch.float32).contiguous()


def _faces_arg(faces: torch.Tensor) -> torch.Tensor:
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("faces must be an int32 or int64 tensor with dimensions (num_faces, 3)")
    if faces.dtype == torch.int64:  # an index beyond int32 names no vertex either way: -1 is out of range for every V
        faces = torch.where((faces >= 0) & (faces < 2 ** 31), faces, torch.full_like(faces, -1))
    return faces.to(torch.int32).contiguous()


def _keep_arg(keep: Optional[torch.Tensor], F: int) -> Optional[torch.Tensor]:
    if keep is None:
        return None
    if keep.shape != (F,) or keep.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError("keep must be a bool or uint8 tensor with dimensions (num_faces,)")
    return keep.contiguous()


def _workspace(V: int, F: int, device) -> torch.Tensor:
    return torch.empty((_lib.ts2d_weld_workspace_bytes(V, F),), device=device, dtype=torch.uint8)


def _check_eps(eps: float) -> float:
    eps = float(eps)
    if not (math.isfinite(eps) and eps >= 0.0):
        raise ValueError("eps must be finite and >= 0")
    return eps


def weld_labels(vertices: torch.Tensor, eps: float, box_visits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(V,) int32: the smallest index of every vertex's cluster.  `box_visits`: an int64 tensor of one element that gains the number of
    (workgroup, box) visits of the search (tools/bench_mesh_weld.py)."""
    eps = _check_eps(eps)
    v = _vertices_arg(vertices)
    device = _device_of("weld_labels", v, box_visits)
    V = v.shape[0]
    with torch.cuda.device(device):
        label = torch.empty((V,), device=device, dtype=torch.int32)
        if V:
            ws = _workspace(V, 0, device)
            _native._check(_lib.ts2d_weld_labels_counted(V, v.data_ptr(), eps, label.data_ptr(), _native._ptr(box_visits), ws.data_ptr(), ws.numel(),
                                                         _native.stream()), "weld_labels")
    return label


def face_components(num_vertices: int, faces: torch.Tensor, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(V,) int32: the smallest vertex index every vertex is joined to along the edges of the kept faces."""
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    device = _device_of("face_components", f, k)
    V, F = int(num_vertices), f.shape[0]
    if V < 0:
        raise ValueError("num_vertices must be >= 0")
    with torch.cuda.device(device):
        label = torch.empty((V,), device=device, dtype=torch.int32)
        if V:
            _native._check(_lib.ts2d_weld_face_components(V, F, _native._ptr(f) if F else None, _native._ptr(k), label.data_ptr(), None, 0, _native.stream()),
                           "face_components")
    return label


def compact_labels(label: torch.Tensor, vertices: torch.Tensor, position: str = "first"):
    """(remap (V,) int32, welded vertices (V', 3) float32, V') from cluster labels.  Reads V' back: the one host synchronisation of a weld."""
    if position not in POSITION_MODES:
        raise ValueError(f"position must be one of {sorted(POSITION_MODES)}, not {position!r}")
    v = _vertices_arg(vertices)
    device = _device_of("compact_labels", v, label)
    V = v.shape[0]
    if label.shape != (V,) or label.dtype != torch.int32:
        raise RuntimeError("label must be an int32 tensor with dimensions (num_vertices,)")
    with torch.cuda.device(device):
        label = label.contiguous()
        remap = torch.empty((V,), device=device, dtype=torch.int32)
        out = torch.empty((V, 3), device=device, dtype=torch.float32)
        count = torch.zeros((1,), device=device, dtype=torch.int32)
        if V:
            ws = _workspace(V, 0, device)
            _native._check(_lib.ts2d_weld_compact(V, label.data_ptr(), v.data_ptr(), POSITION_MODES[position], remap.data_ptr(), out.data_ptr(),
                                                  count.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream()), "compact_labels")
        n = int(count.item())
    return remap, out[:n].contiguous(), n


def remap_faces(num_vertices: int, faces: torch.Tensor, remap: torch.Tensor):
    """(new faces (F, 3) int32, keep (F,) bool): every face through `remap`; a face with an index outside [0, V) becomes -1 -1 -1 and is not
    kept, nor is one with two equal new indices."""
    f = _faces_arg(faces)
    device = _device_of("remap_faces", f, remap)
    V, F = int(num_vertices), f.shape[0]
    if remap.shape != (V,) or remap.dtype != torch.int32:
        raise RuntimeError("remap must be an int32 tensor with dimensions (num_vertices,)")
    with torch.cuda.device(device):
        remap = remap.contiguous()
        out = torch.empty((F, 3), device=device, dtype=torch.int32)
        keep = torch.zeros((F,), device=device, dtype=torch.bool)
        if F:
            _native._check(_lib.ts2d_weld_remap_faces(V, F, f.data_ptr(), _native._ptr(remap) if V else None, out.data_ptr(), keep.data_ptr(),
                                                      _native.stream()), "remap_faces")
    return out, keep


def edge_census(num_vertices: int, faces: torch.Tensor, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(4,) int64 on the device: {edges, boundary, manifold, nonmanifold} of the kept faces' undirected edges."""
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    device = _device_of("edge_census", f, k)
    V, F = int(num_vertices), f.shape[0]
    if V < 0:
        raise ValueError("num_vertices must be >= 0")
    with torch.cuda.device(device):
        counts = torch.zeros((4,), device=device, dtype=torch.int64)
        if F:
            ws = _workspace(V, F, device)
            _native._check(_lib.ts2d_weld_edge_census(V, F, f.data_ptr(), _native._ptr(k), counts.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream()),
                           "edge_census")
    return counts


def weld_mesh(vertices: torch.Tensor, faces: torch.Tensor, faces_color: Optional[torch.Tensor] = None, eps: float = 0.0,
              position: str = "first") -> WeldedMesh:
    """Welds an indexed mesh (module text).  `faces_color` (F, 3), when given, is cut down to the kept faces.  stats: num_vertices_in,
    num_vertices, num_faces_in, num_faces, largest_cluster (members of the largest cluster) and max_displacement (the largest distance
    between a vertex and its welded position, over the finite vertices; float)."""
    if position not in POSITION_MODES:
        raise ValueError(f"position must be one of {sorted(POSITION_MODES)}, not {position!r}")
    eps = _check_eps(eps)
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    device = _device_of("weld_mesh", v, f, faces_color)
    V, F = v.shape[0], f.shape[0]
    if faces_color is not None and (faces_color.dim() != 2 or faces_color.shape[0] != F):
        raise RuntimeError("faces_color must have dimensions (num_faces, C)")
    with torch.cuda.device(device):
        label = weld_labels(v, eps)
        remap, welded, n = compact_labels(label, v, position)
        new_faces, keep = remap_faces(V, f, remap)
        largest, displacement = 0, 0.0
        if V:
            largest = int(torch.bincount(remap.to(torch.int64), minlength=n).max().item())
            d = (v.to(torch.float64) - welded[remap.to(torch.int64)].to(torch.float64)).norm(dim=1)
            d = d[torch.isfinite(d)]
            displacement = float(d.max().item()) if d.numel() else 0.0
        kept = new_faces[keep].contiguous()
        color = faces_color[keep].contiguous() if faces_color is not None else None
    stats = {"num_vertices_in": V, "num_vertices": n, "num_faces_in": F, "num_faces": int(kept.shape[0]), "largest_cluster": largest,
             "max_displacement": displacement}
    return WeldedMesh(welded, kept, color, remap, keep, stats)


def mesh_topology(num_vertices: int, faces: torch.Tensor, keep: Optional[torch.Tensor] = None) -> Dict[str, int]:
    """Integers of a face list on `num_vertices` vertices (kept faces with their indices in range only): `edges` distinct undirected edges, of
    which `boundary` are used by exactly one face, `manifold` by exactly two, `nonmanifold` by three or more; `pieces` connected components
    of the vertices that those faces name, joined along face edges; `vertices_referenced`, `faces`; `euler` = V_ref - edges + F_kept.
    Pass FRONT faces only: reversed twins double every edge."""
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    V = int(num_vertices)
    counts = edge_census(V, f, k)
    label = face_components(V, f, k)
    valid = ((f >= 0) & (f < V)).all(dim=1)
    if k is not None:
        valid &= k.to(torch.bool)
    used = f[valid].to(torch.int64).reshape(-1)
    referenced = torch.zeros((V,), device=f.device, dtype=torch.bool)
    referenced[used] = True
    pieces = int((referenced & (label == torch.arange(V, device=f.device, dtype=torch.int32))).sum().item())
    v_ref, f_kept = int(referenced.sum().item()), int(valid.sum().item())
    edges, boundary, manifold, nonmanifold = (int(x) for x in counts.tolist())
    return {"edges": edges, "boundary": boundary, "manifold": manifold, "nonmanifold": nonmanifold, "pieces": pieces,
            "vertices_referenced": v_ref, "faces": f_kept, "euler": v_ref - edges + f_kept}


__all__ = ["WeldedMesh", "weld_mesh", "mesh_topology", "weld_labels", "face_components", "compact_labels", "remap_faces", "edge_census"]
