"""Triangle overlap on the triangle index: the self-intersections of a mesh and the face pairs in which two meshes meet.

    MeshBVH.overlap(other=None, capacity=None)             MeshOverlap: the pairs of one mesh, or (face of self, face of other)
    self_intersections(mesh, capacity=None)                that for mesh = a MeshBVH or (vertices, faces[, keep])
    mesh_intersections(mesh_a, mesh_b, capacity=None)      the cross form: count_a, count_b
    intersecting_face_mask(mesh)                           (F,) bool: count > 0
    drop_intersecting_faces(mesh, vertex_attributes=None)  CleanedMesh: the mesh without those faces; the holes are fill_holes' job
    self_intersection_report(mesh)                         a dict of integers: faces, crossing_pairs, crossing_faces, coplanar_pairs, ...

The indexed-mesh chain can make a surface pass through itself: vertex clustering moves vertices of separate sheets into neighbouring
cells, a centroid fan over a non-planar loop can cut through its surroundings, Taubin smoothing moves vertices with no regard for other
pieces.  mesh_topology reports connectivity; this reports geometry.  Every pair of faces whose bounding boxes overlap is classified in
float64 (include/ts_overlap.h):

    kind 1  CROSSING   an edge of one face meets the other face (closed: a touch counts); pairs that share one vertex are tested on the
                       two opposite edges, pairs that share an edge are ADJACENT and only counted
    kind 2  COPLANAR   all vertices of one face lie in the plane of the other: a candidate, its overlap in the plane is not resolved
    kind 3  DUPLICATE  the same three vertex indices (self mode)

`count` is, per face, the number of its partners of kind 1.  The result is a pure function of the input, equal to a brute force over
all pairs bit for bit; it is not a proof about the geometry of the real numbers.

Native code: libts_overlap.so beside this file (include/ts_overlap.h, csrc/mesh_overlap.hip), a fifteenth library because the export
lists of the other fourteen are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, NamedTuple, Optional

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_overlap

from .mesh_surface import MeshBVH, _device_of

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_overlap.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The triangle-overlap kernels have no CPU fallback."
    )
_lib = bind_overlap(C.CDLL(_LIB_PATH))

KIND_CROSSING, KIND_COPLANAR, KIND_DUPLICATE = 1, 2, 3
STATS_KEYS = ("candidates", "adjacent", "crossing", "coplanar", "duplicate", "degenerate", "stored")  # stats[0..6] of include/ts_overlap.h


class MeshOverlap(NamedTuple):
    pairs: torch.Tensor              # (P, 2) int32, ascending by (first, second): (lo, hi), or (face of a, face of b)
    kind: torch.Tensor               # (P,) uint8: KIND_CROSSING, KIND_COPLANAR or KIND_DUPLICATE
    count: torch.Tensor              # (F,) int32: per face of the (first) mesh its partners of kind 1
    count_b: Optional[torch.Tensor]  # cross mode: the same for the faces of the second mesh; None in self mode
    stats: Dict[str, int]

    @property
    def count_a(self) -> torch.Tensor:
        return self.count


class CleanedMesh(NamedTuple):
    vertices: torch.Tensor                      # (V', 3): the vertices that the remaining faces name, in their order
    faces: torch.Tensor                         # (F', 3) int32
    face_keep: torch.Tensor                     # (F,) bool over the input's faces
    vertex_keep: torch.Tensor                   # (V,) bool over the input's vertices
    vertex_attributes: Optional[torch.Tensor]   # (V', ...) when given
    stats: Dict[str, int]


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsx_last_error().decode()} (ts2d error {rc})")


def _as_bvh(mesh) -> MeshBVH:
    if isinstance(mesh, MeshBVH):
        return mesh
    if hasattr(mesh, "vertices") and hasattr(mesh, "faces"):
        return MeshBVH(mesh.vertices, mesh.faces)
    return MeshBVH(*mesh)


def default_capacity(num_faces: int) -> int:
    """The list capacity of the first call: max(1024, F // 8).  A list that overflows it costs one more call."""
    return max(1024, int(num_faces) // 8)


def _bits(n: int) -> int:
    return max(1, (max(int(n), 1) - 1).bit_length())


def _query(a: MeshBVH, b: Optional[MeshBVH], capacity: int, leaf_visits: Optional[torch.Tensor]):
    device = a.device
    FA, FB = a.num_faces, (b.num_faces if b is not None else 0)
    with torch.cuda.device(device):
        count_a = torch.empty((FA,), device=device, dtype=torch.int32)
        count_b = torch.empty((FB,), device=device, dtype=torch.int32) if b is not None else None
        stats = torch.empty((8,), device=device, dtype=torch.int64)
        pairs = torch.empty((capacity, 2), device=device, dtype=torch.int32)
        kind = torch.empty((capacity,), device=device, dtype=torch.uint8)
        _check(_lib.tsx_overlap(FA, a.bvh.data_ptr() if FA else None, a.bvh.numel(), a.faces.data_ptr() if b is None and FA else None, FB,
                                b.bvh.data_ptr() if FB else None, b.bvh.numel() if b is not None else 0, _native._ptr(count_a) if FA else None,
                                _native._ptr(count_b) if FB else None, stats.data_ptr(), capacity, pairs.data_ptr() if capacity else None,
                                kind.data_ptr() if capacity else None, _native._ptr(leaf_visits), _native.stream()), "overlap")
        st = [int(x) for x in stats.tolist()]
    return count_a, count_b, st, pairs, kind


def overlap(a: MeshBVH, other: Optional[MeshBVH] = None, capacity: Optional[int] = None, leaf_visits: Optional[torch.Tensor] = None) -> MeshOverlap:
    """MeshBVH.overlap: the pairs of kind != 0 of `a` with itself (other = None) or of (face of a, face of other), sorted, the per-face
    crossing counts and the stats of include/ts_overlap.h.  capacity: the room of the first call's list, default max(1024, F // 8); when the
    list overflows it the stats say by how much and a second call with the exact total returns the complete list.  `leaf_visits`: an int64
    tensor of one element that gains the (wave, leaf) visits of every call made."""
    if not isinstance(a, MeshBVH) or (other is not None and not isinstance(other, MeshBVH)):
        raise TypeError("overlap takes MeshBVH objects")
    if other is not None:
        _device_of("MeshBVH.overlap", a.bvh, other.bvh, leaf_visits)
    else:
        _device_of("MeshBVH.overlap", a.bvh, leaf_visits)
    capacity = default_capacity(a.num_faces) if capacity is None else int(capacity)
    if capacity < 0:
        raise ValueError(f"capacity must be >= 0, not {capacity}")
    count_a, count_b, st, pairs, kind = _query(a, other, capacity, leaf_visits)
    total = st[2] + st[3] + st[4]
    if total > capacity:
        count_a, count_b, st, pairs, kind = _query(a, other, total, leaf_visits)
    P = st[6]
    pairs, kind = pairs[:P].contiguous(), kind[:P].contiguous()
    if P:
        with torch.cuda.device(a.device):
            ws = torch.empty((_lib.tsx_sort_workspace_bytes(P),), device=a.device, dtype=torch.uint8)
            _check(_lib.tsx_sort_pairs(P, _bits(a.num_faces), _bits(other.num_faces if other is not None else a.num_faces), pairs.data_ptr(),
                                       kind.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream()), "sort_pairs")
    return MeshOverlap(pairs, kind, count_a, count_b, dict(zip(STATS_KEYS, st)))


def _counts(bvh: MeshBVH):
    """(count, stats) of the self check without a list: one call, capacity 0."""
    _device_of("MeshBVH.overlap", bvh.bvh)
    count, _, st, _, _ = _query(bvh, None, 0, None)
    return count, dict(zip(STATS_KEYS, st))


def self_intersections(mesh, capacity: Optional[int] = None) -> MeshOverlap:
    """overlap of one mesh with itself; mesh = a MeshBVH, (vertices, faces[, keep]) or an object with .vertices and .faces."""
    return overlap(_as_bvh(mesh), None, capacity)


def mesh_intersections(mesh_a, mesh_b, capacity: Optional[int] = None) -> MeshOverlap:
    """overlap of the faces of mesh_a with those of mesh_b: pairs (face of a, face of b), count (= count_a) and count_b."""
    return overlap(_as_bvh(mesh_a), _as_bvh(mesh_b), capacity)


def intersecting_face_mask(mesh) -> torch.Tensor:
    """(F,) bool: the faces with at least one partner of kind 1."""
    return _counts(_as_bvh(mesh))[0] > 0


def drop_intersecting_faces(mesh, vertex_attributes: Optional[torch.Tensor] = None) -> CleanedMesh:
    """The mesh without the faces of intersecting_face_mask and without the vertices that no remaining face names, as drop_small_pieces
    leaves a mesh; vertex_attributes (V, ...) are carried along.  A face with an index outside [0, V) is dropped too.  The holes this
    leaves are fill_holes' job."""
    bvh = _as_bvh(mesh)
    v, f = bvh.vertices, bvh.faces
    V, F = v.shape[0], f.shape[0]
    if vertex_attributes is not None and vertex_attributes.shape[0] != V:
        raise RuntimeError("vertex_attributes must have one row per vertex")
    count, counted = _counts(bvh)
    with torch.cuda.device(bvh.device):
        valid = ((f >= 0) & (f < V)).all(dim=1) if F else torch.zeros((0,), device=bvh.device, dtype=torch.bool)
        keep = valid & (count == 0)
        used = torch.zeros((V,), device=bvh.device, dtype=torch.bool)
        kept = f[keep].to(torch.int64)
        used[kept.reshape(-1)] = True
        new_index = torch.cumsum(used.to(torch.int64), 0) - 1
        out_faces = new_index[kept].to(torch.int32).reshape(-1, 3).contiguous()
        out_vertices = v[used].contiguous()
        attrs = vertex_attributes[used].contiguous() if vertex_attributes is not None else None
    stats = dict(counted, dropped_faces=int(F - out_faces.shape[0]), num_vertices=int(out_vertices.shape[0]), num_faces=int(out_faces.shape[0]))
    return CleanedMesh(out_vertices, out_faces, keep, used, attrs, stats)


def self_intersection_report(mesh) -> Dict[str, int]:
    """Integers only: faces, crossing_pairs, crossing_faces (faces with count > 0), coplanar_pairs, duplicate_pairs, degenerate_faces."""
    bvh = _as_bvh(mesh)
    count, st = _counts(bvh)
    return {"faces": int(bvh.num_faces), "crossing_pairs": st["crossing"], "crossing_faces": int((count > 0).sum().item()),
            "coplanar_pairs": st["coplanar"], "duplicate_pairs": st["duplicate"], "degenerate_faces": st["degenerate"]}


__all__ = ["KIND_CROSSING", "KIND_COPLANAR", "KIND_DUPLICATE", "MeshOverlap", "CleanedMesh", "self_intersections", "mesh_intersections",
           "intersecting_face_mask", "drop_intersecting_faces", "self_intersection_report"]
