"""Exact point-to-SURFACE distance on the device: a bounding-volume hierarchy over the triangles of a mesh, and the scores built on it.

    MeshBVH(vertices, faces, keep=None)                 the index of a mesh, built once; .closest(queries) -> (face, dist2, point);
                                                        .ray_cast(origins, directions) -> the first hit of every ray (mesh_ray.py);
                                                        .ray_crossings(origins, directions) -> all hits, counted (mesh_inside.py);
                                                        .winding_number(points) -> the generalised winding number (mesh_winding.py);
                                                        .overlap(other=None) -> the face pairs that intersect (mesh_overlap.py)
    point_to_mesh_distance(points, (vertices, faces))   the same in one call
    mesh_surface_distance((va, fa), (vb, fb), samples, seed=0, thresholds=(), visible_from=None)
                                                        accuracy / completeness / Chamfer / Hausdorff / precision / recall / F-score, sample to surface;
                                                        with visible_from = (C, 3) centres over the samples that some centre sees (mesh_ray.py)

mesh_distance.mesh_distance measures point to POINT: both surfaces are sampled and two identical surfaces score about half the sample
spacing.  Here the samples of one mesh are measured against the triangles of the other, so identical surfaces score 0 (up to the fp32
rounding of the sampler's points) and a tight threshold means something.  The query is defined so that the native results are pure functions
of their input (include/ts_bvh.h):

    distance    D'(q, T) in float64: the minimum over the three edges (clamped projection) and the interior (plane distance when the three
                side tests pass), raised to the distance to the face's bounding box, every operation rounded
    closest     the eligible face (kept, indices in range, finite coordinates; zero-area faces included) with the smallest D', ties to the
                smallest face index; face = -1, dist2 = +inf, point = NaN when no face is eligible; face = -1, dist2 = NaN, point = NaN for a
                query with a non-finite coordinate
    scores      in float64 from sqrt(dist2) over the samples that found a face (the others are counted in a_dropped / b_dropped)

Native code: libts_bvh.so beside this file (include/ts_bvh.h, csrc/mesh_bvh.hip), a third library because the export lists of libts2d.so and
libts_geom.so are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence, Tuple

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_bvh

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_bvh.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The mesh-surface kernels have no CPU fallback."
    )
_lib = bind_bvh(C.CDLL(_LIB_PATH))


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsb_last_error().decode()} (ts2d error {rc})")


def _device_of(what: str, *tensors) -> torch.device:
    tensors = [t for t in tensors if t is not None]
    device = tensors[0].device
    if device.type != "cuda" or any(t.device != device for t in tensors):
        raise RuntimeError(f"{what} (MI355X build) needs its tensors on one HIP device; there is no CPU fallback")
    return device


def _points_arg(points: torch.Tensor, name: str) -> torch.Tensor:
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f"{name} must have dimensions (num_points, 3)")
    return points.detach().to(torch.float32).contiguous()


def _faces_arg(faces: torch.Tensor) -> torch.Tensor:
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("faces must be an int32 or int64 tensor with dimensions (num_faces, 3)")
    if faces.dtype == torch.int64:  # an index beyond int32 names no vertex either way: -1 is out of range for every V
        faces = torch.where((faces >= 0) & (faces < 2 ** 31), faces, torch.full_like(faces, -1))
    return faces.to(torch.int32).contiguous()


class MeshBVH:
    """The triangle index of one mesh on its device: vertices (V, 3) floating, faces (F, 3) int32 / int64, keep (F,) bool / uint8 or None.
    Built once (a sort of the faces and one pass per tree level); holds the index and the two arrays it was built from."""

    def __init__(self, vertices: torch.Tensor, faces: torch.Tensor, keep: Optional[torch.Tensor] = None):
        v, f = _points_arg(vertices, "vertices"), _faces_arg(faces)
        F = f.shape[0]
        if keep is not None:
            if keep.shape != (F,) or keep.dtype not in (torch.bool, torch.uint8):
                raise RuntimeError("keep must be a bool or uint8 tensor with dimensions (num_faces,)")
            keep = keep.contiguous()
        self.device = _device_of("MeshBVH", v, f, keep)
        self.vertices, self.faces = v, f
        with torch.cuda.device(self.device):
            self.bvh = torch.empty((_lib.tsb_bvh_bytes(F),), device=self.device, dtype=torch.uint8)
            if F:
                ws = torch.empty((_lib.tsb_build_workspace_bytes(F),), device=self.device, dtype=torch.uint8)
                _check(_lib.tsb_build(v.shape[0], F, _native._ptr(v), f.data_ptr(), _native._ptr(keep), self.bvh.data_ptr(), self.bvh.numel(),
                                      ws.data_ptr(), ws.numel(), _native.stream()), "MeshBVH")

    @property
    def num_faces(self) -> int:
        return self.faces.shape[0]

    def closest(self, queries: torch.Tensor, leaf_visits: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(face (Q,) int32, dist2 (Q,) float64, point (Q, 3) float32): for every query the nearest face of the mesh, the squared distance to
        it and the closest point on it (module text).  `leaf_visits`: an int64 tensor of one element that gains the number of (wave, leaf)
        visits (tools/bench_mesh_distance.py)."""
        q = _points_arg(queries, "queries")
        device = _device_of("MeshBVH.closest", q, self.bvh, leaf_visits)
        Q, V, F = q.shape[0], self.vertices.shape[0], self.faces.shape[0]
        with torch.cuda.device(device):
            face = torch.empty((Q,), device=device, dtype=torch.int32)
            dist2 = torch.empty((Q,), device=device, dtype=torch.float64)
            point = torch.empty((Q, 3), device=device, dtype=torch.float32)
            if Q:
                ws = torch.empty((_lib.tsb_closest_workspace_bytes(Q),), device=device, dtype=torch.uint8)
                _check(_lib.tsb_closest(Q, q.data_ptr(), V, F, _native._ptr(self.vertices), _native._ptr(self.faces), self.bvh.data_ptr(),
                                        self.bvh.numel(), face.data_ptr(), dist2.data_ptr(), point.data_ptr(), _native._ptr(leaf_visits),
                                        ws.data_ptr(), ws.numel(), _native.stream()), "MeshBVH.closest")
        return face, dist2, point

    def ray_cast(self, origins: torch.Tensor, directions: torch.Tensor, **kwargs):
        """mesh_ray.ray_cast(self, origins, directions, ...): the first hit of every ray.  The module and its library (libts_ray.so) are
        loaded here, on the first call: `closest` needs neither."""
        from .mesh_ray import ray_cast
        return ray_cast(self, origins, directions, **kwargs)

    def ray_crossings(self, origins: torch.Tensor, directions: torch.Tensor, **kwargs):
        """mesh_inside.ray_crossings(self, origins, directions, ...): all hits of every ray, counted in half crossings.  The module and its
        library (libts_inside.so) are loaded here, on the first call."""
        from .mesh_inside import ray_crossings
        return ray_crossings(self, origins, directions, **kwargs)

    def winding_number(self, points: torch.Tensor, **kwargs):
        """mesh_winding.generalized_winding_number(points, self, ...): the generalised winding number of the mesh at every point, open
        meshes included.  The module and its library (libts_winding.so) are loaded here, on the first call; the node moments are built
        then and kept on this object."""
        from .mesh_winding import generalized_winding_number
        return generalized_winding_number(points, self, **kwargs)

    def overlap(self, other: Optional["MeshBVH"] = None, capacity: Optional[int] = None, leaf_visits: Optional[torch.Tensor] = None):
        """mesh_overlap.overlap(self, other, capacity): the face pairs of this mesh that cross, lie in one plane or are duplicates of each
        other (other = None), or the pairs (face of this mesh, face of `other`) that do.  The module and its library (libts_overlap.so) are
        loaded here, on the first call."""
        from .mesh_overlap import overlap
        return overlap(self, other, capacity, leaf_visits)


def point_to_mesh_distance(points: torch.Tensor, mesh) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """MeshBVH(*mesh).closest(points) for mesh = (vertices, faces) or (vertices, faces, keep); a MeshBVH is taken as it is."""
    bvh = mesh if isinstance(mesh, MeshBVH) else MeshBVH(*mesh)
    return bvh.closest(points)


def _one_way(dist2: torch.Tensor, face: torch.Tensor):
    found = face >= 0
    d2 = dist2[found]
    return d2, d2.sqrt(), int(face.numel() - d2.numel())


def _mean(x: torch.Tensor) -> float:
    return float(x.sum().item()) / x.numel() if x.numel() else float("nan")


def mesh_surface_distance(mesh_a, mesh_b, samples: int, seed: int = 0, thresholds: Sequence[float] = (),
                          visible_from: Optional[torch.Tensor] = None) -> Dict[str, object]:
    """Scores between the candidate mesh_a = (vertices, faces) and the ground truth mesh_b: `samples` surface points of a, drawn with `seed`,
    against the SURFACE of b, and as many of b, drawn with `seed + 1`, against the surface of a.  The keys are mesh_distance's:

        accuracy       mean distance from a sample of a to the surface of b              completeness   the same from b to a
        chamfer        (accuracy + completeness) / 2                                     chamfer_sq     the sum of the two mean SQUARED distances
        hausdorff      the largest of all those distances (of the samples: a lower bound of the surfaces')
        a_count / b_count, a_dropped / b_dropped, thresholds, precision, recall, fscore, a_within, b_within, area_a, area_b

    visible_from: a (C, 3) tensor of viewing centres (the camera centres of the captured views).  The samples of each mesh are then restricted,
    before they are scored, to those that at least one centre sees past their OWN mesh (mesh_ray.point_visibility): the faces buried inside a
    triangle soup stop counting in accuracy and precision.  a_hidden / b_hidden count the samples left out, a_count / b_count what remains.
    With None the result is what it was without the parameter, bit for bit, and has no such keys.

    Pass FRONT faces only, as for mesh_distance."""
    from .mesh_distance import sample_mesh_surface
    (va, fa), (vb, fb) = mesh_a, mesh_b
    sa = sample_mesh_surface(va, fa, samples, seed)
    sb = sample_mesh_surface(vb, fb, samples, int(seed) + 1)
    bvh_a, bvh_b = MeshBVH(va, fa), MeshBVH(vb, fb)
    pa, pb = sa.points, sb.points
    hidden = None
    if visible_from is not None:
        from .mesh_ray import point_visibility
        seen_a, seen_b = point_visibility(bvh_a, pa, visible_from) > 0, point_visibility(bvh_b, pb, visible_from) > 0
        hidden = (int((~seen_a).sum().item()), int((~seen_b).sum().item()))
        pa, pb = pa[seen_a], pb[seen_b]
    face_ab, d2_ab, _ = bvh_b.closest(pa)
    face_ba, d2_ba, _ = bvh_a.closest(pb)
    sq_a, da, a_dropped = _one_way(d2_ab, face_ab)
    sq_b, db, b_dropped = _one_way(d2_ba, face_ba)
    accuracy, completeness = _mean(da), _mean(db)
    res = {"accuracy": accuracy, "completeness": completeness, "chamfer": (accuracy + completeness) / 2, "chamfer_sq": _mean(sq_a) + _mean(sq_b),
           "hausdorff": max([float(d.max().item()) for d in (da, db) if d.numel()], default=float("nan")),
           "a_count": int(da.numel()), "b_count": int(db.numel()), "a_dropped": a_dropped, "b_dropped": b_dropped,
           "thresholds": [float(t) for t in thresholds], "precision": [], "recall": [], "fscore": [], "a_within": [], "b_within": [],
           "area_a": sa.area, "area_b": sb.area}
    if hidden is not None:
        res["a_hidden"], res["b_hidden"] = hidden
    for tau in res["thresholds"]:
        na, nb = int((da <= tau).sum().item()), int((db <= tau).sum().item())
        p = na / da.numel() if da.numel() else 0.0
        r = nb / db.numel() if db.numel() else 0.0
        res["a_within"].append(na)
        res["b_within"].append(nb)
        res["precision"].append(p)
        res["recall"].append(r)
        res["fscore"].append(2 * p * r / (p + r) if p + r > 0 else 0.0)
    return res


__all__ = ["MeshBVH", "point_to_mesh_distance", "mesh_surface_distance"]
