"""Geometric scores of an exported mesh, on the device: how far one surface is from another.

    nearest_points(queries, refs)                                  exact nearest neighbour of every query among ANOTHER point set
    sample_mesh_surface(vertices, faces, n, seed=0, keep=None)     n area-weighted surface points, deterministic
    point_cloud_distance(a, b, thresholds=())                      accuracy / completeness / Chamfer / Hausdorff / precision / recall / F-score
    mesh_distance((va, fa), (vb, fb), samples, seed=0, thresholds=())   the same between two sampled meshes

The image-space scores (metrics.evaluate_mesh) say how a mesh LOOKS; these say where it IS.  No counterpart in the reference beyond the
nearest search itself, which stands in for scipy.spatial.KDTree in RawTriangle's set difference (src/diff_recon/models/raw_triangle.py:79-87).
Everything is defined so that the native results are pure functions of their input (include/ts_geom.h):

    distance    d(q, r) = (dx*dx + dy*dy) + dz*dz in fp32 with every operation rounded
    nearest     the ref with finite coordinates and the smallest d, ties to the smallest ref index; idx = -1, dist2 = +inf when no ref is
                eligible; idx = -1, dist2 = NaN for a query with a non-finite coordinate
    sampling    integer weights floor(area / max area * 2^32), stratified positions from splitmix64 counters, 24-bit barycentrics: the same
                (mesh, n, seed) gives the same bits on every run; `face` is non-decreasing
    scores      in float64 from sqrt(float64(dist2)) over the points that found a neighbour (the others are counted in a_dropped / b_dropped)

Native code: libts_geom.so beside this file (include/ts_geom.h, csrc/mesh_distance.hip), a second library because libts2d.so's export list is
closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError.  The search is quadratic for queries that lie far from
ALL refs (see the header): it is built for surfaces that are near each other."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_geom

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_geom.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The mesh-distance kernels have no CPU fallback."
    )
_lib = bind_geom(C.CDLL(_LIB_PATH))

_MASK64 = 0xFFFFFFFFFFFFFFFF


class SurfaceSamples(NamedTuple):
    points: torch.Tensor  # (n, 3) float32
    face: torch.Tensor    # (n,) int32: the face every point lies in, non-decreasing
    area: float           # the float64 sum of the (kept, valid) faces' areas


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsg_last_error().decode()} (ts2d error {rc})")


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


def nearest_points(queries: torch.Tensor, refs: torch.Tensor, box_visits: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(idx (Q,) int32, dist2 (Q,) float32): for every query the index of its nearest ref and the squared distance (module text).
    `box_visits`: an int64 tensor of one element that gains the number of (workgroup, ref box) visits (tools/bench_mesh_distance.py)."""
    q, r = _points_arg(queries, "queries"), _points_arg(refs, "refs")
    device = _device_of("nearest_points", q, r, box_visits)
    Q, R = q.shape[0], r.shape[0]
    with torch.cuda.device(device):
        idx = torch.empty((Q,), device=device, dtype=torch.int32)
        dist2 = torch.empty((Q,), device=device, dtype=torch.float32)
        if Q:
            ws = torch.empty((_lib.tsg_cross_workspace_bytes(Q, R),), device=device, dtype=torch.uint8)
            _check(_lib.tsg_nearest_cross(Q, q.data_ptr(), R, _native._ptr(r), idx.data_ptr(), dist2.data_ptr(), _native._ptr(box_visits),
                                          ws.data_ptr(), ws.numel(), _native.stream()), "nearest_points")
    return idx, dist2


def face_areas(vertices: torch.Tensor, faces: torch.Tensor, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(F,) float64: the area of every face, 0 for a face that `keep` drops, that names a vertex outside [0, V) or that has a non-finite
    coordinate."""
    v, f = _points_arg(vertices, "vertices"), _faces_arg(faces)
    F = f.shape[0]
    if keep is not None:
        if keep.shape != (F,) or keep.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError("keep must be a bool or uint8 tensor with dimensions (num_faces,)")
        keep = keep.contiguous()
    device = _device_of("face_areas", v, f, keep)
    with torch.cuda.device(device):
        area = torch.empty((F,), device=device, dtype=torch.float64)
        if F:
            _check(_lib.tsg_face_areas(v.shape[0], F, _native._ptr(v), f.data_ptr(), _native._ptr(keep), area.data_ptr(), _native.stream()),
                   "face_areas")
    return area


def sample_mesh_surface(vertices: torch.Tensor, faces: torch.Tensor, n: int, seed: int = 0, keep: Optional[torch.Tensor] = None) -> SurfaceSamples:
    """`n` points on the surface of the (kept, valid) faces, every face drawn in proportion to its area (module text): stratified, so a face
    of weight w receives within 2 of n w / W points.  `seed`: any integer, taken mod 2^64.  Raises ValueError when the total area is 0
    (one blocking read)."""
    n = int(n)
    if n < 0:
        raise ValueError("n must be >= 0")
    v, f = _points_arg(vertices, "vertices"), _faces_arg(faces)
    area = face_areas(v, f, keep)
    device = area.device
    V, F = v.shape[0], f.shape[0]
    with torch.cuda.device(device):
        total = float(area.sum().item()) if F else 0.0
        if not total > 0.0:
            raise ValueError("the mesh has no surface to sample: the total area of its kept, valid faces is 0")
        points = torch.empty((n, 3), device=device, dtype=torch.float32)
        face = torch.empty((n,), device=device, dtype=torch.int32)
        if n:
            ws = torch.empty((_lib.tsg_sample_workspace_bytes(F),), device=device, dtype=torch.uint8)
            _check(_lib.tsg_sample_surface(V, F, _native._ptr(v), f.data_ptr(), area.data_ptr(), n, int(seed) & _MASK64, points.data_ptr(),
                                           face.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream()), "sample_mesh_surface")
    return SurfaceSamples(points, face, total)


def _one_way(dist2: torch.Tensor, idx: torch.Tensor):
    found = idx >= 0
    d2 = dist2[found].to(torch.float64)
    return d2, d2.sqrt(), int(idx.numel() - d2.numel())


def _mean(x: torch.Tensor) -> float:
    return float(x.sum().item()) / x.numel() if x.numel() else float("nan")


def point_cloud_distance(a: torch.Tensor, b: torch.Tensor, thresholds: Sequence[float] = ()) -> Dict[str, object]:
    """Scores between two point clouds `a` (the candidate) and `b` (the ground truth), (n, 3) each, in float64 over the points that found
    a neighbour:

        accuracy       mean distance from a point of a to its nearest point of b          completeness   the same from b to a
        chamfer        (accuracy + completeness) / 2                                      chamfer_sq     the sum of the two mean SQUARED distances
        hausdorff      the largest of all those distances
        a_count / b_count      points that found a neighbour                              a_dropped / b_dropped   points that did not
        thresholds     the list given;  precision[k] = the share of a within thresholds[k] of b (dist <= tau), recall[k] the share of b within
                       it of a, fscore[k] = 2 P R / (P + R), 0 when P + R == 0;  a_within[k] / b_within[k] the exact integer counts behind them."""
    a, b = _points_arg(a, "a"), _points_arg(b, "b")
    _device_of("point_cloud_distance", a, b)
    idx_ab, d2_ab = nearest_points(a, b)
    idx_ba, d2_ba = nearest_points(b, a)
    sq_a, da, a_dropped = _one_way(d2_ab, idx_ab)
    sq_b, db, b_dropped = _one_way(d2_ba, idx_ba)
    accuracy, completeness = _mean(da), _mean(db)
    res = {"accuracy": accuracy, "completeness": completeness, "chamfer": (accuracy + completeness) / 2, "chamfer_sq": _mean(sq_a) + _mean(sq_b),
           "hausdorff": max([float(d.max().item()) for d in (da, db) if d.numel()], default=float("nan")),
           "a_count": int(da.numel()), "b_count": int(db.numel()), "a_dropped": a_dropped, "b_dropped": b_dropped,
           "thresholds": [float(t) for t in thresholds], "precision": [], "recall": [], "fscore": [], "a_within": [], "b_within": []}
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


def mesh_distance(mesh_a, mesh_b, samples: int, seed: int = 0, thresholds: Sequence[float] = ()) -> Dict[str, object]:
    """point_cloud_distance between `samples` surface points of mesh_a = (vertices, faces), drawn with `seed`, and as many of mesh_b, drawn
    with `seed + 1`; the result also holds `area_a` and `area_b`.  The distances are point to POINT, so they carry the sampling spacing:
    two identical surfaces score about half the mean spacing of the samples, not 0.
    Pass FRONT faces only: the reversed twins that saveGLB(save_back=True) writes would double every area and halve the sampling density."""
    (va, fa), (vb, fb) = mesh_a, mesh_b
    sa = sample_mesh_surface(va, fa, samples, seed)
    sb = sample_mesh_surface(vb, fb, samples, int(seed) + 1)
    res = point_cloud_distance(sa.points, sb.points, thresholds)
    res["area_a"], res["area_b"] = sa.area, sb.area
    return res


__all__ = ["SurfaceSamples", "nearest_points", "face_areas", "sample_mesh_surface", "point_cloud_distance", "mesh_distance"]
