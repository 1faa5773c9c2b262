"""Ray casting on the triangle index of a mesh: the exact FIRST HIT of every ray, and what is built on it.

    ray_cast(bvh, origins, directions, tmin=0.0, tmax=inf, t_limit=None, cull_back=False) -> RayHits(face, t, bary, side)
    camera_rays(cam)                                    the pixel-centre rays of a pinhole view; their t is the view-space depth
    point_visibility(bvh, points, centres)              how many of the centres see each point past the mesh
    mesh_surface.mesh_surface_distance(..., visible_from=centres)   the surface scores over the OBSERVED samples only

`bvh` is a mesh_surface.MeshBVH (built once) or (vertices, faces[, keep]).  The query is defined so that the native result is a pure function
of its input and EQUALS brute force over all faces, ties included (include/ts_ray.h):

    triangle    the watertight test of Woop, Benthin and Wald in float64 on the fp32 coordinates: a ray never slips between two faces that
                share an edge or a vertex; an edge value of exactly 0 counts for both faces
    first hit   the eligible face (mesh_surface.py) with the smallest t' in [tmin, min(tmax, t_limit)], t' the hit distance raised to where
                the ray enters the face's bounding box; ties to the smallest face index.  t counts in units of the direction's length.
    bary, side  the weights of the face's three vertices at the hit; +1 for a hit on the front of a counter-clockwise face, -1 on its back
    no hit      face = -1, t = +inf, bary = NaN, side = 0;   a bad ray (non-finite component, zero direction, NaN limit): t = NaN

Native code: libts_ray.so beside this file (include/ts_ray.h, csrc/mesh_ray.hip), a fourth library because the export lists of the other
three are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import NamedTuple, Optional, Tuple

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_ray

from .mesh_surface import MeshBVH, _device_of, _points_arg

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_ray.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The ray-casting kernels have no CPU fallback."
    )
_lib = bind_ray(C.CDLL(_LIB_PATH))


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsr_last_error().decode()} (ts2d error {rc})")


class RayHits(NamedTuple):
    face: torch.Tensor  # (Q,) int32, -1 without a hit
    t: torch.Tensor     # (Q,) float64, +inf without a hit, NaN for a bad ray
    bary: torch.Tensor  # (Q, 3) float32: the weights of the face's vertices a, b, c
    side: torch.Tensor  # (Q,) int8: +1 front, -1 back, 0 without a hit


def _as_bvh(bvh) -> MeshBVH:
    return bvh if isinstance(bvh, MeshBVH) else MeshBVH(*bvh)


def ray_cast(bvh, origins: torch.Tensor, directions: torch.Tensor, tmin: float = 0.0, tmax: float = math.inf,
             t_limit: Optional[torch.Tensor] = None, cull_back: bool = False, leaf_visits: Optional[torch.Tensor] = None) -> RayHits:
    """The first face that every ray o + t d meets with t in [tmin, min(tmax, t_limit)] (module text).  origins, directions: (Q, 3);
    t_limit: (Q,) per-ray upper limits or None; cull_back: hits on the back of a face do not count.  `leaf_visits`: an int64 tensor of one
    element that gains the number of (wave, leaf) visits (tools/bench_mesh_distance.py)."""
    bvh = _as_bvh(bvh)
    o, d = _points_arg(origins, "origins"), _points_arg(directions, "directions")
    if o.shape != d.shape:
        raise RuntimeError("origins and directions must have the same dimensions (num_rays, 3)")
    Q = o.shape[0]
    if t_limit is not None:
        if t_limit.shape != (Q,):
            raise RuntimeError("t_limit must have dimensions (num_rays,)")
        t_limit = t_limit.detach().to(torch.float32).contiguous()
    device = _device_of("ray_cast", o, d, t_limit, bvh.bvh, leaf_visits)
    with torch.cuda.device(device):
        face = torch.empty((Q,), device=device, dtype=torch.int32)
        t = torch.empty((Q,), device=device, dtype=torch.float64)
        bary = torch.empty((Q, 3), device=device, dtype=torch.float32)
        side = torch.empty((Q,), device=device, dtype=torch.int8)
        ws = torch.empty((_lib.tsr_cast_workspace_bytes(Q),), device=device, dtype=torch.uint8)
        _check(_lib.tsr_cast(Q, _native._ptr(o), _native._ptr(d), _native._ptr(t_limit), float(tmin), float(tmax), int(bool(cull_back)),
                             bvh.num_faces, bvh.bvh.data_ptr(), bvh.bvh.numel(), _native._ptr(face), _native._ptr(t), _native._ptr(bary),
                             _native._ptr(side), _native._ptr(leaf_visits), ws.data_ptr(), ws.numel(), _native.stream()), "ray_cast")
    return RayHits(face, t, bary, side)


def camera_rays(cam) -> Tuple[torch.Tensor, torch.Tensor]:
    """(origins (H*W, 3), directions (H*W, 3)), float32, row-major over the pixels: the rays through the pixel centres (i + 0.5, j + 0.5) of
    the duck-typed camera that MeshRenderer takes (`world_view_transform` in the row-vector convention, `tan_fovx`, `tan_fovy`,
    `image_width`, `image_height`).  Every direction has unit VIEW-SPACE depth, so the t of a hit is the depth that MeshRenderer reports.
    Worked out in float64 and rounded once."""
    W, H = int(cam.image_width), int(cam.image_height)
    view = cam.world_view_transform.detach().to(torch.float64)
    back = torch.linalg.inv(view[:3, :3].cpu()).to(view.device)  # view = world @ view[:3, :3] + view[3, :3]
    centre = -(view[3, :3] @ back)
    x = ((torch.arange(W, device=view.device, dtype=torch.float64) + 0.5) / (0.5 * W) - 1.0) * float(cam.tan_fovx)
    y = ((torch.arange(H, device=view.device, dtype=torch.float64) + 0.5) / (0.5 * H) - 1.0) * float(cam.tan_fovy)
    d_view = torch.stack([x[None, :].expand(H, W), y[:, None].expand(H, W), torch.ones((H, W), device=view.device, dtype=torch.float64)], dim=-1)
    directions = (d_view.reshape(-1, 3) @ back).to(torch.float32).contiguous()
    origins = centre.to(torch.float32).expand(H * W, 3).contiguous()
    return origins, directions


def point_visibility(bvh, points: torch.Tensor, centres: torch.Tensor, rel_eps: float = 1e-5) -> torch.Tensor:
    """(Q,) int32: the number of `centres` (C, 3) that see each of `points` (Q, 3).  A centre c sees p iff the ray o = c, d = fp32(p - c)
    has no hit with t' <= 1 - rel_eps: one ray_cast per centre.  The points may lie ON the mesh: their own face sits at t about 1 and is
    excluded by the limit."""
    bvh = _as_bvh(bvh)
    p, c = _points_arg(points, "points"), _points_arg(centres, "centres")
    _device_of("point_visibility", p, c, bvh.bvh)
    seen = torch.zeros((p.shape[0],), device=p.device, dtype=torch.int32)
    for k in range(c.shape[0]):
        hits = ray_cast(bvh, c[k].expand_as(p), p - c[k], tmin=0.0, tmax=1.0 - float(rel_eps))
        seen += (hits.face < 0).to(torch.int32)
    return seen


__all__ = ["RayHits", "ray_cast", "camera_rays", "point_visibility"]
