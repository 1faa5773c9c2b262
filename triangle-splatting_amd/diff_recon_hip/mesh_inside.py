"""Inside test and signed distance of a mesh: ALL hits of a ray on the triangle index, counted in half crossings, and what is built on it.

    ray_crossings(bvh, origins, directions, tmin=0.0, tmax=inf, t_limit=None) -> RayCrossings(hits, winding2, touches)
    winding_number(points, mesh)                        (w int32, decided bool): how often the surface winds around each point
    contains_points(points, mesh, rule="nonzero")       (inside bool, decided bool)
    signed_distance(points, mesh, rule="nonzero")       (sdf float32, face int32, decided bool): negative inside
    mesh_to_sdf(mesh, origin, voxel_size, dims, trunc=None, rule="nonzero")   the signed distance on a grid, (nz, ny, nx) float32
    remesh(mesh, resolution, offset=0.0, pad_voxels=2)  the level set of that grid: one uniform closed surface, or an offset surface
    mesh_volume_iou(mesh_a, mesh_b, resolution)         the volumetric IoU of two meshes on one grid, in integer counts

`bvh` / `mesh` is a mesh_surface.MeshBVH (built once) or (vertices, faces[, keep]).  The counts are pure functions of their input and EQUAL
brute force over all faces (include/ts_inside.h):

    hit         a face is hit exactly when ray_cast's test (mesh_ray.py, include/ts_ray.h) says so, culling off; every hit counts
    winding2    HALF crossings: 2 s for a hit in the face's interior, s for a hit through one of its edges (s = +1 on the front, -1 on the
                back).  The two faces of a shared edge see the edge value 0 together, so a crossing through an edge sums to one crossing,
                a grazed fold to none, and a boundary edge leaves winding2 odd
    touches     hits through a vertex of the face: no weight is right there, the ray is not CLEAN and another direction is cast
    clean       hits >= 0 (not a bad ray), touches == 0 and winding2 even;  w = -winding2 / 2: +1 inside an outward-facing closed mesh
    rule        "nonzero": w != 0;  "odd": w odd;  "positive": w > 0

Every function below casts along INSIDE_DIRECTIONS in order, t in [0, inf), and takes for each point the FIRST direction whose ray is
clean; a point without one is undecided.  Pass meshes whose faces wind consistently (mesh_orient.orient_faces) when the sign matters.

All of this needs a CLOSED mesh: behind an open sheet a ray crosses the surface once.  contains_points, signed_distance and mesh_volume_iou
take method="winding" (and beta) and then decide by the generalised winding number of mesh_winding.py, which degrades smoothly at a hole;
mesh_to_sdf and remesh have mesh_winding.mesh_to_sdf_winding and remesh_winding beside them.  The default, method="rays", is this module.

Native code: libts_inside.so beside this file (include/ts_inside.h, csrc/mesh_inside.hip), a thirteenth library because the export lists of
the other twelve are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_inside

from .mesh_surface import MeshBVH, _device_of, _points_arg

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_inside.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The inside-test kernels have no CPU fallback."
    )
_lib = bind_inside(C.CDLL(_LIB_PATH))

# include/ts_inside.h: fp32, in this order
INSIDE_DIRECTIONS = ((0.7548777, 0.5698403, 0.3247180), (-0.4301597, 0.6823278, -0.5905000), (0.2360680, -0.4142136, 0.8793852))
RULES = {"nonzero": 0, "odd": 1, "positive": 2}


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsi_last_error().decode()} (ts2d error {rc})")


class RayCrossings(NamedTuple):
    hits: torch.Tensor      # (Q,) int32: the number of faces hit, -1 for a bad ray
    winding2: torch.Tensor  # (Q,) int32: half crossings, fronts positive
    touches: torch.Tensor   # (Q,) int32: hits through a vertex of the face


def _as_bvh(bvh) -> MeshBVH:
    return bvh if isinstance(bvh, MeshBVH) else MeshBVH(*bvh)


METHODS = ("rays", "winding")


def _method(method: str, rule: str = "nonzero") -> bool:
    """True for method = "winding" (mesh_winding.py: the generalised winding number decides every finite point and nothing is retried),
    False for "rays" (the crossing counts of this module).  The winding number knows one rule, w >= 1/2."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {list(METHODS)}, not {method!r}")
    if method == "winding" and rule != "nonzero":
        raise ValueError(f'method="winding" decides by w >= 1/2 and takes no rule, got rule={rule!r}')
    return method == "winding"


def _rule(rule: str) -> int:
    if rule not in RULES:
        raise ValueError(f"rule must be one of {sorted(RULES)}, not {rule!r}")
    return RULES[rule]


def ray_crossings(bvh, origins: torch.Tensor, directions: torch.Tensor, tmin: float = 0.0, tmax: float = math.inf,
                  t_limit: Optional[torch.Tensor] = None, leaf_visits: Optional[torch.Tensor] = None) -> RayCrossings:
    """All faces that every ray o + t d meets with t in [tmin, min(tmax, t_limit)], counted (module text).  origins: (Q, 3); directions:
    (Q, 3), or (3,) for one direction shared by every ray; t_limit: (Q,) per-ray upper limits or None.  `leaf_visits`: an int64 tensor of
    one element that gains the number of (wave, leaf) visits (tools/bench_mesh_inside.py)."""
    bvh = _as_bvh(bvh)
    o = _points_arg(origins, "origins")
    shared = directions.dim() == 1
    if shared:
        if directions.shape != (3,):
            raise RuntimeError("a shared direction must have dimensions (3,)")
        d = directions.detach().to(torch.float32).contiguous()
    else:
        d = _points_arg(directions, "directions")
        if o.shape != d.shape:
            raise RuntimeError("origins and directions must have the same dimensions (num_rays, 3)")
    Q = o.shape[0]
    if t_limit is not None:
        if t_limit.shape != (Q,):
            raise RuntimeError("t_limit must have dimensions (num_rays,)")
        t_limit = t_limit.detach().to(torch.float32).contiguous()
    device = _device_of("ray_crossings", o, d, t_limit, bvh.bvh, leaf_visits)
    with torch.cuda.device(device):
        hits = torch.empty((Q,), device=device, dtype=torch.int32)
        winding2 = torch.empty((Q,), device=device, dtype=torch.int32)
        touches = torch.empty((Q,), device=device, dtype=torch.int32)
        ws = torch.empty((_lib.tsi_crossings_workspace_bytes(Q),), device=device, dtype=torch.uint8)
        _check(_lib.tsi_crossings(Q, _native._ptr(o), _native._ptr(d), int(shared), _native._ptr(t_limit), float(tmin), float(tmax),
                                  bvh.num_faces, bvh.bvh.data_ptr(), bvh.bvh.numel(), _native._ptr(hits), _native._ptr(winding2),
                                  _native._ptr(touches), _native._ptr(leaf_visits), ws.data_ptr(), ws.numel(), _native.stream()), "ray_crossings")
    return RayCrossings(hits, winding2, touches)


def _direction(k: int, device) -> torch.Tensor:
    return torch.tensor(INSIDE_DIRECTIONS[k], device=device, dtype=torch.float32)


def winding_number(points: torch.Tensor, mesh) -> Tuple[torch.Tensor, torch.Tensor]:
    """(w (Q,) int32, decided (Q,) bool): w = -winding2 / 2 of the first clean direction; 0 where undecided."""
    bvh = _as_bvh(mesh)
    p = _points_arg(points, "points")
    device = _device_of("winding_number", p, bvh.bvh)
    w = torch.zeros((p.shape[0],), device=device, dtype=torch.int32)
    decided = torch.zeros((p.shape[0],), device=device, dtype=torch.bool)
    todo = torch.arange(p.shape[0], device=device)
    for k in range(len(INSIDE_DIRECTIONS)):
        if todo.numel() == 0:
            break
        c = ray_crossings(bvh, p[todo], _direction(k, device))
        clean = (c.hits >= 0) & (c.touches == 0) & ((c.winding2 & 1) == 0)
        w[todo[clean]] = -(c.winding2[clean] // 2)
        decided[todo[clean]] = True
        todo = todo[~clean]
    return w, decided


def contains_points(points: torch.Tensor, mesh, rule: str = "nonzero", method: str = "rays", beta: float = 2.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(inside (Q,) bool, decided (Q,) bool) by the winding number of every point and `rule`; an undecided point is not inside.
    method = "winding": mesh_winding.contains_points_winding(points, mesh, beta) instead, for meshes that are not closed."""
    code = _rule(rule)
    if _method(method, rule):
        from .mesh_winding import contains_points_winding
        return contains_points_winding(points, mesh, beta)
    w, decided = winding_number(points, mesh)
    inside = (w != 0) if code == 0 else ((w & 1) != 0) if code == 1 else (w > 0)
    return inside & decided, decided


def signed_distance(points: torch.Tensor, mesh, rule: str = "nonzero", method: str = "rays",
                    beta: float = 2.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(sdf (Q,) float32, face (Q,) int32, decided (Q,) bool): the distance to the nearest face (MeshBVH.closest), negative inside by
    `rule`.  A point ON the mesh (distance 0) is +0 and decided; a point without a clean ray keeps the unsigned distance and is not
    decided; a point without a finite distance (a non-finite coordinate, no eligible face) is NaN and not decided.
    method = "winding": mesh_winding.signed_distance_winding(points, mesh, beta) instead, for meshes that are not closed."""
    code = _rule(rule)
    if _method(method, rule):
        from .mesh_winding import signed_distance_winding
        return signed_distance_winding(points, mesh, beta)
    bvh = _as_bvh(mesh)
    p = _points_arg(points, "points")
    device = _device_of("signed_distance", p, bvh.bvh)
    Q = p.shape[0]
    face, dist2, _ = bvh.closest(p)
    with torch.cuda.device(device):
        out = torch.empty((Q,), device=device, dtype=torch.float32)
        decided = torch.empty((Q,), device=device, dtype=torch.uint8)
        if Q:
            c = ray_crossings(bvh, p, _direction(0, device))
            _check(_lib.tsi_signed_distance(Q, dist2.data_ptr(), c.winding2.data_ptr(), c.touches.data_ptr(), c.hits.data_ptr(), code, 0,
                                            out.data_ptr(), decided.data_ptr(), _native.stream()), "signed_distance")
        for k in range(1, len(INSIDE_DIRECTIONS)):  # the retries: only the points that are still undecided are cast again
            todo = (decided == 0).nonzero().reshape(-1)
            n = int(todo.numel())
            if n == 0:
                break
            c = ray_crossings(bvh, p[todo], _direction(k, device))
            sub_d2, sub_out, sub_dec = dist2[todo].contiguous(), out[todo].contiguous(), decided[todo].contiguous()
            _check(_lib.tsi_signed_distance(n, sub_d2.data_ptr(), c.winding2.data_ptr(), c.touches.data_ptr(), c.hits.data_ptr(), code, 1,
                                            sub_out.data_ptr(), sub_dec.data_ptr(), _native.stream()), "signed_distance (retry)")
            out[todo], decided[todo] = sub_out, sub_dec
    return out, face, decided != 0


def _grid_points(origin, voxel_size: float, dims, device) -> torch.Tensor:
    """(nz ny nx, 3) float32, x fastest: sample (i, j, k) at (float)((double)o + (double)h idx) with o and h rounded to fp32 first, the
    sample position of include/ts_volume.h."""
    nx, ny, nz = (int(n) for n in dims)
    o = torch.tensor([float(v) for v in origin], dtype=torch.float32).to(torch.float64)
    h = float(torch.tensor(float(voxel_size), dtype=torch.float32))
    axes = [(o[a] + h * torch.arange(n, dtype=torch.float64)).to(torch.float32).to(device) for a, n in enumerate((nx, ny, nz))]
    z, y, x = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return torch.stack([x, y, z], dim=-1).reshape(-1, 3)


def _check_grid(origin, voxel_size: float, dims):
    dims = tuple(int(n) for n in dims)
    if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] > 1 << 27:
        raise ValueError(f"dims must be three positive counts with at most 2^27 samples in all, got {dims}")
    if len(tuple(origin)) != 3 or not (math.isfinite(float(voxel_size)) and float(voxel_size) > 0.0):
        raise ValueError("origin must have three values and voxel_size must be finite and > 0")
    return dims


def mesh_to_sdf(mesh, origin, voxel_size: float, dims, trunc: Optional[float] = None, rule: str = "nonzero") -> torch.Tensor:
    """(nz, ny, nx) float32: signed_distance of the mesh at the samples of the grid (origin, voxel_size, dims = (nx, ny, nz)) of
    TSDFVolume / extract_isosurface; an undecided sample is NaN, "no data" to the extraction.  With `trunc` the value is divided by it
    (in float64, rounded once) and clipped to [-1, 1], the units of TSDFVolume.field."""
    nx, ny, nz = _check_grid(origin, voxel_size, dims)
    bvh = _as_bvh(mesh)
    sdf, _, decided = signed_distance(_grid_points(origin, voxel_size, (nx, ny, nz), bvh.device), bvh, rule)
    if trunc is not None:
        if not (math.isfinite(float(trunc)) and float(trunc) > 0.0):
            raise ValueError("trunc must be finite and > 0")
        sdf = (sdf.to(torch.float64) / float(trunc)).clamp(-1.0, 1.0).to(torch.float32)
    sdf = torch.where(decided, sdf, torch.full_like(sdf, math.nan))
    return sdf.reshape(nz, ny, nx)


def _bounds(vertices: torch.Tensor, resolution: int, pad_voxels: float, extra: float = 0.0):
    """(origin, voxel_size, dims) in the manner of volume.fusion_bounds: `resolution` samples along the longest side of the bounding box of
    the finite vertices grown by `extra`, with pad_voxels samples of room either side."""
    resolution = int(resolution)
    v = vertices.detach().to(torch.float32)
    finite = v[torch.isfinite(v).all(dim=1)]
    if finite.shape[0] == 0:
        raise ValueError("the mesh needs at least one finite vertex")
    lo = finite.min(dim=0).values.to(torch.float64).cpu() - extra
    hi = finite.max(dim=0).values.to(torch.float64).cpu() + extra
    extent, room = float((hi - lo).max()), resolution - 1 - 2.0 * float(pad_voxels)
    if not (room > 0 and extent > 0.0 and math.isfinite(extent)):
        raise ValueError(f"resolution {resolution} leaves no room for {pad_voxels} voxels of padding either side of the mesh")
    h = extent / room
    dims = tuple(min(resolution, int(math.ceil(float(hi[a] - lo[a]) / h + 2.0 * float(pad_voxels) - 1e-9)) + 1) for a in range(3))
    return (lo - float(pad_voxels) * h).tolist(), h, dims


def _mesh_arrays(mesh):
    return (mesh.vertices, mesh.faces) if isinstance(mesh, MeshBVH) else (mesh[0], mesh[1])


def remesh(mesh, resolution: int, offset: float = 0.0, pad_voxels: int = 2):
    """The mesh as one uniform closed surface: mesh_to_sdf on a grid of `resolution` samples along the longest side of its bounding box
    (grown by a positive `offset`, pad_voxels samples of room either side), extract_isosurface at iso = offset and weld_mesh(eps=0).
    offset > 0 is an outer offset surface, < 0 an inner one.  Returns the WeldedMesh; its stats gain "origin", "voxel_size", "dims",
    "offset", "samples", "undecided" and "inside"."""
    from .mesh_weld import weld_mesh
    from .volume import extract_isosurface
    if not math.isfinite(float(offset)):
        raise ValueError("offset must be finite")
    bvh = _as_bvh(mesh)
    origin, h, dims = _bounds(_mesh_arrays(bvh)[0], resolution, pad_voxels, max(float(offset), 0.0))
    field = mesh_to_sdf(bvh, origin, h, dims)
    vertices, faces = extract_isosurface(field, origin, h, iso=float(offset))
    out = weld_mesh(vertices, faces, eps=0.0)
    out.stats.update(origin=origin, voxel_size=h, dims=dims, offset=float(offset), samples=int(field.numel()),
                     undecided=int(torch.isnan(field).sum().item()), inside=int((field < float(offset)).sum().item()))
    return out


def mesh_volume_iou(mesh_a, mesh_b, resolution: int, origin=None, voxel_size: Optional[float] = None, dims=None, method: str = "rays",
                    beta: float = 2.0) -> Dict[str, object]:
    """The volumetric intersection over union of two meshes: contains_points of both at the samples of ONE grid, `resolution` samples
    along the longest side of the box around both (one voxel of room), or the grid given by origin, voxel_size and dims.  Integer counts
    `inside_a`, `inside_b`, `inside_both`, `inside_either` over the samples that both meshes decide; `undecided` counts the others, which are
    left out; `iou` = inside_both / inside_either (NaN when nothing is inside), `samples`, `origin`, `voxel_size`, `dims`.
    method = "winding": mesh_winding.mesh_volume_iou_winding on the same grid instead, for meshes that are not closed."""
    if _method(method):
        from .mesh_winding import mesh_volume_iou_winding
        return mesh_volume_iou_winding(mesh_a, mesh_b, resolution, origin, voxel_size, dims, beta)
    a, b = _as_bvh(mesh_a), _as_bvh(mesh_b)
    if origin is None:
        origin, voxel_size, dims = _bounds(torch.cat([_mesh_arrays(a)[0], _mesh_arrays(b)[0].to(a.device)]), resolution, 1)
    dims = _check_grid(origin, voxel_size, dims)
    points = _grid_points(origin, voxel_size, dims, a.device)
    in_a, dec_a = contains_points(points, a)
    in_b, dec_b = contains_points(points, b)
    both = dec_a & dec_b
    na, nb = int((in_a & both).sum().item()), int((in_b & both).sum().item())
    nab, nor = int((in_a & in_b & both).sum().item()), int(((in_a | in_b) & both).sum().item())
    return {"inside_a": na, "inside_b": nb, "inside_both": nab, "inside_either": nor, "undecided": int((~both).sum().item()),
            "iou": nab / nor if nor else float("nan"), "samples": int(points.shape[0]), "origin": [float(v) for v in origin],
            "voxel_size": float(voxel_size), "dims": dims}


__all__ = ["INSIDE_DIRECTIONS", "RayCrossings", "ray_crossings", "winding_number", "contains_points", "signed_distance", "mesh_to_sdf", "remesh",
           "mesh_volume_iou"]
