"""Generalised winding numbers on the triangle index: the inside test and the signed distance of OPEN meshes.

    winding_moments(bvh)                                   the far-field record of every node of a MeshBVH: built once, cached on it
    leaf_faces(bvh)                                        the face id of every leaf slot: what a reference needs to restate the tree
    generalized_winding_number(points, mesh, beta=2.0, return_terms=False)
                                                           (w float64, wq int64[, terms (Q, 2) int32]): w = wq 2^-38, NaN for a bad point
    contains_points_winding(points, mesh, beta=2.0, threshold=0.5)      (inside bool, decided bool): wq >= threshold, an integer compare
    signed_distance_winding(points, mesh, beta=2.0, threshold=0.5)      (sdf float32, face int32, decided bool): negative inside
    mesh_to_sdf_winding(mesh, origin, voxel_size, dims, trunc=None, beta=2.0, threshold=0.5)     that on a grid, (nz, ny, nx) float32
    remesh_winding(mesh, resolution, offset=0.0, pad_voxels=2, beta=2.0, threshold=0.5)          its level set: one closed surface
    mesh_volume_iou_winding(mesh_a, mesh_b, resolution, ..., beta=2.0, threshold=0.5)            the volumetric IoU on one grid

`mesh` is a mesh_surface.MeshBVH (built once) or (vertices, faces[, keep]).  mesh_inside.py decides inside and outside by counting the
crossings of a ray: right on a closed, oriented mesh, wrong behind every open sheet, where a ray crosses the surface once all the way to
the border of the grid.  The generalised winding number w(q) = sum over the faces of their signed solid angle seen from q, over 4 pi
(Jacobson et al. 2013), is an integer away from a closed surface and degrades smoothly at a hole: w >= 1/2 is a robust "inside", every
finite point is decided and no ray is retried.  A point inside an outward-facing closed mesh has w = +1, the sign of
mesh_inside.winding_number.

The sum is taken on the MeshBVH's tree with one far-field term per node (Barill et al. 2018, first order): a node whose faces lie within
sqrt(R2) of their area-weighted centre p is replaced by the dipole of its summed area vector when the query is farther than beta sqrt(R2)
from p.  beta = inf is the exact sum over all faces.  Every term is quantised to 2^-38 turns and the sum is a 64-bit integer: the result
is a pure function of the input, whatever the order of the walk (include/ts_winding.h).

Native code: libts_winding.so beside this file (include/ts_winding.h, csrc/mesh_winding.hip), a fourteenth library because the export
lists of the other thirteen are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Optional, Tuple

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_winding

from .mesh_surface import MeshBVH, _device_of, _points_arg

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_winding.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The winding-number kernels have no CPU fallback."
    )
_lib = bind_winding(C.CDLL(_LIB_PATH))

UNITS_PER_TURN = 1 << 38          # include/ts_winding.h: wq counts 2^-38 turns
BAD_QUERY = -(1 << 63)            # wq of a point with a non-finite coordinate


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsn_last_error().decode()} (ts2d error {rc})")


def _as_bvh(bvh) -> MeshBVH:
    return bvh if isinstance(bvh, MeshBVH) else MeshBVH(*bvh)


def _beta(beta: float) -> float:
    beta = float(beta)
    if not beta >= 1.0:
        raise ValueError(f"beta must be at least 1 (inf for the exact sum), not {beta!r}")
    return beta


def threshold_units(threshold: float) -> int:
    """A threshold in turns as the integer that wq is compared with: round(threshold 2^38), half to even."""
    threshold = float(threshold)
    if not math.isfinite(threshold) or abs(threshold) > float(1 << 24):
        raise ValueError(f"threshold must be finite and at most 2^24 turns in magnitude, not {threshold!r}")
    return int(round(threshold * UNITS_PER_TURN))


def _build(bvh: MeshBVH):
    F = bvh.num_faces
    with torch.cuda.device(bvh.device):
        moments = torch.empty((_lib.tsn_moments_bytes(F) // 8,), device=bvh.device, dtype=torch.float64)
        faces = torch.empty((_lib.tsn_leaf_faces_bytes(F) // 4,), device=bvh.device, dtype=torch.int32)
        _check(_lib.tsn_moments(F, bvh.bvh.data_ptr(), bvh.bvh.numel(), _native._ptr(moments), moments.numel() * 8, _native._ptr(faces),
                                faces.numel() * 4, _native.stream()), "winding_moments")
    bvh._winding = (moments.reshape(-1, 8), faces)
    return bvh._winding


def winding_moments(bvh: MeshBVH) -> torch.Tensor:
    """(nodes, 8) float64: [Nx, Ny, Nz, px, py, pz, R2, S] of every node of the index, level 0 (the leaves) first.  Built on the first call
    and kept on the MeshBVH."""
    return (getattr(bvh, "_winding", None) or _build(bvh))[0]


def leaf_faces(bvh: MeshBVH) -> torch.Tensor:
    """(8 ceil(F / 8),) int32: the face id of every leaf slot of the index, -1 for padding and for faces that are not eligible."""
    return (getattr(bvh, "_winding", None) or _build(bvh))[1]


def _winding(bvh: MeshBVH, p: torch.Tensor, beta: float, want_terms: bool):
    device = _device_of("generalized_winding_number", p, bvh.bvh)
    Q, F = p.shape[0], bvh.num_faces
    moments = winding_moments(bvh)
    with torch.cuda.device(device):
        wq = torch.empty((Q,), device=device, dtype=torch.int64)
        terms = torch.empty((Q, 2), device=device, dtype=torch.int32) if want_terms else None
        ws = torch.empty((_lib.tsn_winding_workspace_bytes(Q),), device=device, dtype=torch.uint8)
        _check(_lib.tsn_winding(Q, _native._ptr(p), beta, F, bvh.bvh.data_ptr(), bvh.bvh.numel(), _native._ptr(moments), moments.numel() * 8,
                                _native._ptr(wq), _native._ptr(terms), ws.data_ptr(), ws.numel(), _native.stream()), "generalized_winding_number")
    return wq, terms


def generalized_winding_number(points: torch.Tensor, mesh, beta: float = 2.0, return_terms: bool = False):
    """(w (Q,) float64, wq (Q,) int64): the generalised winding number of the mesh at every point, w = wq 2^-38; a point with a non-finite
    coordinate has w = NaN and wq = INT64_MIN.  beta >= 1 is the far-field ratio, inf the exact sum.  With return_terms a third tensor
    (Q, 2) int32: the faces evaluated and the nodes accepted for each point (-1, -1 for a bad one)."""
    beta = _beta(beta)
    bvh = _as_bvh(mesh)
    wq, terms = _winding(bvh, _points_arg(points, "points"), beta, bool(return_terms))
    w = torch.where(wq == BAD_QUERY, torch.full_like(wq, math.nan, dtype=torch.float64), wq.to(torch.float64) / UNITS_PER_TURN)
    return (w, wq, terms) if return_terms else (w, wq)


def contains_points_winding(points: torch.Tensor, mesh, beta: float = 2.0, threshold: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
    """(inside (Q,) bool, decided (Q,) bool): wq >= round(threshold 2^38), an integer compare; every point with finite coordinates is
    decided, the others are not inside."""
    beta, thr = _beta(beta), threshold_units(threshold)
    wq, _ = _winding(_as_bvh(mesh), _points_arg(points, "points"), beta, False)
    decided = wq != BAD_QUERY
    return (wq >= thr) & decided, decided


def signed_distance_winding(points: torch.Tensor, mesh, beta: float = 2.0, threshold: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(sdf (Q,) float32, face (Q,) int32, decided (Q,) bool): the distance to the nearest face (MeshBVH.closest), negative where
    wq >= the threshold.  A point ON the mesh (distance 0) is +0; a point without a finite distance (a non-finite coordinate, no eligible
    face) is NaN and not decided; every other point is decided."""
    beta, thr = _beta(beta), threshold_units(threshold)
    bvh = _as_bvh(mesh)
    p = _points_arg(points, "points")
    device = _device_of("signed_distance_winding", p, bvh.bvh)
    Q = p.shape[0]
    face, dist2, _ = bvh.closest(p)
    wq, _ = _winding(bvh, p, beta, False)
    with torch.cuda.device(device):
        out = torch.empty((Q,), device=device, dtype=torch.float32)
        decided = torch.empty((Q,), device=device, dtype=torch.uint8)
        _check(_lib.tsn_sign_distance(Q, _native._ptr(dist2), _native._ptr(wq), thr, _native._ptr(out), _native._ptr(decided), _native.stream()),
               "signed_distance_winding")
    return out, face, decided != 0


def mesh_to_sdf_winding(mesh, origin, voxel_size: float, dims, trunc: Optional[float] = None, beta: float = 2.0,
                        threshold: float = 0.5) -> torch.Tensor:
    """(nz, ny, nx) float32: signed_distance_winding at the samples of the grid of mesh_inside.mesh_to_sdf, with its `trunc`; only a mesh
    without an eligible face leaves NaNs."""
    from .mesh_inside import _check_grid, _grid_points
    nx, ny, nz = _check_grid(origin, voxel_size, dims)
    bvh = _as_bvh(mesh)
    sdf, _, decided = signed_distance_winding(_grid_points(origin, voxel_size, (nx, ny, nz), bvh.device), bvh, beta, threshold)
    if trunc is not None:
        if not (math.isfinite(float(trunc)) and float(trunc) > 0.0):
            raise ValueError("trunc must be finite and > 0")
        sdf = (sdf.to(torch.float64) / float(trunc)).clamp(-1.0, 1.0).to(torch.float32)
    sdf = torch.where(decided, sdf, torch.full_like(sdf, math.nan))
    return sdf.reshape(nz, ny, nx)


def remesh_winding(mesh, resolution: int, offset: float = 0.0, pad_voxels: int = 2, beta: float = 2.0, threshold: float = 0.5):
    """mesh_inside.remesh with the winding-number sign: the level set of mesh_to_sdf_winding, welded.  An open input comes out closed: the
    sign changes only where w crosses the threshold, across the surface and across the caps that w = threshold spans over its holes."""
    from .mesh_inside import _bounds, _mesh_arrays
    from .mesh_weld import weld_mesh
    from .volume import extract_isosurface
    if not math.isfinite(float(offset)):
        raise ValueError("offset must be finite")
    bvh = _as_bvh(mesh)
    origin, h, dims = _bounds(_mesh_arrays(bvh)[0], resolution, pad_voxels, max(float(offset), 0.0))
    field = mesh_to_sdf_winding(bvh, origin, h, dims, beta=beta, threshold=threshold)
    vertices, faces = extract_isosurface(field, origin, h, iso=float(offset))
    out = weld_mesh(vertices, faces, eps=0.0)
    out.stats.update(origin=origin, voxel_size=h, dims=dims, offset=float(offset), samples=int(field.numel()),
                     undecided=int(torch.isnan(field).sum().item()), inside=int((field < float(offset)).sum().item()), method="winding",
                     beta=float(beta), threshold=float(threshold))
    return out


def mesh_volume_iou_winding(mesh_a, mesh_b, resolution: int, origin=None, voxel_size: Optional[float] = None, dims=None, beta: float = 2.0,
                            threshold: float = 0.5) -> Dict[str, object]:
    """mesh_inside.mesh_volume_iou with contains_points_winding: the same keys, in integer counts."""
    from .mesh_inside import _bounds, _check_grid, _grid_points, _mesh_arrays
    a, b = _as_bvh(mesh_a), _as_bvh(mesh_b)
    if origin is None:
        origin, voxel_size, dims = _bounds(torch.cat([_mesh_arrays(a)[0], _mesh_arrays(b)[0].to(a.device)]), resolution, 1)
    dims = _check_grid(origin, voxel_size, dims)
    points = _grid_points(origin, voxel_size, dims, a.device)
    in_a, dec_a = contains_points_winding(points, a, beta, threshold)
    in_b, dec_b = contains_points_winding(points, b, beta, threshold)
    both = dec_a & dec_b
    na, nb = int((in_a & both).sum().item()), int((in_b & both).sum().item())
    nab, nor = int((in_a & in_b & both).sum().item()), int(((in_a | in_b) & both).sum().item())
    return {"inside_a": na, "inside_b": nb, "inside_both": nab, "inside_either": nor, "undecided": int((~both).sum().item()),
            "iou": nab / nor if nor else float("nan"), "samples": int(points.shape[0]), "origin": [float(v) for v in origin],
            "voxel_size": float(voxel_size), "dims": dims}


__all__ = ["UNITS_PER_TURN", "winding_moments", "leaf_faces", "generalized_winding_number", "contains_points_winding", "signed_distance_winding",
           "mesh_to_sdf_winding", "remesh_winding", "mesh_volume_iou_winding", "threshold_units"]
