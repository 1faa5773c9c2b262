"""Surface from depth: per-view depth fused into a truncated signed distance (TSDF) volume, and the zero level set extracted as one
connected, oriented, closed mesh.

    TSDFVolume(origin, voxel_size, dims, trunc, device)
        .integrate(cam, depth, mask=None, carve_uncovered=False)   one view into the state (nothing is read back)
        .field(min_weight=1)                                       (nz, ny, nx) float32, NaN where fewer than min_weight views saw the sample
        .extract(min_weight=1, iso=0.0, weld=True)                 the level set as a WeldedMesh (mesh_weld.py)
        .sum (int64), .weight (int32)                              the state: integers, so volumes add (`a.sum += b.sum; a.weight += b.weight`)
    extract_isosurface(field, origin, voxel_size, iso=0.0)         marching tetrahedra on any (nz, ny, nx) fp32 grid -> (vertices (3T, 3), faces (T, 3))
    fuse_mesh(views, vertices, faces, resolution, trunc=None)      MeshRenderer depth of every view, fused with carving, extracted and welded;
                                                                   simplify_cell=K (voxels) / min_piece_faces=N: mesh_simplify.py behind it

Both kernels are pure functions of their input (include/ts_volume.h): the sums are integers, so the state is bit-identical in
any view order; the vertex of a grid edge is a function of the edge alone, so every tetrahedron that shares it writes the same bits and
weld_mesh(eps=0) closes the soup.  NaN or infinite field values are "no data": cells that touch one emit nothing and leave a boundary loop.

Native code: libts_volume.so beside this file (include/ts_volume.h, csrc/volume.hip), a fifth library because the export lists of the other
four are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Sequence

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_volume

from .mesh_weld import weld_mesh

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_volume.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The volume kernels have no CPU fallback."
    )
_lib = bind_volume(C.CDLL(_LIB_PATH))

CARVE_UNCOVERED = 1  # TSV_CARVE_UNCOVERED


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsv_last_error().decode()} (ts2d error {rc})")


def _cuda_device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the TSDF volume (MI355X build) lives on a HIP device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def _triple(x, cast):
    t = tuple(cast(v) for v in (x.tolist() if isinstance(x, torch.Tensor) else x))
    if len(t) != 3:
        raise ValueError(f"expected three values, got {len(t)}")
    return t


def extract_isosurface(field: torch.Tensor, origin, voxel_size: float, iso: float = 0.0, with_cells: bool = False):
    """Marching tetrahedra on `field` (nz, ny, nx) float32 on a HIP device, sample (i, j, k) at origin + voxel_size * (i, j, k): the level
    set f = iso as a triangle soup, (vertices (3T, 3) float32, faces (T, 3) int32) with three private vertices per triangle, normals
    pointing from f < iso to f >= iso.  NaN and infinite samples are "no data".  with_cells: also (T,) int32, the linear sample index of
    each triangle's cell.  Two calls: the count is read back, the soup allocated, the triangles written."""
    if field.dim() != 3 or field.dtype != torch.float32:
        raise RuntimeError("field must be a float32 tensor with dimensions (nz, ny, nx)")
    device = _cuda_device(field.device)
    field = field.detach().contiguous()
    nz, ny, nx = field.shape
    ox, oy, oz = _triple(origin, float)
    with torch.cuda.device(device):
        ws = torch.empty((_lib.tsv_extract_workspace_bytes(nx, ny, nz),), device=device, dtype=torch.uint8)
        total = torch.empty((1,), device=device, dtype=torch.int64)
        args = (nx, ny, nz, ox, oy, oz, float(voxel_size), field.data_ptr(), float(iso))
        _check(_lib.tsv_extract(*args, 0, None, None, total.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream()), "extract_isosurface (count)")
        T = int(total.item())
        triangles = torch.empty((T, 3, 3), device=device, dtype=torch.float32)
        cells = torch.empty((T,), device=device, dtype=torch.int32) if with_cells else None
        if T:
            _check(_lib.tsv_extract(*args, T, triangles.data_ptr(), _native._ptr(cells), total.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _native.stream()), "extract_isosurface")
        faces = torch.arange(3 * T, device=device, dtype=torch.int32).reshape(T, 3)
    vertices = triangles.reshape(3 * T, 3)
    return (vertices, faces, cells) if with_cells else (vertices, faces)


class TSDFVolume:
    """nx * ny * nz samples, sample (i, j, k) at origin + voxel_size * (i, j, k); dims = (nx, ny, nz).  The state is `sum` (nz, ny, nx) int64,
    the signed distances in units of trunc / 2^20 clipped at +trunc, and `weight` (nz, ny, nx) int32, the number of views behind it."""

    def __init__(self, origin, voxel_size: float, dims: Sequence[int], trunc: float, device="cuda"):
        self.device = _cuda_device(device)
        self.origin = _triple(origin, float)
        self.dims = _triple(dims, int)
        self.voxel_size, self.trunc = float(voxel_size), float(trunc)
        nx, ny, nz = self.dims
        if min(self.dims) < 1 or nx * ny * nz > 1 << 27:
            raise ValueError(f"dims must be positive with at most 2^27 samples in all, got {self.dims}")
        for name, v in (("voxel_size", self.voxel_size), ("trunc", self.trunc)):
            if not (math.isfinite(v) and v > 0.0):
                raise ValueError(f"{name} must be finite and > 0, not {v}")
        self.sum = torch.zeros((nz, ny, nx), device=self.device, dtype=torch.int64)
        self.weight = torch.zeros((nz, ny, nx), device=self.device, dtype=torch.int32)

    def integrate(self, cam, depth: torch.Tensor, mask: Optional[torch.Tensor] = None, carve_uncovered: bool = False,
                  updated: Optional[torch.Tensor] = None) -> None:
        """One view into the state.  `cam` is duck-typed as for MeshRenderer (`world_view_transform` in the row-vector convention,
        `tan_fovx`, `tan_fovy`, `image_width`, `image_height`); depth (H, W): view-space depth, 0 = uncovered, NaN / inf / negative =
        ignored; mask (H, W), optional: pixels that are 0 / False are ignored.  carve_uncovered: an uncovered pixel marks its ray as free
        space (what closes the surface at silhouettes) instead of saying nothing.  `updated`: an int64 tensor of one element that gains the
        number of samples updated.  Nothing is read back."""
        W, H = int(cam.image_width), int(cam.image_height)
        if tuple(depth.shape[-2:]) != (H, W) or depth.numel() != H * W:
            raise RuntimeError(f"depth must have dimensions ({H}, {W})")
        if mask is not None and mask.numel() != H * W:
            raise RuntimeError(f"mask must have dimensions ({H}, {W})")
        if not depth.is_cuda:
            raise RuntimeError("TSDFVolume.integrate (MI355X build) needs depth on a HIP device; there is no CPU fallback")
        nx, ny, nz = self.dims
        with torch.cuda.device(self.device):
            depth = depth.detach().to(device=self.device, dtype=torch.float32).contiguous()
            view = cam.world_view_transform.detach().to(device=self.device, dtype=torch.float32).contiguous()
            if mask is not None:
                mask = (mask.detach().to(self.device) != 0).to(torch.uint8).contiguous()
            _check(_lib.tsv_integrate(nx, ny, nz, *self.origin, self.voxel_size, self.trunc, view.data_ptr(), float(cam.tan_fovx),
                                      float(cam.tan_fovy), W, H, depth.data_ptr(), _native._ptr(mask), CARVE_UNCOVERED if carve_uncovered else 0,
                                      self.sum.data_ptr(), self.weight.data_ptr(), _native._ptr(updated), _native.stream()), "TSDFVolume.integrate")

    def field(self, min_weight: int = 1) -> torch.Tensor:
        """(nz, ny, nx) float32: sum / (weight 2^20), the mean signed distance in units of trunc, at most 1; NaN below min_weight views."""
        nx, ny, nz = self.dims
        with torch.cuda.device(self.device):
            out = torch.empty((nz, ny, nx), device=self.device, dtype=torch.float32)
            _check(_lib.tsv_field(nx, ny, nz, self.sum.data_ptr(), self.weight.data_ptr(), int(min_weight), out.data_ptr(), _native.stream()),
                   "TSDFVolume.field")
        return out

    def extract(self, min_weight: int = 1, iso: float = 0.0, weld: bool = True):
        """The level set of field(min_weight) at `iso` (in units of trunc): welded with eps = 0 into a WeldedMesh, or with weld=False the
        soup (vertices (3T, 3), faces (T, 3))."""
        vertices, faces = extract_isosurface(self.field(min_weight), self.origin, self.voxel_size, iso)
        return weld_mesh(vertices, faces, eps=0.0) if weld else (vertices, faces)


def fuse_mesh(views, vertices: torch.Tensor, faces: torch.Tensor, resolution: int, trunc: Optional[float] = None,
              return_volume: bool = False, simplify_cell: Optional[float] = None, min_piece_faces: int = 0):
    """The closed surface that the views see of the mesh (vertices (V, 3), faces (F, 3)): every view's MeshRenderer depth integrated with
    carving into a volume of `resolution` samples along the longest side of the bounding box of the finite vertices, padded by trunc
    (default 4 voxels); then extracted and welded.  Returns a WeldedMesh (with return_volume: and the TSDFVolume).
    simplify_cell (in voxels, on the volume's own grid) and min_piece_faces, when given, run simplify_mesh and drop_small_pieces
    (mesh_simplify.py) on the welded level set: vertex_map and face_keep then lead from the level set to the result and stats gains
    "simplify" / "small_piece_faces" (mesh_simplify.simplify_fused; the same call serves a fuse_colored_mesh result).  Their defaults change
    nothing."""
    from .mesh_renderer import MeshRenderer
    if int(resolution) < 2:
        raise ValueError("resolution must be at least 2")
    device = _cuda_device(vertices.device)
    v = vertices.detach().to(torch.float32)
    volume = TSDFVolume(*fusion_bounds(v, resolution, trunc), device)
    colour = torch.zeros((faces.shape[0], 3), device=device, dtype=torch.float32)
    for cam in views:
        out = MeshRenderer(cam).render(vertices=v, faces=faces, faces_color=colour)
        volume.integrate(cam, out["depth"], carve_uncovered=True)
    mesh = volume.extract()
    if simplify_cell is not None or int(min_piece_faces) > 0:
        from .mesh_simplify import simplify_fused
        mesh = simplify_fused(mesh, volume, simplify_cell, min_piece_faces)
    return (mesh, volume) if return_volume else mesh


def fusion_bounds(vertices: torch.Tensor, resolution: int, trunc: Optional[float] = None):
    """(origin, voxel_size, dims, trunc) of the volume fuse_mesh builds around `vertices` (V, 3): `resolution` samples along the longest side
    of the bounding box of the finite vertices, padded by trunc (default 4 voxels) either side."""
    resolution = int(resolution)
    if resolution < 2:
        raise ValueError("resolution must be at least 2")
    v = vertices.detach().to(torch.float32)
    finite = v[torch.isfinite(v).all(dim=1)]
    if finite.shape[0] == 0:
        raise ValueError("fuse_mesh needs at least one finite vertex")
    lo, hi = finite.min(dim=0).values.to(torch.float64).cpu(), finite.max(dim=0).values.to(torch.float64).cpu()
    extent = float((hi - lo).max())
    # h from the padded extent: (resolution - 1) h = extent + 2 trunc, trunc = 4 h by default
    h = (extent + 2.0 * float(trunc)) / (resolution - 1) if trunc is not None else extent / (resolution - 9) if resolution > 9 else None
    if h is None or not (h > 0.0 and math.isfinite(h)):
        raise ValueError(f"resolution {resolution} leaves no room for the padding of {'4 voxels' if trunc is None else trunc} either side")
    tr = float(trunc) if trunc is not None else 4.0 * h
    dims = tuple(min(resolution, int(math.ceil((float(hi[a] - lo[a]) + 2.0 * tr) / h - 1e-9)) + 1) for a in range(3))
    return (lo - tr).tolist(), h, dims, tr


__all__ = ["TSDFVolume", "extract_isosurface", "fuse_mesh", "fusion_bounds", "CARVE_UNCOVERED"]
