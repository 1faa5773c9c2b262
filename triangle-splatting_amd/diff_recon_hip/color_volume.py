"""Colour through depth fusion: colour fused beside the distances of a TSDFVolume, read off the grid at the extracted surface, and drawn per
vertex -- so that the fused mesh can be scored against images and written like every other mesh here.

    ColorTSDFVolume(origin, voxel_size, dims, trunc, device)       a TSDFVolume with .csum (nz, ny, nx, 3) int64 and .cweight (nz, ny, nx) int32
        .integrate(cam, depth, image=None, mask=None, ...)         the parent's integration, then the view's colour (nothing is read back)
        .color_field(min_weight=1)                                 (3, nz, ny, nx) float32, NaN where fewer than min_weight views coloured
        .extract(min_weight=1, iso=0.0, fill=0.5)                  the welded level set with a colour per vertex: a ColoredMesh
    sample_grid(grid, origin, voxel_size, points)                  trilinear over the samples that have data -> (values (N, C), valid (N,))
    interpolate_vertex_attributes(cam, vertices, faces, face_idx, attributes, background)   (C, H, W): perspective-correct, held inside the face
    render_vertex_colors(cam, vertices, faces, vertex_color)       MeshRenderer's coverage, the vertex colours interpolated, clamped to [0, 1]
    (metrics.evaluate_vertex_colors                                PSNR / SSIM of that render against each view's gt_image)
    fuse_colored_mesh(views, vertices, faces, faces_color, resolution, trunc=None, images=None)   fuse_mesh with colour -> ColoredMesh
    save_glb_mesh(path, vertices, faces, vertex_color)             an indexed glTF 2.0 binary with COLOR_0 per vertex

Every kernel is a pure function of its input (include/ts_color.h): the colour sums are integers, so the state is bit-identical
in any view order and volumes add; the colour of a vertex is a function of its position and the grid alone, so vertices that weld_mesh(eps=0)
merged would have had equal colours bit for bit.

Native code: libts_color.so beside this file (include/ts_color.h, csrc/color_volume.hip), a sixth library because the export lists of the
other five are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import json
import os
import struct
from pathlib import Path
from typing import Dict, NamedTuple, Optional, Sequence

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_color

from .volume import TSDFVolume, _cuda_device, _triple, fusion_bounds

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_color.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The colour volume kernels have no CPU fallback."
    )
_lib = bind_color(C.CDLL(_LIB_PATH))

MAX_CHANNELS = 8  # TSC_MAX_CHANNELS


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsc_last_error().decode()} (ts2d error {rc})")


class ColoredMesh(NamedTuple):
    vertices: torch.Tensor      # (V', 3) float32: the welded level set
    faces: torch.Tensor         # (F', 3) int32
    vertex_color: torch.Tensor  # (V', 3) float32: the colour field at the vertex, `fill` where color_valid is False
    color_valid: torch.Tensor   # (V',) bool: at least one corner of the vertex's cell carried colour with a positive weight
    stats: Dict[str, object]    # the weld's


def sample_grid(grid: torch.Tensor, origin, voxel_size: float, points: torch.Tensor):
    """Trilinear samples of `grid` ((C, nz, ny, nx) or (nz, ny, nx) float32 on a HIP device, 1 <= C <= 8, sample (i, j, k) at origin +
    voxel_size * (i, j, k)) at `points` (N, 3).  A sample has data iff all C of its values are finite; the corners without data are left out
    and the weights of the others renormalised.  Returns (values (N, C) float32, valid (N,) bool); a point outside the grid, or whose corners
    with data weigh nothing, gets NaN and False."""
    if grid.dtype != torch.float32 or grid.dim() not in (3, 4):
        raise RuntimeError("grid must be a float32 tensor with dimensions (C, nz, ny, nx) or (nz, ny, nx)")
    device = _cuda_device(grid.device)
    g = grid.detach().contiguous()
    channels = 1 if g.dim() == 3 else g.shape[0]
    nz, ny, nx = g.shape[-3:]
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("points must have dimensions (N, 3)")
    ox, oy, oz = _triple(origin, float)
    N = points.shape[0]
    with torch.cuda.device(device):
        pts = points.detach().to(device=device, dtype=torch.float32).contiguous()
        out = torch.empty((N, channels), device=device, dtype=torch.float32)
        valid = torch.empty((N,), device=device, dtype=torch.uint8)
        _check(_lib.tsc_sample(nx, ny, nz, ox, oy, oz, float(voxel_size), channels, g.data_ptr(), N, _native._ptr(pts), _native._ptr(out),
                               _native._ptr(valid), _native.stream()), "sample_grid")
    return out, valid.to(torch.bool)


class ColorTSDFVolume(TSDFVolume):
    """A TSDFVolume that also holds `csum` (nz, ny, nx, 3) int64, the colours of the views that saw a sample inside the band |sd| <= trunc in
    units of 2^-16 clamped to [0, 1], and `cweight` (nz, ny, nx) int32, the number of views behind them."""

    def __init__(self, origin, voxel_size: float, dims: Sequence[int], trunc: float, device="cuda"):
        super().__init__(origin, voxel_size, dims, trunc, device)
        nx, ny, nz = self.dims
        self.csum = torch.zeros((nz, ny, nx, 3), device=self.device, dtype=torch.int64)
        self.cweight = torch.zeros((nz, ny, nx), device=self.device, dtype=torch.int32)

    def integrate(self, cam, depth: torch.Tensor, image: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                  carve_uncovered: bool = False, updated: Optional[torch.Tensor] = None, colored: Optional[torch.Tensor] = None) -> None:
        """TSDFVolume.integrate of the view, then, when `image` (3, H, W) is given, its colour: a sample takes the colour of the pixel it
        projects to where that pixel's depth is finite and > 0 and the sample lies within trunc of it; pixels whose colour is NaN or infinite
        colour nothing.  `colored`: an int64 tensor of one element that gains the number of samples coloured.  Nothing is read back."""
        super().integrate(cam, depth, mask=mask, carve_uncovered=carve_uncovered, updated=updated)
        if image is None:
            return
        W, H = int(cam.image_width), int(cam.image_height)
        if tuple(image.shape) != (3, H, W):
            raise RuntimeError(f"image must have dimensions (3, {H}, {W})")
        nx, ny, nz = self.dims
        with torch.cuda.device(self.device):
            depth = depth.detach().to(device=self.device, dtype=torch.float32).contiguous()
            image = image.detach().to(device=self.device, dtype=torch.float32).contiguous()
            view = cam.world_view_transform.detach().to(device=self.device, dtype=torch.float32).contiguous()
            if mask is not None:
                mask = (mask.detach().to(self.device) != 0).to(torch.uint8).contiguous()
            _check(_lib.tsc_integrate(nx, ny, nz, *self.origin, self.voxel_size, self.trunc, view.data_ptr(), float(cam.tan_fovx),
                                      float(cam.tan_fovy), W, H, depth.data_ptr(), _native._ptr(mask), image.data_ptr(), self.csum.data_ptr(),
                                      self.cweight.data_ptr(), _native._ptr(colored), _native.stream()), "ColorTSDFVolume.integrate")

    def color_field(self, min_weight: int = 1) -> torch.Tensor:
        """(3, nz, ny, nx) float32: csum / (cweight 2^16), the mean colour; NaN in all three channels below min_weight views."""
        nx, ny, nz = self.dims
        with torch.cuda.device(self.device):
            out = torch.empty((3, nz, ny, nx), device=self.device, dtype=torch.float32)
            _check(_lib.tsc_color_field(nx, ny, nz, self.csum.data_ptr(), self.cweight.data_ptr(), int(min_weight), out.data_ptr(),
                                        _native.stream()), "ColorTSDFVolume.color_field")
        return out

    def extract(self, min_weight: int = 1, iso: float = 0.0, fill: float = 0.5) -> ColoredMesh:
        """The parent's welded level set with sample_grid of color_field(min_weight) at its vertices; `fill` where no colour was found."""
        mesh = super().extract(min_weight, iso, weld=True)
        values, valid = sample_grid(self.color_field(min_weight), self.origin, self.voxel_size, mesh.vertices)
        color = torch.where(valid[:, None], values, torch.full_like(values, float(fill)))
        return ColoredMesh(mesh.vertices, mesh.faces, color, valid, mesh.stats)


def interpolate_vertex_attributes(cam, vertices: torch.Tensor, faces: torch.Tensor, face_idx: torch.Tensor, attributes: torch.Tensor,
                                  background: torch.Tensor, return_bary: bool = False):
    """(C, H, W) float32: at every pixel whose face_idx (H, W) int32 names a face of `faces` (F, 3) with indices inside `vertices` (V, 3), the
    attributes (V, C) of the face's vertices weighted by the perspective-correct barycentrics of the pixel-centre ray's hit on the face's
    plane, held inside the face; `background` (C,) elsewhere.  Nothing is clamped.  return_bary: also (3, H, W), the weights (0 where nothing
    was drawn).  `cam` is duck-typed as for MeshRenderer."""
    W, H = int(cam.image_width), int(cam.image_height)
    device = _cuda_device(vertices.device)
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError("vertices must have dimensions (num_vertices, 3)")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("faces must have dimensions (num_faces, 3)")
    if attributes.dim() != 2 or attributes.shape[0] != vertices.shape[0] or not 1 <= attributes.shape[1] <= MAX_CHANNELS:
        raise RuntimeError(f"attributes must have dimensions (num_vertices, C) with 1 <= C <= {MAX_CHANNELS}")
    if face_idx.numel() != H * W:
        raise RuntimeError(f"face_idx must have dimensions ({H}, {W})")
    channels = attributes.shape[1]
    if background.numel() != channels:
        raise RuntimeError(f"background must have {channels} values")
    with torch.cuda.device(device):
        vertices = vertices.detach().to(device=device, dtype=torch.float32).contiguous()
        faces = faces.to(device=device, dtype=torch.int32).contiguous()
        face_idx = face_idx.to(device=device, dtype=torch.int32).contiguous()
        attributes = attributes.detach().to(device=device, dtype=torch.float32).contiguous()
        background = background.detach().to(device=device, dtype=torch.float32).contiguous()
        view = cam.world_view_transform.detach().to(device=device, dtype=torch.float32).contiguous()
        out = torch.empty((channels, H, W), device=device, dtype=torch.float32)
        bary = torch.empty((3, H, W), device=device, dtype=torch.float32) if return_bary else None
        _check(_lib.tsc_interpolate(view.data_ptr(), float(cam.tan_fovx), float(cam.tan_fovy), W, H, vertices.shape[0], _native._ptr(vertices),
                                    faces.shape[0], _native._ptr(faces), face_idx.data_ptr(), channels, _native._ptr(attributes),
                                    background.data_ptr(), out.data_ptr(), _native._ptr(bary), _native.stream()), "interpolate_vertex_attributes")
    return (out, bary) if return_bary else out


def render_vertex_colors(cam, vertices: torch.Tensor, faces: torch.Tensor, vertex_color: torch.Tensor,
                         bg_color: torch.Tensor = torch.Tensor([0, 0, 0])) -> Dict[str, torch.Tensor]:
    """MeshRenderer(cam).render's dictionary for a mesh with one colour per VERTEX: coverage, `mask`, `depth` and `face_idx` are the
    renderer's; `render` (3, H, W) is the vertex colours (V, 3) interpolated over each pixel's winning face, bg_color elsewhere, clamped to
    [0, 1]."""
    from .mesh_renderer import MeshRenderer
    flat = torch.zeros((faces.shape[0], 3), device=vertices.device, dtype=torch.float32)
    out = MeshRenderer(cam, bg_color).render(vertices=vertices, faces=faces, faces_color=flat)
    image = interpolate_vertex_attributes(cam, vertices, faces, out["face_idx"], vertex_color, bg_color.to(torch.float32))
    return {"render": image.clamp_(0.0, 1.0), "mask": out["mask"], "depth": out["depth"], "face_idx": out["face_idx"]}


def fuse_colored_mesh(views, vertices: torch.Tensor, faces: torch.Tensor, faces_color: torch.Tensor, resolution: int,
                      trunc: Optional[float] = None, images=None, return_volume: bool = False):
    """fuse_mesh with colour: every view's MeshRenderer depth integrated with carving into a ColorTSDFVolume of fuse_mesh's bounds, and with
    it the view's image -- images[v] (3, H, W) when given (the training targets), else the renderer's own `render` of faces_color (F, 3) --
    then extracted, welded and coloured.  Returns a ColoredMesh (with return_volume: and the ColorTSDFVolume)."""
    from .mesh_renderer import MeshRenderer
    if int(resolution) < 2:
        raise ValueError("resolution must be at least 2")
    device = _cuda_device(vertices.device)
    v = vertices.detach().to(torch.float32)
    volume = ColorTSDFVolume(*fusion_bounds(v, resolution, trunc), device)
    for k, cam in enumerate(views):
        out = MeshRenderer(cam).render(vertices=v, faces=faces, faces_color=faces_color)
        volume.integrate(cam, out["depth"], image=out["render"] if images is None else images[k], carve_uncovered=True)
    mesh = volume.extract()
    return (mesh, volume) if return_volume else mesh


def save_glb_mesh(path, vertices, faces, vertex_color) -> None:
    """Writes the indexed mesh (vertices (V, 3), faces (F, 3), vertex_color (V, 3) in [0, 1]; tensors or arrays) as a glTF 2.0 binary in the
    container of RawTriangle.saveGLB: POSITION float32, COLOR_0 uint8 VEC4 normalised (alpha 255), uint32 indices.
    diff_recon_hip.mesh_renderer.load_glb_mesh and raw_triangle.read_glb read it back."""
    import numpy as np
    host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    pos = np.ascontiguousarray(host(vertices), dtype="<f4").reshape(-1, 3)
    idx = np.ascontiguousarray(host(faces).reshape(-1), dtype="<u4")
    rgb = np.nan_to_num(host(vertex_color).astype(np.float64).reshape(-1, 3), nan=0.0)
    if len(rgb) != len(pos):
        raise ValueError("vertex_color must have one row per vertex")
    col = np.concatenate([np.round(np.clip(rgb, 0.0, 1.0) * 255.0), np.full((len(pos), 1), 255.0)], axis=1).astype(np.uint8)
    blobs, views, off = [], [], 0
    for arr, target in ((pos, 34962), (np.ascontiguousarray(col), 34962), (idx, 34963)):
        raw = arr.tobytes()
        views.append({"buffer": 0, "byteOffset": off, "byteLength": len(raw), "target": target})
        raw += b"\x00" * (-len(raw) % 4)
        blobs.append(raw)
        off += len(raw)
    doc = {
        "asset": {"version": "2.0", "generator": "diff_recon_hip.color_volume"},
        "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"name": "geometry_0", "mesh": 0}],
        "meshes": [{"name": "geometry_0", "primitives": [{"attributes": {"POSITION": 0, "COLOR_0": 1}, "indices": 2, "mode": 4}]}],
        "buffers": [{"byteLength": off}], "bufferViews": views,
        "accessors": [
            {"bufferView": 0, "componentType": 5126, "count": int(len(pos)), "type": "VEC3",
             "min": [float(x) for x in (pos.min(axis=0) if len(pos) else np.zeros(3))], "max": [float(x) for x in (pos.max(axis=0) if len(pos) else np.zeros(3))]},
            {"bufferView": 1, "componentType": 5121, "normalized": True, "count": int(len(col)), "type": "VEC4"},
            {"bufferView": 2, "componentType": 5125, "count": int(len(idx)), "type": "SCALAR"},
        ],
    }
    js = json.dumps(doc, separators=(",", ":")).encode("utf-8")
    js += b" " * (-len(js) % 4)
    binary = b"".join(blobs)
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        f.write(struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(js) + 8 + len(binary)))
        f.write(struct.pack("<I4s", len(js), b"JSON") + js)
        f.write(struct.pack("<I4s", len(binary), b"BIN\x00") + binary)


__all__ = ["ColorTSDFVolume", "ColoredMesh", "sample_grid", "interpolate_vertex_attributes", "render_vertex_colors", "fuse_colored_mesh",
           "save_glb_mesh"]
