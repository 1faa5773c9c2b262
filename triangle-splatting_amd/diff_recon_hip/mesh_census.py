"""`MeshCensus`: what the opaque mesh renderer's `face_idx` image says about the mesh, summed over views -- how many pixels every face wins
and the sum of the target pixels it wins -- and the two refinements of an exported mesh that follow from it:

    bake_face_colors(views, ...)        the best constant colour of a face under the opaque render: the mean of the target pixels it wins
    visible_triangle_mask(views, ...)   the triangles that win at least `min_pixels` pixels from any of the views (multi-view visibility)

Native code: libts2d.so (include/ts_mesh.h: ts2d_mesh_census_add, csrc/mesh_census.hip), bound with ctypes like mesh_renderer.py.  The
accumulator holds 64-bit INTEGERS (pixel counts and Q16 fixed-point colour sums), so a census is a pure function of its inputs: the same
views in any order, on any rank, in any run leave the same bits.  No CPU / eager fallback.

Twins.  `mesh_from_triangles(save_back=True)` appends every triangle's back face as a reversed twin, face f + P behind face f, naming the
same three vertices.  The renderer builds a face's record from its vertices in ascending index order, so a twin has its front face's
coverage and depth on every pixel, bit for bit, and ties go to the smaller index: a twin never wins a pixel in this renderer.  The raw
census of such a mesh has empty rows P .. 2 P - 1, and a front face stands for its triangle.  Visibility and colour are therefore per
TRIANGLE: `fold_twins` adds rows f and f + P (which also covers a mesh whose twins name other, coincident vertices and so may win), a kept
triangle keeps both faces, and both faces get the same baked colour -- which is also all a GLB file can hold (one colour per triangle)."""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch

from diff_triangle_rasterization_2D import _C as _native

from .mesh_renderer import MeshRenderer, mesh_from_triangles

_lib = _native._lib

Q16 = 65536.0


class MeshCensus:
    """Per-face accumulator over views.  `acc` is an (F, 4) int64 tensor {pixels, sum_r, sum_g, sum_b}, zero at the start; the colour sums
    are Q16 fixed point (round-to-nearest-even of clip(target, 0, 1) * 65536, a NaN target counting as 0).  The kernel adds to it as
    unsigned 64-bit words; its values stay far below 2^63, so it reads as int64."""

    def __init__(self, num_faces: int, device):
        if num_faces < 0:
            raise ValueError("num_faces must be >= 0")
        self.acc = torch.zeros((int(num_faces), 4), device=device, dtype=torch.int64)

    @property
    def num_faces(self) -> int:
        return self.acc.shape[0]

    def add(self, face_idx: torch.Tensor, target: Optional[torch.Tensor] = None, pixel_mask: Optional[torch.Tensor] = None) -> "MeshCensus":
        """Adds one view on the current stream.  face_idx (H, W) int32 (MeshRenderer's output); a pixel is counted iff its index lies in
        [0, F) and `pixel_mask` ((H, W) or (1, H, W) float32), when given, is > 0 there.  With `target` ((3, H, W) float32) the face's
        colour sums grow too; without it only the pixel counts."""
        if face_idx.dim() != 2 or face_idx.dtype != torch.int32:
            raise RuntimeError("face_idx must be an int32 tensor with dimensions (H, W)")
        H, W = face_idx.shape
        if target is not None and (target.shape != (3, H, W) or target.dtype != torch.float32):
            raise RuntimeError("target must be a float32 tensor with dimensions (3, H, W)")
        if pixel_mask is not None and (tuple(pixel_mask.shape) not in ((H, W), (1, H, W)) or pixel_mask.dtype != torch.float32):
            raise RuntimeError("pixel_mask must be a float32 tensor with dimensions (H, W) or (1, H, W)")
        if H < 1 or W < 1:
            raise RuntimeError("face_idx must hold at least one pixel")
        device = self.acc.device
        tensors = [x for x in (face_idx, target, pixel_mask) if x is not None]
        if device.type != "cuda" or any(x.device != device for x in tensors):
            raise RuntimeError("MeshCensus (MI355X build) needs the accumulator and the images on one HIP device; there is no CPU fallback")
        with torch.cuda.device(device):
            face_idx = face_idx.contiguous()
            target = target.detach().contiguous() if target is not None else None
            pixel_mask = pixel_mask.detach().contiguous() if pixel_mask is not None else None
            stream = _native.stream()
            _native._check(_lib.ts2d_mesh_census_add(W, H, self.num_faces, face_idx.data_ptr(), _native._ptr(target), _native._ptr(pixel_mask),
                                                     _native._ptr(self.acc) if self.num_faces else None, stream), "MeshCensus.add")
        return self

    def add_view(self, view, vertices: torch.Tensor, faces: torch.Tensor, faces_color: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Renders the mesh with MeshRenderer(view) and adds the result with `view.gt_image` as the target, under `view.alpha_mask` when the
        view has one: the pixels counted are then exactly the ones evaluate_mesh's PSNR weighs.  Returns the render dict.  `faces_color`
        only colours the returned image (grey when missing); the census does not depend on it."""
        if faces_color is None:
            faces_color = torch.full((faces.shape[0], 3), 0.5, device=vertices.device, dtype=torch.float32)
        out = MeshRenderer(view).render(vertices, faces, faces_color)
        device = out["face_idx"].device
        alpha = getattr(view, "alpha_mask", None)
        self.add(out["face_idx"], view.gt_image.to(device=device, dtype=torch.float32),
                 alpha.to(device=device, dtype=torch.float32) if alpha is not None else None)
        return out

    def pixels(self) -> torch.Tensor:
        """(F,) int64: the pixels every face has won."""
        return self.acc[:, 0].clone()

    def mean_color(self, fallback: torch.Tensor) -> torch.Tensor:
        """(F, 3) float32: float32(float64(sum) / (float64(pixels) * 65536)) where the face has pixels, the row of `fallback` elsewhere."""
        if fallback.shape != (self.num_faces, 3):
            raise ValueError("fallback must have dimensions (num_faces, 3)")
        n = self.acc[:, :1]
        mean = (self.acc[:, 1:].to(torch.float64) / (n.clamp_min(1).to(torch.float64) * Q16)).to(torch.float32)
        return torch.where(n > 0, mean, fallback.to(device=self.acc.device, dtype=torch.float32))

    def fold_twins(self, P: int) -> "MeshCensus":
        """A census of P rows, row f = rows f and f + P of this one added: per triangle, for the layout of mesh_from_triangles(save_back=True)."""
        if self.num_faces != 2 * P:
            raise ValueError(f"fold_twins({P}) needs a census of {2 * P} faces, not {self.num_faces}")
        out = MeshCensus(0, self.acc.device)
        out.acc = self.acc[:P] + self.acc[P:]
        return out


def bake_face_colors(views: Iterable, vertices: torch.Tensor, faces: torch.Tensor, faces_color: torch.Tensor,
                     twin_period: Optional[int] = None) -> torch.Tensor:
    """New (F, 3) face colours: one census over all `views` (cameras with `gt_image`, optionally `alpha_mask`, as evaluate_mesh takes them),
    then every face that won a pixel takes the mean of the target pixels it won -- the constant that minimises its squared error under the
    opaque render -- and every other face keeps its old colour.  twin_period = P (faces f and f + P are twins, F = 2 P): the twins' rows
    are added first and both get the same colour (the first twin's old colour where the triangle won nothing), as saveGLB stores it."""
    census = MeshCensus(faces.shape[0], vertices.device)
    for view in views:
        census.add_view(view, vertices, faces, faces_color)
    if twin_period is None:
        return census.mean_color(faces_color)
    color = census.fold_twins(twin_period).mean_color(faces_color[:twin_period])
    return torch.cat([color, color], dim=0)


def visible_triangle_mask(views: Iterable, vertex: torch.Tensor, shs: torch.Tensor, min_pixels: int = 1, save_back: bool = True) -> torch.Tensor:
    """(P,) bool: the triangles of a model (`vertex (P, 3, 3)`, `shs` as mesh_from_triangles takes them) whose face -- or, with `save_back`,
    whose back twin -- wins at least `min_pixels` pixels in the opaque render of the exported mesh, summed over all `views`.  Pixels outside
    a view's `alpha_mask` do not count.  A back twin has the same depth as its front face and ties go to the smaller index, so a twin never
    wins a pixel (see the module text): visibility is decided per triangle, and a kept triangle keeps both faces."""
    vertices, faces, color = mesh_from_triangles(vertex, shs, save_back=save_back)
    census = MeshCensus(faces.shape[0], vertices.device)
    for view in views:
        out = MeshRenderer(view).render(vertices, faces, color)
        alpha = getattr(view, "alpha_mask", None)
        census.add(out["face_idx"], None, alpha.to(device=out["face_idx"].device, dtype=torch.float32) if alpha is not None else None)
    if save_back:
        census = census.fold_twins(vertex.shape[0])
    return census.pixels() >= min_pixels
