"""A texture atlas for an indexed mesh, baked from views: colour resolution that does not depend on the face count.

    atlas_layout(num_faces, res, cells_per_row=None)               AtlasLayout: res x res half-cells, two faces to a cell of (res + 1) x res texels
    face_uvs(layout, num_faces)                                    (F, 3, 2) float32, glTF's convention (origin top-left), exact under NEAREST
    texel_index(cam, vertices, faces, face_idx, layout, ...)       (H, W) int32: the compact texel of every pixel, -1 where nothing is drawn
    TextureAtlas(num_faces, res, device)                           a MeshCensus over num_faces * T texels
        .add(cam, vertices, faces, face_idx, target, pixel_mask)   one view into the state (nothing is read back)
        .add_view(view, vertices, faces)                           MeshRenderer's face_idx of the view, its gt_image under its alpha_mask
        .face_totals()                                             (F, 4) int64: the sums of every face's texels
        a += b                                                     the states of two atlases add
        .resolve(min_count=1, face_fallback=None, fill=0.5)        BakedTexture(image, rgb8, state, uv, layout)
    render_textured(cam, vertices, faces, baked, bg_color)         render_vertex_colors' dictionary, the colours read from the atlas
    bake_texture(views, vertices, faces, res, ...)                 one TextureAtlas over all views, resolved
    evaluate_textured(views, vertices, faces, baked)               PSNR / SSIM of that render against each view's gt_image (metrics.py)
    save_glb_textured_mesh(path, vertices, faces, baked)           a glTF 2.0 binary with TEXCOORD_0 and the atlas as an embedded PNG

Every step is a pure function of its inputs (include/ts_atlas.h): the texel of a pixel follows from the barycentrics of
interpolate_vertex_attributes (one source: csrc/ts_mesh_bary.h), the sums are MeshCensus' integers, so the state is bit-identical in any view
order and atlases add.  With res == 1 a texel is a face and the bake is bake_face_colors.  A texel that fewer than min_count pixels saw
takes the mean of its face, then the caller's per-face fallback, then `fill`; `state` says which (3, 2, 1, 0).  The atlas has no gutters: it
is exact under a NEAREST sampler, and a bilinear one mixes neighbouring faces along every edge.

Native code: libts_atlas.so beside this file (include/ts_atlas.h, csrc/mesh_atlas.hip), a twelfth library because the export lists of the
other eleven are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import struct
import zlib
from pathlib import Path
from typing import Dict, Iterable, NamedTuple, Optional

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_atlas

from .mesh_census import MeshCensus
from .mesh_renderer import MeshRenderer

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_atlas.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The texture atlas kernels have no CPU fallback."
    )
_lib = bind_atlas(C.CDLL(_LIB_PATH))

MAX_RES = 64  # TSA_MAX_RES
INT32_MAX = 2 ** 31 - 1


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsa_last_error().decode()} (ts2d error {rc})")


def _cuda_device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the texture atlas (MI355X build) lives on a HIP device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


class AtlasLayout(NamedTuple):
    res: int              # R: texels per face edge
    texels_per_face: int  # T = R (R + 1) / 2
    cells_per_row: int    # Cx
    cells_per_col: int    # Cy = max(1, ceil(K / Cx)), K = ceil(F / 2)
    width: int            # Wa = Cx (R + 1)
    height: int           # Ha = Cy R


class BakedTexture(NamedTuple):
    image: torch.Tensor   # (3, Ha, Wa) float32
    rgb8: torch.Tensor    # (Ha, Wa, 3) uint8: the image clamped to [0, 1] in 8 bits, as save_glb_textured_mesh stores it
    state: torch.Tensor   # (Ha, Wa) uint8: 3 the texel's own mean, 2 its face's mean, 1 face_fallback, 0 fill
    uv: torch.Tensor      # (F, 3, 2) float32
    layout: AtlasLayout


def atlas_layout(num_faces: int, res: int, cells_per_row: Optional[int] = None) -> AtlasLayout:
    """The atlas of `num_faces` faces with `res` texels per face edge.  cells_per_row defaults to the smallest Cx >= 1 with
    Cx Cx (R + 1) >= K R, a near-square image.  ValueError: num_faces < 0, res outside [1, 64], cells_per_row < 1, or more than 2^31 - 1
    texels (num_faces * T, or width * height)."""
    F, R = int(num_faces), int(res)
    if F < 0:
        raise ValueError("num_faces must be >= 0")
    if not 1 <= R <= MAX_RES:
        raise ValueError(f"res must lie in [1, {MAX_RES}], got {R}")
    T = R * (R + 1) // 2
    if F * T > INT32_MAX:
        raise ValueError(f"{F} faces of {T} texels exceed 2^31 - 1 texels")
    K = (F + 1) // 2
    if cells_per_row is None:
        Cx = max(1, math.isqrt(K * R // (R + 1)))
        while Cx * Cx * (R + 1) < K * R:
            Cx += 1
        while Cx > 1 and (Cx - 1) * (Cx - 1) * (R + 1) >= K * R:
            Cx -= 1
    else:
        Cx = int(cells_per_row)
        if Cx < 1:
            raise ValueError("cells_per_row must be >= 1")
    Cy = max(1, -(-K // Cx))
    Wa, Ha = Cx * (R + 1), Cy * R
    if Wa * Ha > INT32_MAX:
        raise ValueError(f"an atlas of {Wa} x {Ha} texels exceeds 2^31 - 1")
    return AtlasLayout(R, T, Cx, Cy, Wa, Ha)


def face_uvs(layout: AtlasLayout, num_faces: int, device=None) -> torch.Tensor:
    """(F, 3, 2) float32: the atlas position of every face's corners (a, b, c) over (width, height), origin top-left.  Integers and float64,
    rounded once to float32: floor(uv * size) of an interior point of a face is its texel."""
    import numpy as np
    F, R = int(num_faces), layout.res
    if F < 0 or (F + 1) // 2 > layout.cells_per_row * layout.cells_per_col:
        raise ValueError(f"the layout holds {2 * layout.cells_per_row * layout.cells_per_col} faces, not {F}")
    f = np.arange(F, dtype=np.int64)
    k, upper = f // 2, (f % 2 == 1)[:, None]
    X0, Y0 = ((k % layout.cells_per_row) * (R + 1))[:, None], ((k // layout.cells_per_row) * R)[:, None]
    x = np.where(upper, X0 + np.array([R + 1, 1, R + 1]), X0 + np.array([0, R, 0]))
    y = np.where(upper, Y0 + np.array([R, R, 0]), Y0 + np.array([0, 0, R]))
    uv = np.stack([x.astype(np.float64) / float(layout.width), y.astype(np.float64) / float(layout.height)], axis=-1).astype(np.float32)
    out = torch.from_numpy(np.ascontiguousarray(uv.reshape(F, 3, 2)))
    return out if device is None else out.to(device)


def _mesh_args(vertices: torch.Tensor, faces: torch.Tensor, device):
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError("vertices must have dimensions (num_vertices, 3)")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("faces must have dimensions (num_faces, 3)")
    return (vertices.detach().to(device=device, dtype=torch.float32).contiguous(), faces.to(device=device, dtype=torch.int32).contiguous())


def texel_index(cam, vertices: torch.Tensor, faces: torch.Tensor, face_idx: torch.Tensor, layout: AtlasLayout, return_atlas_idx: bool = False,
                return_bary: bool = False):
    """(H, W) int32: the compact texel index f T + j R - j (j - 1) / 2 + i of every pixel whose face_idx (H, W) int32 names a face of `faces`
    (F, 3) with indices inside `vertices` (V, 3), -1 elsewhere.  return_atlas_idx: also (H, W) int32, y * width + x of that texel in the
    atlas; return_bary: also (3, H, W) float32, interpolate_vertex_attributes' weights.  `cam` is duck-typed as for MeshRenderer."""
    W, H = int(cam.image_width), int(cam.image_height)
    device = _cuda_device(vertices.device)
    vertices, faces = _mesh_args(vertices, faces, device)
    if face_idx.numel() != H * W:
        raise RuntimeError(f"face_idx must have dimensions ({H}, {W})")
    if (faces.shape[0] + 1) // 2 > layout.cells_per_row * layout.cells_per_col:
        raise ValueError(f"the layout holds {2 * layout.cells_per_row * layout.cells_per_col} faces, not {faces.shape[0]}")
    with torch.cuda.device(device):
        face_idx = face_idx.to(device=device, dtype=torch.int32).contiguous()
        view = cam.world_view_transform.detach().to(device=device, dtype=torch.float32).contiguous()
        texel = torch.empty((H, W), device=device, dtype=torch.int32)
        atlas = torch.empty((H, W), device=device, dtype=torch.int32) if return_atlas_idx else None
        bary = torch.empty((3, H, W), device=device, dtype=torch.float32) if return_bary else None
        _check(_lib.tsa_texel_index(view.data_ptr(), float(cam.tan_fovx), float(cam.tan_fovy), W, H, vertices.shape[0], _native._ptr(vertices),
                                    faces.shape[0], _native._ptr(faces), face_idx.data_ptr(), layout.res, layout.cells_per_row, texel.data_ptr(),
                                    _native._ptr(atlas), _native._ptr(bary), _native.stream()), "texel_index")
    extra = tuple(x for x in (atlas, bary) if x is not None)
    return (texel, *extra) if extra else texel


class TextureAtlas:
    """The texel accumulator of a mesh of `num_faces` faces with `res` texels per face edge: a MeshCensus of num_faces * T rows
    {count, sum_r, sum_g, sum_b} (`census`, its tensor `texels`), 64-bit integers, zero at the start."""

    def __init__(self, num_faces: int, res: int, device, cells_per_row: Optional[int] = None):
        self.layout = atlas_layout(num_faces, res, cells_per_row)
        self.num_faces = int(num_faces)
        self.census = MeshCensus(self.num_faces * self.layout.texels_per_face, device)

    @property
    def texels(self) -> torch.Tensor:
        return self.census.acc

    def add(self, cam, vertices: torch.Tensor, faces: torch.Tensor, face_idx: torch.Tensor, target: Optional[torch.Tensor] = None,
            pixel_mask: Optional[torch.Tensor] = None) -> "TextureAtlas":
        """Adds one view on the current stream: texel_index of face_idx, then MeshCensus.add with the texel as the key."""
        if faces.shape[0] != self.num_faces:
            raise ValueError(f"the atlas was made for {self.num_faces} faces, not {faces.shape[0]}")
        self.census.add(texel_index(cam, vertices, faces, face_idx, self.layout), target, pixel_mask)
        return self

    def add_view(self, view, vertices: torch.Tensor, faces: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Renders the mesh with MeshRenderer(view) and adds the result with `view.gt_image` as the target, under `view.alpha_mask` when the
        view has one, as MeshCensus.add_view does.  Returns the render dict."""
        grey = torch.full((faces.shape[0], 3), 0.5, device=vertices.device, dtype=torch.float32)
        out = MeshRenderer(view).render(vertices, faces, grey)
        device = out["face_idx"].device
        alpha = getattr(view, "alpha_mask", None)
        self.add(view, vertices, faces, out["face_idx"], view.gt_image.to(device=device, dtype=torch.float32),
                 alpha.to(device=device, dtype=torch.float32) if alpha is not None else None)
        return out

    def face_totals(self) -> torch.Tensor:
        """(F, 4) int64: the integer sum of every face's T rows; at res == 1 the state itself."""
        device = _cuda_device(self.texels.device)
        with torch.cuda.device(device):
            out = torch.empty((self.num_faces, 4), device=device, dtype=torch.int64)
            _check(_lib.tsa_face_totals(self.num_faces, self.layout.res, _native._ptr(self.texels) if self.num_faces else None,
                                        _native._ptr(out) if self.num_faces else None, _native.stream()), "TextureAtlas.face_totals")
        return out

    def __iadd__(self, other: "TextureAtlas") -> "TextureAtlas":
        if not isinstance(other, TextureAtlas):
            return NotImplemented
        if (other.num_faces, other.layout.res) != (self.num_faces, self.layout.res):
            raise ValueError("only atlases of the same face count and resolution add")
        self.census.acc += other.census.acc.to(self.census.acc.device)
        return self

    def resolve(self, min_count: int = 1, face_fallback: Optional[torch.Tensor] = None, fill=0.5) -> BakedTexture:
        """The atlas image.  A texel that at least min_count pixels saw takes their mean; otherwise the mean of its face, where any pixel
        saw it; otherwise its row of face_fallback (F, 3) when given; otherwise `fill` (one value or three), as do the cells without a face."""
        if int(min_count) < 1:
            raise ValueError("min_count must be >= 1")
        if face_fallback is not None and tuple(face_fallback.shape) != (self.num_faces, 3):
            raise ValueError("face_fallback must have dimensions (num_faces, 3)")
        fill3 = [float(fill)] * 3 if isinstance(fill, (int, float)) else [float(x) for x in fill]
        if len(fill3) != 3:
            raise ValueError("fill must be one value or three")
        device = _cuda_device(self.texels.device)
        lay, F = self.layout, self.num_faces
        with torch.cuda.device(device):
            totals = self.face_totals()
            if face_fallback is not None:
                face_fallback = face_fallback.detach().to(device=device, dtype=torch.float32).contiguous()
            image = torch.empty((3, lay.height, lay.width), device=device, dtype=torch.float32)
            state = torch.empty((lay.height, lay.width), device=device, dtype=torch.uint8)
            rgb8 = torch.empty((lay.height, lay.width, 3), device=device, dtype=torch.uint8)
            _check(_lib.tsa_resolve(F, lay.res, lay.cells_per_row, lay.cells_per_col, _native._ptr(self.texels) if F else None,
                                    _native._ptr(totals) if F else None, int(min_count), _native._ptr(face_fallback) if F else None,
                                    (C.c_float * 3)(*fill3), image.data_ptr(), state.data_ptr(), rgb8.data_ptr(), _native.stream()),
                   "TextureAtlas.resolve")
        return BakedTexture(image, rgb8, state, face_uvs(lay, F, device), lay)


def render_textured(cam, vertices: torch.Tensor, faces: torch.Tensor, baked: BakedTexture,
                    bg_color: torch.Tensor = torch.Tensor([0, 0, 0])) -> Dict[str, torch.Tensor]:
    """render_vertex_colors' dictionary for a mesh with a baked atlas: coverage, `mask`, `depth` and `face_idx` are MeshRenderer's; `render`
    (3, H, W) is the atlas texel of every drawn pixel (a NEAREST lookup, by index), bg_color elsewhere, clamped to [0, 1]."""
    W, H = int(cam.image_width), int(cam.image_height)
    flat = torch.zeros((faces.shape[0], 3), device=vertices.device, dtype=torch.float32)
    out = MeshRenderer(cam, bg_color).render(vertices=vertices, faces=faces, faces_color=flat)
    _, atlas = texel_index(cam, vertices, faces, out["face_idx"], baked.layout, return_atlas_idx=True)
    device = atlas.device
    with torch.cuda.device(device):
        image = baked.image.detach().to(device=device, dtype=torch.float32).contiguous()
        if tuple(image.shape) != (3, baked.layout.height, baked.layout.width):
            raise RuntimeError("baked.image does not have the dimensions of baked.layout")
        background = bg_color.detach().to(device=device, dtype=torch.float32).contiguous()
        if background.numel() != 3:
            raise RuntimeError("bg_color must have 3 values")
        render = torch.empty((3, H, W), device=device, dtype=torch.float32)
        _check(_lib.tsa_render(W, H, baked.layout.width, baked.layout.height, atlas.data_ptr(), image.data_ptr(), background.data_ptr(),
                               render.data_ptr(), _native.stream()), "render_textured")
    return {"render": render.clamp_(0.0, 1.0), "mask": out["mask"], "depth": out["depth"], "face_idx": out["face_idx"]}


def bake_texture(views: Iterable, vertices: torch.Tensor, faces: torch.Tensor, res: int, min_count: int = 1,
                 face_fallback: Optional[torch.Tensor] = None, fill=0.5, cells_per_row: Optional[int] = None) -> BakedTexture:
    """One TextureAtlas over all `views` (cameras with `gt_image`, optionally `alpha_mask`, as evaluate_mesh takes them), resolved."""
    atlas = TextureAtlas(faces.shape[0], res, _cuda_device(vertices.device), cells_per_row)
    for view in views:
        atlas.add_view(view, vertices, faces)
    return atlas.resolve(min_count, face_fallback, fill)


def evaluate_textured(views: Iterable, vertices: torch.Tensor, faces: torch.Tensor, baked: BakedTexture,
                      bg_color: torch.Tensor = torch.Tensor([0, 0, 0])) -> Dict[str, object]:
    """evaluate_mesh for a mesh with a baked atlas, drawn by render_textured: the same loop, the same keys."""
    from .metrics import psnr, ssim
    psnrs, ssims = [], []
    for view in views:
        image = render_textured(view, vertices, faces, baked, bg_color)["render"]
        gt = view.gt_image.to(image.device)
        alpha = getattr(view, "alpha_mask", None)
        psnrs.append(float(psnr(image, gt, alpha.to(image.device) if alpha is not None else None).item()))
        ssims.append(float(ssim(image, gt.contiguous()).item()))
    n = len(psnrs)
    return {"psnr": psnrs, "ssim": ssims, "mean_psnr": sum(psnrs) / n if n else float("nan"), "mean_ssim": sum(ssims) / n if n else float("nan")}


def encode_png(rgb8) -> bytes:
    """A PNG file of an (H, W, 3) uint8 image: colour type 2, 8 bits, every row with filter 0, one IDAT chunk."""
    import numpy as np
    a = np.ascontiguousarray(rgb8.detach().cpu().numpy() if isinstance(rgb8, torch.Tensor) else rgb8)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("rgb8 must be a uint8 array with dimensions (H, W, 3), H, W >= 1")
    H, W = a.shape[:2]
    rows = np.concatenate([np.zeros((H, 1), np.uint8), a.reshape(H, 3 * W)], axis=1)  # the filter byte of every row: 0

    def chunk(kind: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 9))
            + chunk(b"IEND", b""))


def save_glb_textured_mesh(path, vertices, faces, baked: BakedTexture) -> None:
    """Writes the mesh (vertices (V, 3), faces (F, 3); tensors or arrays) with its atlas as a glTF 2.0 binary in the container of
    save_glb_mesh: 3 F un-shared vertices (a vertex has one UV per face) with POSITION and TEXCOORD_0 float32, uint32 indices, and one
    material whose baseColorTexture is baked.rgb8 as a PNG inside the BIN chunk, sampled NEAREST and clamped to the edge.
    diff_recon_hip.mesh_renderer.load_glb_mesh reads the geometry back."""
    import numpy as np
    host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    v = np.ascontiguousarray(host(vertices), dtype="<f4").reshape(-1, 3)
    f = host(faces).astype(np.int64).reshape(-1, 3)
    uv = np.ascontiguousarray(host(baked.uv), dtype="<f4").reshape(-1, 2)
    if len(uv) != 3 * len(f):
        raise ValueError("baked.uv must have one row per face")
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("faces name vertices that do not exist")
    pos = np.ascontiguousarray(v[f.reshape(-1)])
    idx = np.arange(3 * len(f), dtype="<u4")
    png = encode_png(baked.rgb8)
    blobs, views, off = [], [], 0
    for raw, target in ((pos.tobytes(), 34962), (uv.tobytes(), 34962), (idx.tobytes(), 34963), (png, None)):
        views.append({"buffer": 0, "byteOffset": off, "byteLength": len(raw), **({"target": target} if target else {})})
        raw += b"\x00" * (-len(raw) % 4)
        blobs.append(raw)
        off += len(raw)
    doc = {
        "asset": {"version": "2.0", "generator": "diff_recon_hip.mesh_texture"},
        "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"name": "geometry_0", "mesh": 0}],
        "meshes": [{"name": "geometry_0", "primitives": [{"attributes": {"POSITION": 0, "TEXCOORD_0": 1}, "indices": 2, "material": 0, "mode": 4}]}],
        "materials": [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 1.0}}],
        "textures": [{"sampler": 0, "source": 0}],
        "samplers": [{"magFilter": 9728, "minFilter": 9728, "wrapS": 33071, "wrapT": 33071}],
        "images": [{"bufferView": 3, "mimeType": "image/png"}],
        "buffers": [{"byteLength": off}], "bufferViews": views,
        "accessors": [
            {"bufferView": 0, "componentType": 5126, "count": int(len(pos)), "type": "VEC3",
             "min": [float(x) for x in (pos.min(axis=0) if len(pos) else np.zeros(3))], "max": [float(x) for x in (pos.max(axis=0) if len(pos) else np.zeros(3))]},
            {"bufferView": 1, "componentType": 5126, "count": int(len(uv)), "type": "VEC2"},
            {"bufferView": 2, "componentType": 5125, "count": int(len(idx)), "type": "SCALAR"},
        ],
    }
    js = json.dumps(doc, separators=(",", ":")).encode("utf-8")
    js += b" " * (-len(js) % 4)
    binary = b"".join(blobs)
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(js) + 8 + len(binary)))
        fh.write(struct.pack("<I4s", len(js), b"JSON") + js)
        fh.write(struct.pack("<I4s", len(binary), b"BIN\x00") + binary)


__all__ = ["AtlasLayout", "BakedTexture", "TextureAtlas", "atlas_layout", "face_uvs", "texel_index", "render_textured", "bake_texture",
           "evaluate_textured", "encode_png", "save_glb_textured_mesh"]
