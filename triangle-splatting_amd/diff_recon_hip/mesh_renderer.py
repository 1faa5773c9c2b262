"""`MeshRenderer`: the reference's `KaolinRenderer` (src/diff_recon/renderer/kaolin_renderer.py:8-72) on the MI355X -- the opaque,
per-pixel depth-tested look at the triangle soup that `saveGLB` exports, which the reference renders through Kaolin's CUDA-only
`nvdiffrast_fwd` backend.  Same constructor, same `render` signature, same `render` / `mask` results plus `depth` and `face_idx`.

Native code: libts2d.so (include/ts_mesh.h: csrc/mesh_preprocess.hip, the rasterizer's ordering chain, csrc/mesh_resolve.hip), bound
with ctypes like simple_knn and losses.py.  Forward only, like the backend it replaces.  No CPU / eager fallback.

`mesh_from_triangles` builds, on the device, the mesh `saveGLB` would write for a model (raw_triangle.py:189-198 of the reference), so
that a trained model can be rendered and scored without a file round trip."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from diff_triangle_rasterization_2D import _C as _native

from .raw_triangle import C0, _accessor, read_glb

_lib = _native._lib


def mesh_from_triangles(vertex: torch.Tensor, shs: torch.Tensor, save_back: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(vertices (3P, 3) f32, faces (F, 3) int32, faces_color (F, 3) f32) of the mesh `RawTriangle.saveGLB` writes for the triangles
    `vertex (P, 3, 3)` with SH coefficients `shs` ((P, K, 3) as the model holds them, or (P, 3 K) as RawTriangle does; the DC triple
    first): un-shared vertices, one colour per face = clip(SH2RGB(f_dc), 0, 1), and with `save_back` the back faces as reversed twins
    behind the front faces (F = 2 P).  Stays on `vertex.device`."""
    P = vertex.shape[0]
    if vertex.shape != (P, 3, 3):
        raise ValueError("vertex must have dimensions (num_triangles, 3, 3)")
    f_dc = shs[:, 0, :] if shs.dim() == 3 else shs[:, :3]
    if f_dc.shape != (P, 3):
        raise ValueError("shs must have dimensions (num_triangles, K, 3) or (num_triangles, 3 K)")
    vertices = vertex.detach().to(torch.float32).reshape(P * 3, 3).contiguous()
    color = (f_dc.detach().to(torch.float32) * C0 + 0.5).clamp(0.0, 1.0)
    faces = torch.arange(3 * P, device=vertex.device, dtype=torch.int32).reshape(P, 3)
    if save_back:
        faces = torch.cat([faces, faces.flip(1)], dim=0)
        color = torch.cat([color, color], dim=0)
    return vertices, faces.contiguous(), color.contiguous()


def load_glb_mesh(path, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(vertices, faces, faces_color) of the first primitive of a GLB file as `saveGLB` writes it: POSITION, the index buffer, and the colour
    of each face's first vertex (the file stores a face's colour on its three un-shared vertices)."""
    import numpy as np
    doc, binary = read_glb(path)
    mesh = next((m for m in doc["meshes"] if m.get("name") == "geometry_0"), doc["meshes"][0])
    prim = mesh["primitives"][0]
    if prim.get("mode", 4) != 4:
        raise NotImplementedError(f"{path}: only triangle lists (glTF mode 4) are supported")
    pos = _accessor(doc, binary, prim["attributes"]["POSITION"]).astype(np.float32)
    if "indices" in prim:
        idx = _accessor(doc, binary, prim["indices"]).astype(np.int64).reshape(-1, 3)
    else:
        idx = np.arange(len(pos), dtype=np.int64).reshape(-1, 3)
    if "COLOR_0" in prim["attributes"]:
        col = _accessor(doc, binary, prim["attributes"]["COLOR_0"])
        scale = {5121: 255.0, 5123: 65535.0}.get(doc["accessors"][prim["attributes"]["COLOR_0"]]["componentType"], 1.0)
        face_rgb = (col[:, :3].astype(np.float64) / scale)[idx[:, 0]].astype(np.float32) if len(idx) else np.zeros((0, 3), np.float32)
    else:
        face_rgb = np.ones((len(idx), 3), np.float32)
    return (torch.from_numpy(np.ascontiguousarray(pos)).to(device), torch.from_numpy(idx.astype(np.int32)).to(device),
            torch.from_numpy(np.ascontiguousarray(face_rgb)).to(device))


class MeshRenderer:
    """Opaque z-buffer rendering of a triangle mesh with one colour per face.

    `cam` is duck-typed as in triangle_renderer.py: `image_width`, `image_height`, `tan_fovx`, `tan_fovy`, `world_view_transform` (the
    reference's row-vector convention), `device`, and `znear` (1.0 when the attribute is missing).

    A face is drawn iff its three vertices have view-space depth > znear (kaolin_renderer.py:51; no clipping, no back-face culling).  A
    pixel is covered by a face when its centre (i + 0.5, j + 0.5) lies inside or on the projected triangle; the nearest covering face
    wins, ties go to the smaller face index, so the result is a pure function of the inputs (bit-identical from run to run).
    Coverage and depth do not depend on the order in which a face names its vertices (its record is built in ascending index order), so
    a reversed back twin of a face ties with it on every pixel and never wins one.
    The depth of a face at a pixel is the ray / plane intersection in view space (perspective-correct).  Whether Kaolin's backend
    interpolates z this way or linearly in screen space could not be checked (the library is not installable on this platform);
    `render` and `mask` depend on that choice only where triangles interpenetrate.

    render(...) -> {"render": (3, H, W) the winner's colour, else bg_color, clamped to [0, 1]; "mask": (1, H, W) 1.0 / 0.0;
                    "depth": (H, W), 0 where uncovered; "face_idx": (H, W) int32, -1 where uncovered}
    """

    def __init__(self, cam, bg_color: torch.Tensor = torch.Tensor([0, 0, 0])):
        self.cam = cam
        self.bg_color = bg_color.to(cam.device)
        self._geometry: Dict[int, torch.Tensor] = {}  # state buffers, reused between calls: geometry per F ...
        self._image: Dict[Tuple[int, int], torch.Tensor] = {}  # ... image per (W, H) ...
        self._binning: Optional[torch.Tensor] = None  # ... and one binning buffer that only grows
        self.last_num_rendered = 0  # (tile, face) instances of the last render
        self.wave_visits: Optional[torch.Tensor] = None  # measurement (tools/bench_mesh.py): a one-element int64 device tensor that every render adds
        #                                                  the (wavefront, face) pairs its depth test walked to (ts2d_mesh_render_counted)

    def _state(self, F: int, W: int, H: int, device):
        g = self._geometry.get(F)
        if g is None or g.device != device:
            self._geometry.clear()
            g = self._geometry[F] = torch.empty((_lib.ts2d_mesh_geometry_state_bytes(F),), device=device, dtype=torch.uint8)
        im = self._image.get((W, H))
        if im is None or im.device != device:
            self._image.clear()
            im = self._image[(W, H)] = torch.empty((_lib.ts2d_image_state_bytes(W, H),), device=device, dtype=torch.uint8)
        return g, im

    def render(self, vertices: torch.Tensor = None, faces: torch.Tensor = None, faces_color: torch.Tensor = None,
               mesh_path: str = None) -> Dict[str, torch.Tensor]:
        cam = self.cam
        device = torch.device(cam.device)
        if mesh_path is not None:
            if not str(mesh_path).lower().endswith(".glb"):
                raise NotImplementedError(f"{mesh_path}: only GLB files (RawTriangle.saveGLB) can be read here; the reference reads other "
                                          "formats through trimesh, which is not a dependency -- pass vertices, faces and faces_color instead")
            vertices, faces, faces_color = load_glb_mesh(mesh_path, device)
        elif vertices is None or faces is None or faces_color is None:
            raise ValueError("Either mesh_path or vertices, faces, and faces_color must be provided")
        if device.type != "cuda" or not vertices.is_cuda:
            raise RuntimeError("MeshRenderer (MI355X build) needs the camera and the mesh on a HIP device; there is no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if vertices.dim() != 2 or vertices.size(1) != 3:
            raise RuntimeError("vertices must have dimensions (num_vertices, 3)")
        if faces.dim() != 2 or faces.size(1) != 3 or faces.dtype not in (torch.int32, torch.int64):
            raise RuntimeError("faces must be an int32 or int64 tensor with dimensions (num_faces, 3)")
        if faces_color.shape != (faces.size(0), 3):
            raise RuntimeError("faces_color must have dimensions (num_faces, 3)")
        W, H = int(cam.image_width), int(cam.image_height)
        V, F = vertices.size(0), faces.size(0)
        znear = float(getattr(cam, "znear", 1.0))
        with torch.cuda.device(device):
            vertices = vertices.detach().to(device=device, dtype=torch.float32).contiguous()
            faces = faces.to(device=device, dtype=torch.int32).contiguous()
            faces_color = faces_color.detach().to(device=device, dtype=torch.float32).contiguous()
            view = cam.world_view_transform.to(device=device, dtype=torch.float32).contiguous()
            bg = self.bg_color.to(device=device, dtype=torch.float32).contiguous()
            gbuf, ibuf = self._state(F, W, H, device)
            stream = _native.stream()
            ccam = _native._Camera(W, H, float(cam.tan_fovx), float(cam.tan_fovy), view.data_ptr(), None, None)
            bbuf = self._binning if (self._binning is not None and self._binning.device == device) else None
            st = _native._State(gbuf.data_ptr(), gbuf.numel(), _native._ptr(bbuf), 0 if bbuf is None else bbuf.numel(), ibuf.data_ptr(), ibuf.numel())
            n = C.c_int64(0)
            _native._check(_lib.ts2d_mesh_bin(C.byref(ccam), znear, V, _native._ptr(vertices), F, _native._ptr(faces), C.byref(st), C.byref(n), stream),
                           "MeshRenderer.render (bin)")
            N = int(n.value)
            need = _lib.ts2d_binning_state_bytes(N, W, H)
            if bbuf is None or bbuf.numel() < need:
                bbuf = self._binning = torch.empty((need + need // 4,), device=device, dtype=torch.uint8)
                st.binning, st.binning_bytes = bbuf.data_ptr(), bbuf.numel()
            render = torch.empty((3, H, W), device=device, dtype=torch.float32)
            mask = torch.empty((1, H, W), device=device, dtype=torch.float32)
            depth = torch.empty((H, W), device=device, dtype=torch.float32)
            face_idx = torch.empty((H, W), device=device, dtype=torch.int32)
            _native._check(_lib.ts2d_mesh_render_counted(C.byref(ccam), F, _native._ptr(faces_color), bg.data_ptr(), N, C.byref(st), render.data_ptr(),
                                                         mask.data_ptr(), depth.data_ptr(), face_idx.data_ptr(), _native._ptr(self.wave_visits), stream),
                           "MeshRenderer.render")
            self.last_num_rendered = N
        return {"render": render, "mask": mask, "depth": depth, "face_idx": face_idx}
