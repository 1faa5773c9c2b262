"""The regularisation half of the reference trainer's loss and the model's per-view colour affine, on the HIP kernels of
csrc/regularizers.hip (include/ts_loss.h: tsl_reg_*, tsl_color_affine_*):

    triangle_regularization   w_s scaling_reg + w_o opacity_reg + w_v vertex_reg in one pass + finisher, its gradient in one gather-form pass
                              (src/diff_recon/trainers/VanillaTS_trainer.py:87-97, 107-109; trainer_utils.py:339-346; VanillaTS_model.py:72-76)
    prepare_nearest           the inverse of the nearest relation that the vertex term's backward reads, built once per refresh of the indices
    TrainerRegularizers       the schedule of VanillaTSTrainer._get_loss (:56-70, 86-116) around the two: opacity phases, vertex-term start and
                              nearest-index refresh, affine_reg (:98-105) on the masked-L1 kernels
    ColorAffine               the (V, 3, 3) weight / (V, 3) bias of VanillaTSModel.setup_color_affine (VanillaTS_model.py:86-94) and the affine
                              clamp(pixel @ W[uid] + b[uid], 0, 1) of forward (:678-684), one kernel each way; its two named optimizer groups and
                              their exponential_scheduler (:118-121, 146-152)

No CPU / eager fallback: every call needs float32 tensors on the HIP device.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import torch
from torch import nn

from diff_triangle_rasterization_2D import _C as _native

from .schedulers import exponential_scheduler

_lib = _native._lib

OPACITY_MODES = {"none": 0, "quad": 1, "linear": 2}  # TSL_REG_OPACITY_NONE / _QUAD / _LINEAR


def _f32_cuda(t: torch.Tensor, what: str) -> torch.Tensor:
    _native.require_device(what, t)
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what}: expected scalar type Float")
    return t.contiguous()


def _nearest_u32(nearest: torch.Tensor) -> torch.Tensor:
    """nearestNeighbor's uint32 output (or the reference's .long() copy, trainer_utils.py:336) as contiguous 32-bit words."""
    if nearest.dtype in (torch.uint32, torch.int32):
        return nearest.contiguous()
    if nearest.dtype == torch.int64:
        return nearest.to(torch.int32).contiguous()
    raise RuntimeError("nearest indices must be uint32, int32 or int64")


class PreparedNearest:
    """The inverse of one nearest-index array (include/ts_loss.h: tsl_reg_prepare): for each vertex the vertices whose nearest it is, in ascending
    order.  Built once per refresh of the indices; the vertex term's backward reads it."""

    def __init__(self, nearest: torch.Tensor):
        self.nearest = _nearest_u32(nearest)
        if not self.nearest.is_cuda:
            raise RuntimeError("prepare_nearest (MI355X build) needs the indices on a HIP device; there is no CPU fallback")
        n = self.nearest.numel()
        if n % 3:
            raise ValueError("nearest must hold 3 indices per triangle")
        self.P = n // 3
        with torch.cuda.device(self.nearest.device):
            nbytes = _lib.tsl_reg_prepared_bytes(self.P)
            self.buffer = torch.empty((nbytes,), device=self.nearest.device, dtype=torch.uint8)
            _native._check(_lib.tsl_reg_prepare(self.P, self.nearest.data_ptr(), self.buffer.data_ptr(), nbytes, _native.stream()), "prepare_nearest")


def prepare_nearest(nearest: torch.Tensor) -> PreparedNearest:
    return PreparedNearest(nearest)


class _TriangleReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertex, opacity, nearest, w_s, w_o, mode, w_v, prepared):
        P = vertex.numel() // 9
        dev = vertex.device
        with torch.cuda.device(dev):
            nbytes = _lib.tsl_reg_workspace_bytes()
            ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
            out = torch.empty((4,), device=dev, dtype=torch.float32)
            _native._check(_lib.tsl_reg_forward(P, vertex.data_ptr(), opacity.data_ptr() if opacity is not None else None,
                                                nearest.data_ptr() if nearest is not None else None, w_s, w_o, mode, w_v, ws.data_ptr(), nbytes,
                                                out.data_ptr(), _native.stream()), "triangle_regularization")
        ctx.args = (P, w_s, w_o, mode, w_v, prepared)
        ctx.shapes = (vertex.shape, opacity.shape if opacity is not None else None)
        ctx.save_for_backward(vertex, opacity, nearest)
        parts = out.clone()
        ctx.mark_non_differentiable(parts)
        return out[0].clone(), parts

    @staticmethod
    def backward(ctx, grad_total, _grad_parts):
        vertex, opacity, nearest = ctx.saved_tensors
        P, w_s, w_o, mode, w_v, prepared = ctx.args
        dev = vertex.device
        with torch.cuda.device(dev):
            dv = torch.empty((P, 3, 3), device=dev, dtype=torch.float32)
            do = torch.empty((P, 1), device=dev, dtype=torch.float32)
            go = grad_total.contiguous().to(torch.float32)
            buf = prepared.buffer if prepared is not None else None
            _native._check(_lib.tsl_reg_backward(P, vertex.data_ptr(), opacity.data_ptr() if opacity is not None else None,
                                                 nearest.data_ptr() if nearest is not None else None, buf.data_ptr() if buf is not None else None,
                                                 buf.numel() if buf is not None else 0, w_s, w_o, mode, w_v, go.data_ptr(), dv.data_ptr(),
                                                 do.data_ptr(), _native.stream()), "triangle_regularization backward")
        vshape, oshape = ctx.shapes
        return (dv.view(vshape) if ctx.needs_input_grad[0] else None, do.view(oshape) if ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None)


def triangle_regularization(vertex: torch.Tensor, opacity: Optional[torch.Tensor], nearest: Optional[torch.Tensor], *, w_scaling: float = 0.0,
                            w_opacity: float = 0.0, opacity_mode: str = "none", w_vertex: float = 0.0,
                            prepared: Optional[PreparedNearest] = None):
    """(total, parts): total = w_scaling scaling_reg + w_opacity opacity_reg + w_vertex vertex_reg as a 0-dim tensor (differentiable with respect to
    vertex (P, 3, 3) and opacity (P, 1), the post-sigmoid value), parts = [total, scaling_reg, opacity_reg, vertex_reg] (4 floats, no gradient;
    0 for a term that is off).  opacity_mode: "none", "quad" ((0.25 - (o - 0.5)^2).mean()) or "linear" ((1 - o).mean()).  `nearest`: the (3P,)
    output of nearestNeighbor(vertex.view(-1, 3), 3); `prepared`: prepare_nearest(nearest), built here when the vertex term is on and it is not
    passed.  A term whose weight is 0 is neither computed nor read (nearest may be None when w_vertex == 0)."""
    mode = OPACITY_MODES[opacity_mode] if isinstance(opacity_mode, str) else int(opacity_mode)
    v = _f32_cuda(vertex, "triangle_regularization")
    if v.numel() % 9:
        raise ValueError("vertex must be (P, 3, 3)")
    P = v.numel() // 9
    w_s, w_o, w_v = float(w_scaling), float(w_opacity), float(w_vertex)
    if mode == 0:
        w_o = 0.0
    o = None
    if w_o != 0.0:
        if opacity is None or opacity.numel() != P:
            raise ValueError("opacity must be (P, 1)")
        o = _f32_cuda(opacity, "triangle_regularization")
    n = None
    if w_v != 0.0:
        if nearest is None or nearest.numel() != 3 * P:
            raise ValueError("the vertex term needs nearest indices of the 3P vertices")
        if prepared is None or prepared.P != P:
            prepared = prepare_nearest(nearest)
        n = prepared.nearest  # the prepared inverse and the indices the kernels read are one pair
    else:
        prepared = None
    if o is None and opacity is not None and opacity.requires_grad:
        o = opacity  # an input that takes part in the graph gets its (zero) gradient
    return _TriangleReg.apply(v, o, n, w_s, w_o, mode, w_v, prepared)


# ---- affine_reg = L1(image, image_original), both masked by gt_mask (VanillaTS_trainer.py:98-105) ----------------------------------------
class _AffineL1(torch.autograd.Function):
    """mean |x m - y m| over (3, H, W) on tsl_masked_l1_forward / _backward; dL/dy = -dL/dx exactly (sign(0) = 0 on both sides)."""

    @staticmethod
    def forward(ctx, x, y, mask, ws):
        c, h, w = x.shape
        out = torch.empty((1,), device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _native._check(_lib.tsl_masked_l1_forward(x.data_ptr(), y.data_ptr(), mask.data_ptr(), c, h, w, ws.data_ptr(), ws.numel(), out.data_ptr(),
                                                      _native.stream()), "affine_reg")
        ctx.save_for_backward(x, y, mask)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        x, y, mask = ctx.saved_tensors
        c, h, w = x.shape
        g = torch.empty_like(x)
        go = grad_out.contiguous().to(torch.float32)
        with torch.cuda.device(x.device):
            _native._check(_lib.tsl_masked_l1_backward(x.data_ptr(), y.data_ptr(), mask.data_ptr(), c, h, w, go.data_ptr(), g.data_ptr(), _native.stream()),
                           "affine_reg backward")
        return (g if ctx.needs_input_grad[0] else None), (-g if ctx.needs_input_grad[1] else None), None, None


class AffineReg:
    """affine_reg = L1(image * gt_mask, image_original * gt_mask) (VanillaTS_trainer.py:98-105) for planar (C, H, W) renders, C <= 8.  gt_mask: one
    (H, W) or (1, H, W) plane, or None (a cached all-ones plane).  The masked-L1 workspace and the ones plane are cached per shape."""

    def __init__(self):
        self._cache: Dict[Tuple, Tuple[torch.Tensor, torch.Tensor]] = {}

    def _buffers(self, x: torch.Tensor):
        key = (x.device, tuple(x.shape))
        if key not in self._cache:
            c, h, w = x.shape
            with torch.cuda.device(x.device):
                ws = torch.empty((_lib.tsl_aux_loss_workspace_bytes(c, h, w, 1.0),), device=x.device, dtype=torch.uint8)
            self._cache[key] = (ws, torch.ones((h, w), device=x.device, dtype=torch.float32))
        return self._cache[key]

    def __call__(self, image: torch.Tensor, image_original: torch.Tensor, gt_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        x, y = _f32_cuda(image, "affine_reg"), _f32_cuda(image_original, "affine_reg")
        if x.dim() != 3 or x.shape != y.shape or x.size(0) > 8:
            raise ValueError("affine_reg takes two (C, H, W) images of one shape, C <= 8")
        ws, ones = self._buffers(x)
        if gt_mask is None:
            mask = ones
        else:
            mask = _f32_cuda(gt_mask.detach(), "affine_reg")
            if mask.numel() != x.size(1) * x.size(2):
                raise ValueError("gt_mask must be one (H, W) plane")
        return _AffineL1.apply(x, y, mask, ws)


affine_reg = AffineReg()


# ---- per-view colour affine (VanillaTS_model.py:86-94, 118-121, 146-152, 678-684) ---------------------------------------------------------
class _ColorAffine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, weight, bias, uid):
        _, h, w = image.shape
        out = torch.empty_like(image)
        with torch.cuda.device(image.device):
            _native._check(_lib.tsl_color_affine_forward(image.data_ptr(), h, w, weight[uid].data_ptr(), bias[uid].data_ptr(), out.data_ptr(),
                                                         _native.stream()), "ColorAffine")
        ctx.uid = uid
        ctx.save_for_backward(image, weight, bias)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        image, weight, bias = ctx.saved_tensors
        uid = ctx.uid
        _, h, w = image.shape
        dev = image.device
        with torch.cuda.device(dev):
            g = grad_out.contiguous()
            gx = torch.empty_like(image)
            gw = torch.zeros_like(weight)  # torch's indexing backward: dense zeros for the other views
            gb = torch.zeros_like(bias)
            nbytes = _lib.tsl_reg_workspace_bytes()
            ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
            _native._check(_lib.tsl_color_affine_backward(image.data_ptr(), h, w, weight[uid].data_ptr(), bias[uid].data_ptr(), g.data_ptr(),
                                                          ws.data_ptr(), nbytes, gx.data_ptr(), gw[uid].data_ptr(), gb[uid].data_ptr(), _native.stream()),
                           "ColorAffine backward")
        return (gx if ctx.needs_input_grad[0] else None), (gw if ctx.needs_input_grad[1] else None), (gb if ctx.needs_input_grad[2] else None), None


class ColorAffine(nn.Module):
    """Per-view colour affine: `weight` (V, 3, 3) initialised to the identity and `bias` (V, 3) to zeros (VanillaTS_model.py:86-94);
    forward(image, uid) = clamp(image.permute(1, 2, 0) @ weight[uid] + bias[uid], 0, 1).permute(2, 0, 1) for a planar (3, H, W) image
    (:678-684), one kernel each way.  Its optimizer groups are named "color_affine_weight" / "color_affine_bias" (:118-121) and share one
    exponential_scheduler (:146-152): see param_groups() and lr_schedulers()."""

    def __init__(self, view_count: int, device=None):
        super().__init__()
        w = torch.zeros((view_count, 3, 3), dtype=torch.float32, device=device)
        w[:, 0, 0] = w[:, 1, 1] = w[:, 2, 2] = 1.0
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros((view_count, 3), dtype=torch.float32, device=device))

    def forward(self, image: torch.Tensor, uid: int) -> torch.Tensor:
        x = _f32_cuda(image, "ColorAffine")
        if x.dim() != 3 or x.size(0) != 3:
            raise ValueError("ColorAffine takes a planar (3, H, W) image")
        uid = int(uid)
        if not 0 <= uid < self.weight.size(0):
            raise IndexError(f"view uid {uid} out of range for {self.weight.size(0)} views")
        if not self.weight.is_contiguous() or not self.bias.is_contiguous():
            raise RuntimeError("ColorAffine parameters must be contiguous")
        return _ColorAffine.apply(x, self.weight, self.bias, uid)

    def param_groups(self, lr: float = 0.0):
        """The two named groups of VanillaTS_model.py:118-121, for FusedAdam / torch.optim.Adam."""
        return [{"params": [self.weight], "lr": lr, "name": "color_affine_weight"},
                {"params": [self.bias], "lr": lr, "name": "color_affine_bias"}]

    @staticmethod
    def lr_schedulers(**color_affine) -> Dict[str, Callable[[int], float]]:
        """{"color_affine_weight": s, "color_affine_bias": s}, s = exponential_scheduler(**config.optimizer.color_affine) (:146-152)."""
        return {"color_affine_weight": exponential_scheduler(**color_affine), "color_affine_bias": exponential_scheduler(**color_affine)}


# ---- the schedule of VanillaTSTrainer._get_loss ------------------------------------------------------------------------------------------
def _field(cfg, name, default=None):
    if cfg is None:
        return default
    v = cfg.get(name, default) if isinstance(cfg, dict) else getattr(cfg, name, default)
    return default if v is None else v


class TrainerRegularizers:
    """reg_loss of VanillaTSTrainer._get_loss (VanillaTS_trainer.py:56-70, 86-116) for one iteration:

        reg_loss = w_scaling_reg scaling_reg + w_o_reg opacity_reg + w_affine_reg affine_reg + w_v_reg vertex_reg

    built from the trainer config's w_scaling_reg, w_opacity_reg.{quad_reg, linear_reg, quad_start_iter, linear_start_iter},
    vertex_reg.{w_vertex_reg, start_iter, interval_iter} and w_affine_reg (attributes or dict keys; TrainerRegularizers(config.trainer)).
    The schedule is the reference's:
      * opacity: no term while iteration <= quad_start_iter, the quadratic one while iteration <= linear_start_iter, the linear one after;
      * vertex: weight 0 until iteration > start_iter; while it is on, the nearest indices (nearestNeighbor(vertex.view(-1, 3), 3)) and their
        prepared inverse are refreshed when (iteration - 1) % interval_iter == 0 or the cache is empty -- and, a deliberate addition, when the
        triangle count P has changed since the cache was built (densification / pruning between refreshes; the reference's nearest_dist2 would
        fail its size assert there);
      * affine_reg only when render_pkg holds "render_original" (ColorAffine through render_view(..., color_affine=...)).
    __call__(iteration, render_pkg, gt_mask=None) returns reg_loss (a 0-dim tensor, or 0.0 when every active weight is 0: then nothing is
    launched) and sets render_pkg["vertex_loss"] (vertex_reg, 0 while the term is off).  The native calls can be injected (nearest_fn,
    prepare_fn, reg_fn, affine_fn) -- the CPU tests drive the schedule with stand-ins."""

    def __init__(self, config=None, *, w_scaling_reg: Optional[float] = None, w_opacity_reg=None, vertex_reg=None, w_affine_reg: Optional[float] = None,
                 nearest_fn: Optional[Callable] = None, prepare_fn: Optional[Callable] = None, reg_fn: Optional[Callable] = None,
                 affine_fn: Optional[Callable] = None):
        self.w_scaling_reg = float(w_scaling_reg if w_scaling_reg is not None else _field(config, "w_scaling_reg", 0.0))
        o = w_opacity_reg if w_opacity_reg is not None else _field(config, "w_opacity_reg")
        self.quad_reg, self.linear_reg = float(_field(o, "quad_reg", 0.0)), float(_field(o, "linear_reg", 0.0))
        self.quad_start_iter, self.linear_start_iter = int(_field(o, "quad_start_iter", 0)), int(_field(o, "linear_start_iter", 0))
        v = vertex_reg if vertex_reg is not None else _field(config, "vertex_reg")
        self.w_vertex_reg = float(_field(v, "w_vertex_reg", 0.0))
        self.vertex_start_iter, self.vertex_interval_iter = int(_field(v, "start_iter", 0)), int(_field(v, "interval_iter", 1))
        self.w_affine_reg = float(w_affine_reg if w_affine_reg is not None else _field(config, "w_affine_reg", 0.0))
        if nearest_fn is None:
            from simple_knn import nearestNeighbor as nearest_fn
        self._nearest_fn = nearest_fn
        self._prepare_fn = prepare_fn or prepare_nearest
        self._reg_fn = reg_fn or triangle_regularization
        self._affine_fn = affine_fn or AffineReg()
        self._nearest = None  # the reference's _nearest_indices_cache
        self._prepared = None
        self._nearest_P = -1

    def opacity_term(self, iteration: int) -> Tuple[str, float]:
        """(mode, weight) at `iteration` (VanillaTS_trainer.py:89-97)."""
        if iteration <= self.quad_start_iter:
            return "none", 0.0
        if iteration <= self.linear_start_iter:
            return "quad", self.quad_reg
        return "linear", self.linear_reg

    def vertex_weight(self, iteration: int) -> float:
        return self.w_vertex_reg if iteration > self.vertex_start_iter else 0.0  # :62

    def __call__(self, iteration: int, render_pkg: dict, gt_mask: Optional[torch.Tensor] = None):
        vertex, opacity = render_pkg["vertex"], render_pkg["opacity"]
        mode, w_o = self.opacity_term(iteration)
        w_v = self.vertex_weight(iteration)
        P = vertex.numel() // 9
        if w_v > 0 and ((iteration - 1) % self.vertex_interval_iter == 0 or self._nearest is None or self._nearest_P != P):  # :107-108
            self._nearest = self._nearest_fn(vertex.detach().reshape(-1, 3), 3)
            self._prepared = self._prepare_fn(self._nearest)
            self._nearest_P = P
        reg_loss = 0.0
        render_pkg["vertex_loss"] = 0
        if self.w_scaling_reg != 0.0 or w_o != 0.0 or w_v != 0.0:
            total, parts = self._reg_fn(vertex, opacity, self._nearest if w_v != 0.0 else None, w_scaling=self.w_scaling_reg, w_opacity=w_o,
                                        opacity_mode=mode, w_vertex=w_v, prepared=self._prepared if w_v != 0.0 else None)
            reg_loss = total
            if w_v != 0.0:
                render_pkg["vertex_loss"] = parts[3]
        if self.w_affine_reg != 0.0 and "render_original" in render_pkg:  # :99-105
            reg_loss = reg_loss + self.w_affine_reg * self._affine_fn(render_pkg["render"], render_pkg["render_original"], gt_mask)
        return reg_loss
