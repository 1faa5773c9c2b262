"""`_C` of the drop-in `diff_triangle_rasterization_2D` package: the two entry points the reference exports
through pybind (R2D/ext.cpp:6-8), here the torch extension bindings/_ts2d_torch_C.so (bindings/ts2d_torch_ext.cpp) over the C ABI
of libts2d.so (include/ts2d.h); the rest of that ABI is bound with ctypes.

    rasterize_triangles(image_width, image_height, tan_fovx, tan_fovy, viewmatrix, projmatrix, campos,
                        sh_degree, gamma, scale_modifier, background_depth, background, vertex, shs, feature,
                        opacity, back_culling, rich_info, debug)
        -> (num_rendered, out_feature, radii, depth, normal, contrib_sum, contrib_max,
            geometryBuffer, binningBuffer, imageBuffer)          # R2D/src/extension_interface.cu:19-152
    rasterize_triangles_backward(tan_fovx, tan_fovy, viewmatrix, projmatrix, campos, sh_degree, gamma,
                        scale_modifier, background_depth, background, vertex, shs, feature, opacity,
                        num_rendered, radii, geometryBuffer, binningBuffer, imageBuffer, dL_dout_feature,
                        dL_dout_depth, dL_dout_normal, rich_info, debug)
        -> (dL_dvertex, dL_dcenter2D, dL_dshs, dL_dfeature, dL_dopacity)   # extension_interface.cu:154-260

Same positional signatures, same argument checks and RuntimeErrors, same ownership (the callee allocates every
output on vertex.device; the three uint8 buffers are opaque).  torch is used only for device memory (caching
allocator) and the current stream.  There is NO CPU or eager fallback: if libts2d.so or the extension is missing or the
tensors are not on a HIP device, this module raises.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts2d.so")
# Measurement / triage only (tools/, tests/triage/, the lab-library tests): a statistics or lab build of the same C ABI
# (tools/bin/libts2d_stats.so, tools/bin/libts2d_lab.so) can be loaded in place of the product library.  The product library
# itself reads no environment variable.
_LIB_PATH = os.environ.get("TS2D_LIBRARY_PATH") or _LIB_PATH

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The MI355X rasterizer has no CPU fallback."
    )
_lib = C.CDLL(_LIB_PATH)

# The two hot entry points go through the compiled extension: through ctypes, their argument marshalling and ~15 torch allocations from Python cost
# 0.3-0.4 ms of host time per forward + backward, what bounds every scene below ~100 k triangles (profiles/r06_binding.txt).
# The extension needs libts2d.so by name.  Every library build.py links carries that soname, so the dynamic loader meets the need with the library
# loaded above -- the product's or the one TS2D_LIBRARY_PATH names -- and both bindings call one instance of it.
_EXT_PATH = os.path.join(os.path.dirname(_HERE), "bindings", "_ts2d_torch_C.so")
try:
    _spec = importlib.util.spec_from_file_location("_ts2d_torch_C", _EXT_PATH)
    _ext = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(_ext)
except (ImportError, OSError) as _e:
    raise ImportError(f"{_EXT_PATH} could not be loaded ({_e}): build it with `python triangle-splatting_amd/build.py`") from _e
if C.cast(C.CDLL("libts2d.so", mode=os.RTLD_NOLOAD).ts2d_version, C.c_void_p).value != C.cast(_lib.ts2d_version, C.c_void_p).value:
    raise ImportError(f"{_LIB_PATH} lacks the soname libts2d.so, so the extension would call another copy of the library: rebuild it with "
                      "`python triangle-splatting_amd/build.py`")


FLAG_BACK_CULLING, FLAG_RICH_INFO, FLAG_DEBUG, FLAG_USE_SHS, FLAG_3D, FLAG_SH_FACTORED = 1, 2, 4, 8, 16, 32

# Every struct mirror and every function signature of the C ABI is declared once, in _abi.py; the names stay importable from here.
from ._abi import _BackwardOut, _Camera, _ForwardOut, _Geometry, _LossGrads, _State, bind  # noqa: E402,F401

bind(_lib)


def set_capacity_hint_key(key: int) -> None:
    """Names the stream of views the calling thread's next forwards belong to (ts2d_set_capacity_hint_key): the speculative forward sizes its
    binning buffer from the history of (device, variant, image size, key).  Train and evaluation cameras of one size, or two models in one
    process, should use different keys; the default is 0."""
    _lib.ts2d_set_capacity_hint_key(int(key) & 0xFFFFFFFFFFFFFFFF)


def speculative_overflows() -> int:
    """How many speculative forwards of this process guessed too small a binning buffer and rendered a second time (ts2d.h)."""
    return int(_lib.ts2d_speculative_overflow_count())


def version() -> str:
    return _lib.ts2d_version().decode()


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.ts2d_last_error().decode()} (ts2d error {rc})")


def _ptr(t):
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def stream() -> int:
    """The current stream of the current device, as the `void *stream` of the C ABI."""
    return torch.cuda.current_stream().cuda_stream


def require_device(what: str, *tensors, verb: str = "needs"):
    """There is no CPU or eager fallback anywhere in the package: component `what` refuses tensors that are not on a HIP device."""
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{what} (MI355X build) {verb} tensors on a HIP device; there is no CPU fallback")


def _contiguous_or_raise(*tensors):
    # extension_interface.cu:77-81, 193-199
    for t in tensors:
        if t is not None and not t.is_contiguous():
            raise RuntimeError("input tensors must be contiguous")


def _f32_or_raise(*tensors):
    for t in tensors:
        if t is not None and t.numel() > 0 and t.dtype != torch.float32:
            raise RuntimeError("expected scalar type Float")  # what data_ptr<float>() raises in the reference


def rasterize_triangles(image_width, image_height, tan_fovx, tan_fovy, viewmatrix, projmatrix, campos, sh_degree, gamma,
                        scale_modifier, background_depth, background, vertex, shs, feature, opacity, back_culling,
                        rich_info, debug, *, variant=2, instance_capacity=None):
    """`variant=3` selects the 3D rasterizer (TS2D_FLAG_3D; used by the sibling package diff_triangle_rasterization_3D).
    `instance_capacity` (an int > 0) selects the SYNC-FREE forward (ts2d_forward): the binning state is sized for that many tile
    instances, nothing is read back, and the returned `num_rendered` is the capacity (it only sizes the state for the backward
    call); whether the true count fitted is reported by `forward_status`.  Default None = the reference's sequence with its one
    blocking read of num_rendered.
    `background_depth`: a float like the reference's binding takes, or a one-element float32 tensor on the device (what the reference's
    model computes every step, VanillaTS_model.py:623), handed to the kernels as a pointer: no device synchronisation for the conversion."""
    bg_t = background_depth if isinstance(background_depth, torch.Tensor) else None
    return _ext.rasterize_triangles_ex(int(image_width), int(image_height), tan_fovx, tan_fovy, viewmatrix, projmatrix, campos, int(sh_degree), gamma,
                                       scale_modifier, 0.0 if bg_t is not None else float(background_depth), background, vertex, shs, feature, opacity,
                                       bool(back_culling), bool(rich_info), bool(debug), int(variant),
                                       int(instance_capacity) if (instance_capacity is not None and vertex.size(0) > 0) else 0, bg_t)


def rasterize_triangles_backward(tan_fovx, tan_fovy, viewmatrix, projmatrix, campos, sh_degree, gamma, scale_modifier,
                                 background_depth, background, vertex, shs, feature, opacity, num_rendered, radii,
                                 geometryBuffer, binningBuffer, imageBuffer, dL_dout_feature, dL_dout_depth,
                                 dL_dout_normal, rich_info, debug, *, variant=2, sh_factored=False, out=None, range_events=None):
    """`sh_factored=True` (SH mode only; TS2D_FLAG_SH_FACTORED): dL_dshs is not formed (returned as None) and the fourth
    result holds the clamp-masked colour gradient dL_dRGB (P, 3) for `sh_grad_expand` -- see parallel.py.
    `out`: optional dict of preallocated contiguous float32 device tensors ("vertex" (P,3,3), "center2D" (P,2), "opacity" (P,1),
    "color" = dL_dshs (P,M,3) or dL_dfeature (P,C)) that the library writes instead of fresh allocations (parallel.GradBucket).
    `range_events`: a list of K torch.cuda.Event (each recorded at least once before): the per-triangle kernel runs as K launches over
    consecutive triangle ranges of `backward_range_rows(P, K)` rows and event k is recorded behind range k (ts2d_backward_ranged)."""
    bg_t = background_depth if isinstance(background_depth, torch.Tensor) else None
    o = out or {}
    return _ext.rasterize_triangles_backward_ex(tan_fovx, tan_fovy, viewmatrix, projmatrix, campos, int(sh_degree), gamma, scale_modifier,
                                                0.0 if bg_t is not None else float(background_depth), background, vertex, shs, feature, opacity,
                                                int(num_rendered), radii, geometryBuffer, binningBuffer, imageBuffer, dL_dout_feature, dL_dout_depth,
                                                dL_dout_normal, bool(rich_info), bool(debug), int(variant), bool(sh_factored), o.get("vertex"),
                                                o.get("center2D"), o.get("color"), o.get("opacity"), bg_t,
                                                [int(e.cuda_event) for e in range_events] if range_events else [])


def backward_range_rows(P: int, num_ranges: int) -> int:
    """Rows per triangle range of a ranged backward (ts2d_backward_range_rows): ceil(P / K) rounded up to a multiple of 64."""
    return int(_lib.ts2d_backward_range_rows(int(P), int(num_ranges)))


def forward_status(P, W, H, geometryBuffer, imageBuffer):
    """(overflowed, num_rendered) of the last sync-free forward on these state buffers (ts2d_forward_status; one blocking read)."""
    st = _State(_ptr(geometryBuffer), geometryBuffer.numel(), None, 0, _ptr(imageBuffer), imageBuffer.numel())
    over, n = C.c_int32(0), C.c_int64(0)
    with torch.cuda.device(imageBuffer.device):
        _check(_lib.ts2d_forward_status(C.byref(st), int(P), int(W), int(H), C.byref(over), C.byref(n), stream()),
               "forward_status")
    return bool(over.value), int(n.value)


def sh_grad_expand(vertex, campos, dL_dcolor, sh_degree, M, out=None):
    """dL_dshs (P, M, 3) = sum over views v of basis(normalize(centroid - campos[v])) x dL_dcolor[v]  (ts2d_sh_grad_expand).
    vertex (P,3,3), campos (V,3), dL_dcolor (V,P,3): contiguous float32 on one HIP device."""
    require_device("diff_triangle_rasterization_2D", vertex)
    _contiguous_or_raise(vertex, campos, dL_dcolor, out)
    _f32_or_raise(vertex, campos, dL_dcolor, out)
    P, V = vertex.size(0), campos.size(0)
    if dL_dcolor.shape != (V, P, 3):
        raise RuntimeError("dL_dcolor must have dimensions (num_views, num_points, 3)")
    with torch.cuda.device(vertex.device):
        if out is None:
            out = (torch.zeros if P == 0 else torch.empty)((P, int(M), 3), device=vertex.device, dtype=torch.float32)
        _check(_lib.ts2d_sh_grad_expand(P, int(sh_degree), int(M), V, _ptr(vertex), _ptr(campos), _ptr(dL_dcolor), _ptr(out), stream()),
               "sh_grad_expand")
    return out


# ---- timing hooks used by bench.py (not part of the reference's surface) ----------------------------------------
def profile_enable(on: bool):
    _lib.ts2d_profile_enable(1 if on else 0)


def profile_only(name: str = ""):
    _lib.ts2d_profile_only(name.encode() if name else None)


def profile_reset():
    _lib.ts2d_profile_reset()


def profile_read():
    rows, i = [], 0
    name = C.create_string_buffer(64)
    ms, n = C.c_double(0), C.c_int64(0)
    while _lib.ts2d_profile_read(i, name, 64, C.byref(ms), C.byref(n)) == 0:
        rows.append((name.value.decode(), ms.value, n.value))
        i += 1
    return rows
