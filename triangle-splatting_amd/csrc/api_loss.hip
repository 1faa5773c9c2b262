// api_loss.hip -- the C ABI of include/ts_loss.h: argument checks in front of the loss, regulariser and resampling launchers.
#pragma GCC visibility push(default)
#include "../../include/ts_loss.h"
#pragma GCC visibility pop
#include "ts2d_api.h"

namespace
{
int loss_args_ok(const float *image, const float *gt, int32_t C, int32_t H, int32_t W, const void *ws, size_t ws_bytes)
{
    if (C <= 0 || H <= 0 || W <= 0) return ts_fail(TS2D_ERR_INVALID, "image dimensions must be positive");
    if (C > 65535 || (H + 15) / 16 > 65535) return ts_fail(TS2D_ERR_INVALID, "image too large");
    if (!image || !gt) return ts_fail(TS2D_ERR_INVALID, "null image");
    if (!ws || ws_bytes < ts_loss_workspace_bytes(C, H, W)) return ts_fail(TS2D_ERR_CAPACITY, "loss workspace too small");
    return TS2D_OK;
}
int depth_normal_args_ok(const float *depth, const float *normal, int32_t H, int32_t W, float tan_fovx, float tan_fovy, double scale,
                         const void *ws, size_t ws_bytes)
{
    if (H <= 0 || W <= 0) return ts_fail(TS2D_ERR_INVALID, "height and width must be positive");
    if ((int64_t)H * W > (int64_t)16 * 1000 * 1000) return ts_fail(TS2D_ERR_INVALID, "quantile() input tensor is too large"); // torch.quantile's own limit
    if (!(tan_fovx > 0.0f) || !(tan_fovy > 0.0f)) return ts_fail(TS2D_ERR_INVALID, "tan_fovx / tan_fovy must be positive");
    if (scale > 0.0 && scale != 1.0 && ((int)floor((double)H * scale) < 1 || (int)floor((double)W * scale) < 1))
        return ts_fail(TS2D_ERR_INVALID, "scale_factor leaves no pixel");
    if (!depth || !normal || !ws) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (ws_bytes < ts_depth_normal_workspace_bytes(H, W, scale)) return ts_fail(TS2D_ERR_CAPACITY, "workspace too small");
    return TS2D_OK;
}
int downsample_args_ok(const void *a, const void *b, int32_t C, int32_t H, int32_t W, int32_t h, int32_t w)
{
    if (C <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return ts_fail(TS2D_ERR_INVALID, "dimensions must be positive");
    if (H % h != 0 || W % w != 0 || H / h < 2 || W / w < 2) return ts_fail(TS2D_ERR_INVALID, "the down-sampler takes integer factors >= 2 (H = f h, W = g w)");
    if (!a || !b) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    return TS2D_OK;
}
int downsample_planes_ok(int32_t n, const float *const *a, float *const *b, int32_t H, int32_t W, int32_t h, int32_t w)
{
    if (n < 0) return ts_fail(TS2D_ERR_INVALID, "num_planes must be >= 0");
    if (n == 0) return TS2D_OK;
    if (!a || !b) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    for (int k = 0; k < n; k++)
        if (int rc = downsample_args_ok(a[k], b[k], 1, H, W, h, w)) return rc;
    return TS2D_OK;
}
int aux_args_ok(int32_t C, int32_t H, int32_t W, double scale, const void *ws, size_t ws_bytes, bool need_ws)
{
    if (C <= 0 || C > 8) return ts_fail(TS2D_ERR_INVALID, "channels must be in 1..8");
    if (H <= 0 || W <= 0) return ts_fail(TS2D_ERR_INVALID, "height and width must be positive");
    if ((int64_t)H * W > (int64_t)16 * 1000 * 1000) return ts_fail(TS2D_ERR_INVALID, "quantile() input tensor is too large");
    if (scale > 0.0 && scale != 1.0 && ((int)floor((double)H * scale) < 1 || (int)floor((double)W * scale) < 1))
        return ts_fail(TS2D_ERR_INVALID, "scale_factor leaves no pixel");
    if (need_ws && (!ws || ws_bytes < ts_aux_loss_workspace_bytes(C, H, W, scale))) return ts_fail(TS2D_ERR_CAPACITY, "workspace too small");
    return TS2D_OK;
}
int reg_args_ok(int32_t P, int32_t mode)
{
    if (P < 0 || P > (1 << TS_ID_BITS)) return ts_fail(TS2D_ERR_INVALID, "P must be in 0..2^28");
    if (mode != TSL_REG_OPACITY_NONE && mode != TSL_REG_OPACITY_QUAD && mode != TSL_REG_OPACITY_LINEAR)
        return ts_fail(TS2D_ERR_INVALID, "opacity_mode must be TSL_REG_OPACITY_NONE, _QUAD or _LINEAR");
    return TS2D_OK;
}
int affine_args_ok(int32_t H, int32_t W)
{
    if (H <= 0 || W <= 0) return ts_fail(TS2D_ERR_INVALID, "height and width must be positive");
    if ((int64_t)H * W > ((int64_t)1 << 28)) return ts_fail(TS2D_ERR_INVALID, "image too large");
    return TS2D_OK;
}
} // namespace

extern "C" {
size_t tsl_workspace_bytes(int32_t channels, int32_t height, int32_t width) { return ts_loss_workspace_bytes(channels, height, width); }

int tsl_photometric_forward(const float *image, const float *gt, int32_t channels, int32_t height, int32_t width, float w_l1,
                            float w_ssim, int32_t need_grad, void *workspace, size_t workspace_bytes, float *out, void *stream)
{
    if (int rc = loss_args_ok(image, gt, channels, height, width, workspace, workspace_bytes)) return rc;
    if (!out) return ts_fail(TS2D_ERR_INVALID, "null output");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("photometric_fwd", s);
    TS_HIP(ts_loss_forward(image, gt, channels, height, width, w_l1, w_ssim, need_grad != 0, workspace, out, s));
    return TS2D_OK;
}

int tsl_photometric_backward(const float *image, const float *gt, int32_t channels, int32_t height, int32_t width, float w_l1,
                             float w_ssim, const void *workspace, size_t workspace_bytes, const float *grad_out, float *dL_dimage,
                             void *stream)
{
    if (int rc = loss_args_ok(image, gt, channels, height, width, workspace, workspace_bytes)) return rc;
    if (!dL_dimage) return ts_fail(TS2D_ERR_INVALID, "null output");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("photometric_bwd", s);
    TS_HIP(ts_loss_backward(image, gt, channels, height, width, w_l1, w_ssim, workspace, grad_out, dL_dimage, s));
    return TS2D_OK;
}

size_t tsl_depth_normal_workspace_bytes(int32_t height, int32_t width, double scale_factor)
{
    return ts_depth_normal_workspace_bytes(height, width, scale_factor);
}

int tsl_depth_normal_forward(const float *depth, const float *normal, int32_t height, int32_t width, float tan_fovx, float tan_fovy,
                             double scale_factor, float quantile, void *workspace, size_t workspace_bytes, float *out, void *stream)
{
    if (int rc = depth_normal_args_ok(depth, normal, height, width, tan_fovx, tan_fovy, scale_factor, workspace, workspace_bytes)) return rc;
    if (!out) return ts_fail(TS2D_ERR_INVALID, "null output");
    if (!(quantile >= 0.0f && quantile <= 1.0f)) return ts_fail(TS2D_ERR_INVALID, "quantile() q values must be in the range [0, 1]");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("depth_normal_fwd", s);
    TS_HIP(ts_depth_normal_forward(depth, normal, height, width, tan_fovx, tan_fovy, scale_factor, quantile, workspace, out, s));
    return TS2D_OK;
}

int tsl_depth_normal_backward(const float *depth, const float *normal, int32_t height, int32_t width, float tan_fovx, float tan_fovy,
                              double scale_factor, const void *workspace, size_t workspace_bytes, const float *grad_out, float *dL_ddepth,
                              float *dL_dnormal, void *stream)
{
    if (int rc = depth_normal_args_ok(depth, normal, height, width, tan_fovx, tan_fovy, scale_factor, workspace, workspace_bytes)) return rc;
    if (!dL_ddepth && !dL_dnormal) return TS2D_OK;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("depth_normal_bwd", s);
    TS_HIP(ts_depth_normal_backward(depth, normal, height, width, tan_fovx, tan_fovy, scale_factor, workspace, grad_out, dL_ddepth, dL_dnormal, s));
    return TS2D_OK;
}

// ---- the down-sampler of render_up_scale (resample.hip) ----------------------------------------------------------------------------
int tsl_downsample_forward(const float *in, int32_t C, int32_t H, int32_t W, int32_t h, int32_t w, float *out, void *stream)
{
    if (int rc = downsample_args_ok(in, out, C, H, W, h, w)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("downsample_fwd", s);
    TS_HIP(ts_downsample_forward(in, C, H, W, h, w, out, s));
    return TS2D_OK;
}
int tsl_downsample_backward(const float *grad_out, int32_t C, int32_t H, int32_t W, int32_t h, int32_t w, float *grad_in, void *stream)
{
    if (int rc = downsample_args_ok(grad_out, grad_in, C, H, W, h, w)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("downsample_bwd", s);
    TS_HIP(ts_downsample_backward(grad_out, C, H, W, h, w, grad_in, s));
    return TS2D_OK;
}

int tsl_downsample_forward_planes(int32_t n, const float *const *in_planes, int32_t H, int32_t W, int32_t h, int32_t w, float *const *out_planes, void *stream)
{
    if (int rc = downsample_planes_ok(n, in_planes, out_planes, H, W, h, w)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("downsample_fwd", s);
    TS_HIP(ts_downsample_forward_planes(n, in_planes, H, W, h, w, out_planes, s));
    return TS2D_OK;
}
int tsl_downsample_backward_planes(int32_t n, const float *const *grad_out_planes, int32_t H, int32_t W, int32_t h, int32_t w, float *const *grad_in_planes,
                                   void *stream)
{
    if (int rc = downsample_planes_ok(n, grad_out_planes, grad_in_planes, H, W, h, w)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("downsample_bwd", s);
    TS_HIP(ts_downsample_backward_planes(n, grad_out_planes, H, W, h, w, grad_in_planes, s));
    return TS2D_OK;
}

// ---- DoGLoss / SmoothnessLoss (aux_losses.hip) ------------------------------------------------------------------------------------
size_t tsl_aux_loss_workspace_bytes(int32_t channels, int32_t height, int32_t width, double scale_factor)
{
    return ts_aux_loss_workspace_bytes(channels, height, width, scale_factor);
}
int tsl_dog_mask(const float *gt, int32_t C, int32_t H, int32_t W, double sigma1, int32_t ksize1, double sigma2, int32_t ksize2, int32_t invert,
                 double scale_factor, void *workspace, size_t workspace_bytes, float *mask, void *stream)
{
    if (int rc = aux_args_ok(C, H, W, scale_factor, workspace, workspace_bytes, true)) return rc;
    if (!gt || !mask) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (!(sigma1 > 0.0) || !(sigma2 > 0.0) || ksize1 < 1 || ksize2 < ksize1 || ksize2 > 33 || !(ksize1 & 1) || !(ksize2 & 1))
        return ts_fail(TS2D_ERR_INVALID, "need 0 < sigma, odd kernel sizes with ksize1 <= ksize2 <= 33");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("dog_mask", s);
    TS_HIP(ts_dog_mask(gt, C, H, W, sigma1, ksize1, sigma2, ksize2, invert, scale_factor, workspace, mask, s));
    return TS2D_OK;
}
int tsl_smoothness_mask(const float *gt, int32_t C, int32_t H, int32_t W, double scale_factor, float quantile, void *workspace, size_t workspace_bytes,
                        float *mask, void *stream)
{
    if (int rc = aux_args_ok(C, H, W, scale_factor, workspace, workspace_bytes, true)) return rc;
    if (!gt || !mask) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (!(quantile >= 0.0f && quantile <= 1.0f)) return ts_fail(TS2D_ERR_INVALID, "quantile() q values must be in the range [0, 1]");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("smoothness_mask", s);
    TS_HIP(ts_smoothness_mask(gt, C, H, W, scale_factor, quantile, workspace, mask, s));
    return TS2D_OK;
}
int tsl_masked_l1_forward(const float *image, const float *gt, const float *mask, int32_t C, int32_t H, int32_t W, void *workspace, size_t workspace_bytes,
                          float *out, void *stream)
{
    if (int rc = aux_args_ok(C, H, W, 1.0, workspace, workspace_bytes, true)) return rc;
    if (!image || !gt || !mask || !out) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("masked_l1_fwd", s);
    TS_HIP(ts_masked_l1_forward(image, gt, mask, C, H, W, workspace, out, s));
    return TS2D_OK;
}
int tsl_masked_l1_backward(const float *image, const float *gt, const float *mask, int32_t C, int32_t H, int32_t W, const float *grad_out,
                           float *dL_dimage, void *stream)
{
    if (int rc = aux_args_ok(C, H, W, 1.0, nullptr, 0, false)) return rc;
    if (!image || !gt || !mask || !dL_dimage) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("masked_l1_bwd", s);
    TS_HIP(ts_masked_l1_backward(image, gt, mask, C, H, W, grad_out, dL_dimage, s));
    return TS2D_OK;
}
int tsl_scharr_smoothness_forward(const float *image, const float *mask, int32_t C, int32_t H, int32_t W, void *workspace, size_t workspace_bytes,
                                  float *out, void *stream)
{
    if (int rc = aux_args_ok(C, H, W, 1.0, workspace, workspace_bytes, true)) return rc;
    if (!image || !mask || !out) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("smoothness_fwd", s);
    TS_HIP(ts_scharr_smoothness_forward(image, mask, C, H, W, workspace, out, s));
    return TS2D_OK;
}
int tsl_scharr_smoothness_backward(const float *image, const float *mask, int32_t C, int32_t H, int32_t W, void *workspace, size_t workspace_bytes,
                                   const float *grad_out, float *dL_dimage, void *stream)
{
    if (int rc = aux_args_ok(C, H, W, 1.0, workspace, workspace_bytes, true)) return rc;
    if (!image || !mask || !dL_dimage) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("smoothness_bwd", s);
    TS_HIP(ts_scharr_smoothness_backward(image, mask, C, H, W, workspace, grad_out, dL_dimage, s));
    return TS2D_OK;
}

// ---- the trainer's regularisers + per-view colour affine (regularizers.hip) ------------------------------------------------------
size_t tsl_reg_workspace_bytes(void) { return ts_reg_workspace_bytes(); }
size_t tsl_reg_prepared_bytes(int32_t P) { return ts_reg_prepared_bytes(P); }
int tsl_reg_prepare(int32_t P, const uint32_t *nearest, void *prepared, size_t prepared_bytes, void *stream)
{
    if (int rc = reg_args_ok(P, TSL_REG_OPACITY_NONE)) return rc;
    if (P == 0) return TS2D_OK;
    if (!nearest) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (!prepared || prepared_bytes < ts_reg_prepared_bytes(P)) return ts_fail(TS2D_ERR_CAPACITY, "prepared buffer too small");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("reg_prepare", s);
    TS_HIP(ts_reg_prepare(P, nearest, prepared, s));
    return TS2D_OK;
}
int tsl_reg_forward(int32_t P, const float *vertex, const float *opacity, const uint32_t *nearest, float w_scaling, float w_opacity,
                    int32_t opacity_mode, float w_vertex, void *workspace, size_t workspace_bytes, float *out, void *stream)
{
    if (int rc = reg_args_ok(P, opacity_mode)) return rc;
    if (!out || (P > 0 && (w_scaling != 0.0f || w_vertex != 0.0f) && !vertex)) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (P > 0 && w_opacity != 0.0f && opacity_mode != TSL_REG_OPACITY_NONE && !opacity) return ts_fail(TS2D_ERR_INVALID, "null opacity");
    if (P > 0 && w_vertex != 0.0f && !nearest) return ts_fail(TS2D_ERR_INVALID, "w_vertex != 0 needs the nearest indices");
    if (!workspace || workspace_bytes < ts_reg_workspace_bytes()) return ts_fail(TS2D_ERR_CAPACITY, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("reg_fwd", s);
    TS_HIP(ts_reg_forward(P, vertex, opacity, nearest, w_scaling, w_opacity, opacity_mode, w_vertex, workspace, out, s));
    return TS2D_OK;
}
int tsl_reg_backward(int32_t P, const float *vertex, const float *opacity, const uint32_t *nearest, const void *prepared, size_t prepared_bytes,
                     float w_scaling, float w_opacity, int32_t opacity_mode, float w_vertex, const float *grad_out, float *dL_dvertex,
                     float *dL_dopacity, void *stream)
{
    if (int rc = reg_args_ok(P, opacity_mode)) return rc;
    if (P == 0) return TS2D_OK;
    if (!vertex || !dL_dvertex || !dL_dopacity) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (w_opacity != 0.0f && opacity_mode != TSL_REG_OPACITY_NONE && !opacity) return ts_fail(TS2D_ERR_INVALID, "null opacity");
    if (w_vertex != 0.0f && !nearest) return ts_fail(TS2D_ERR_INVALID, "w_vertex != 0 needs the nearest indices");
    if (w_vertex != 0.0f && (!prepared || prepared_bytes < ts_reg_prepared_bytes(P)))
        return ts_fail(TS2D_ERR_CAPACITY, "w_vertex != 0 needs the buffer tsl_reg_prepare filled for these P");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("reg_bwd", s);
    TS_HIP(ts_reg_backward(P, vertex, opacity, nearest, prepared, w_scaling, w_opacity, opacity_mode, w_vertex, grad_out, dL_dvertex, dL_dopacity, s));
    return TS2D_OK;
}
int tsl_color_affine_forward(const float *image, int32_t H, int32_t W, const float *weight, const float *bias, float *out, void *stream)
{
    if (int rc = affine_args_ok(H, W)) return rc;
    if (!image || !weight || !bias || !out) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("color_affine_fwd", s);
    TS_HIP(ts_color_affine_forward(image, H, W, weight, bias, out, s));
    return TS2D_OK;
}
int tsl_color_affine_backward(const float *image, int32_t H, int32_t W, const float *weight, const float *bias, const float *grad_out, void *workspace,
                              size_t workspace_bytes, float *dL_dimage, float *dL_dweight, float *dL_dbias, void *stream)
{
    if (int rc = affine_args_ok(H, W)) return rc;
    if (!image || !weight || !bias || !grad_out || !dL_dimage || !dL_dweight || !dL_dbias) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (!workspace || workspace_bytes < ts_reg_workspace_bytes()) return ts_fail(TS2D_ERR_CAPACITY, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("color_affine_bwd", s);
    TS_HIP(ts_color_affine_backward(image, H, W, weight, bias, grad_out, workspace, dL_dimage, dL_dweight, dL_dbias, s));
    return TS2D_OK;
}
} // extern "C"
