// api_model.hip -- the C ABI of include/ts_model.h, include/ts_optim.h and include/ts_knn.h: argument checks in front of the model-update,
// optimiser and nearest-neighbour launchers.
#pragma GCC visibility push(default)
#include "../../include/ts_model.h"
#include "../../include/ts_optim.h"
#include "../../include/ts_knn.h"
#pragma GCC visibility pop
#include "ts2d_api.h"

namespace
{
int rows_ok(int64_t rows, int32_t row_bytes, const void *a, const void *b, const void *c)
{
    if (rows < 0 || row_bytes <= 0 || (row_bytes & 3)) return ts_fail(TS2D_ERR_INVALID, "rows must be >= 0 and row_bytes a positive multiple of 4");
    if (rows > 0 && (!a || !b || !c)) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    return TS2D_OK;
}
} // namespace

extern "C" {
// ---- include/ts_model.h -----------------------------------------------------------------------------------------------
int tsm_training_statistic(int32_t P, int32_t num_views, const int32_t *radii, const float *center2D_grad, const float *contrib_sum,
                           const float *contrib_max, float *gradient_accum, float *gradient_denom, float *max_radii2D,
                           float *contrib_sum_state, float *contrib_max_state, float *contrib_denom, void *stream)
{
    if (P < 0 || num_views < 0) return ts_fail(TS2D_ERR_INVALID, "P / num_views must be >= 0");
    if (P == 0 || num_views == 0) return TS2D_OK;
    if (!radii || !center2D_grad || !gradient_accum || !gradient_denom || !max_radii2D || !contrib_denom)
        return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if ((contrib_sum == nullptr) != (contrib_max == nullptr)) return ts_fail(TS2D_ERR_INVALID, "contrib_sum and contrib_max go together");
    if (contrib_sum && (!contrib_sum_state || !contrib_max_state)) return ts_fail(TS2D_ERR_INVALID, "null contribution state");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("training_statistic", s);
    TS_HIP(ts_model_training_statistic(P, num_views, radii, center2D_grad, contrib_sum, contrib_max, gradient_accum, gradient_denom,
                                       max_radii2D, contrib_sum_state, contrib_max_state, contrib_denom, s));
    return TS2D_OK;
}

size_t tsm_select_scratch_bytes(int32_t P) { return ts_model_select_scratch_bytes(P); }

int tsm_select_rows(int32_t P, const uint8_t *mask, int32_t match, uint32_t *pos, void *scratch, size_t scratch_bytes, uint32_t *count,
                    void *stream)
{
    if (P < 0 || !count) return ts_fail(TS2D_ERR_INVALID, "P must be >= 0 and count non-null");
    *count = 0;
    if (P == 0) return TS2D_OK;
    if (!mask || !pos) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (!scratch || scratch_bytes < ts_model_select_scratch_bytes(P)) return ts_fail(TS2D_ERR_CAPACITY, "select scratch too small");
    TS_HIP(ts_model_select_rows(P, mask, match, pos, (uint32_t *)scratch, count, (hipStream_t)stream));
    return TS2D_OK;
}

int tsm_scatter_rows(int64_t rows, int32_t row_bytes, const uint32_t *pos, const void *src, void *dst, int64_t dst_row0, void *stream)
{
    if (int rc = rows_ok(rows, row_bytes, pos, src, dst)) return rc;
    TS_HIP(ts_model_scatter_rows(rows, row_bytes / 4, pos, src, dst, dst_row0, (hipStream_t)stream));
    return TS2D_OK;
}
int tsm_gather_rows(int64_t rows, int32_t row_bytes, const uint32_t *idx, const void *src, void *dst, int64_t dst_row0, void *stream)
{
    if (int rc = rows_ok(rows, row_bytes, idx, src, dst)) return rc;
    TS_HIP(ts_model_gather_rows(rows, row_bytes / 4, idx, src, dst, dst_row0, (hipStream_t)stream));
    return TS2D_OK;
}
int tsm_grow_classify(int32_t P, const float *vertex, float *gradient_accum, float *gradient_denom, float min_view_count, float grad_threshold,
                      float split_scale_threshold, uint8_t *code, void *stream)
{
    if (P < 0) return ts_fail(TS2D_ERR_INVALID, "P must be >= 0");
    if (P > 0 && (!vertex || !gradient_accum || !gradient_denom || !code)) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    TS_HIP(ts_model_grow_classify(P, vertex, gradient_accum, gradient_denom, min_view_count, grad_threshold, split_scale_threshold, code,
                                  (hipStream_t)stream));
    return TS2D_OK;
}
int tsm_split_vertex(int32_t n_split, const uint32_t *parents, const float *vertex, float *child1, float *child2, void *stream)
{
    if (n_split < 0) return ts_fail(TS2D_ERR_INVALID, "n_split must be >= 0");
    if (n_split > 0 && (!parents || !vertex || !child1 || !child2)) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    TS_HIP(ts_model_split_vertex(n_split, parents, vertex, child1, child2, (hipStream_t)stream));
    return TS2D_OK;
}
int tsm_update_mask(int32_t P, int32_t mode, const float *opacity, const float *vertex, const float *max_radii2D, float a, float b, uint8_t *mask,
                    void *stream)
{
    if (P < 0 || mode < 0 || mode > 3) return ts_fail(TS2D_ERR_INVALID, "bad P / mode");
    if (P > 0 && (!mask || (mode <= 1 && !opacity) || (mode >= 2 && !vertex) || (mode == 2 && !max_radii2D)))
        return ts_fail(TS2D_ERR_INVALID, "null pointer");
    TS_HIP(ts_model_update_mask(P, mode, opacity, vertex, max_radii2D, a, b, mask, (hipStream_t)stream));
    return TS2D_OK;
}
int tsm_clip(int32_t P, int32_t mode, const uint8_t *mask, float value, float *param, float *exp_avg, float *exp_avg_sq, void *stream)
{
    if (P < 0 || mode < 0 || mode > 1) return ts_fail(TS2D_ERR_INVALID, "bad P / mode");
    if (P > 0 && (!mask || !param || ((exp_avg == nullptr) != (exp_avg_sq == nullptr)))) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    TS_HIP(ts_model_clip(P, mode, mask, value, param, exp_avg, exp_avg_sq, (hipStream_t)stream));
    return TS2D_OK;
}
int tsm_opacity_reset(int32_t P, float reset_value, float *opacity, float *exp_avg, float *exp_avg_sq, void *stream)
{
    if (P < 0) return ts_fail(TS2D_ERR_INVALID, "P must be >= 0");
    if (P > 0 && (!opacity || ((exp_avg == nullptr) != (exp_avg_sq == nullptr)))) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    TS_HIP(ts_model_opacity_reset(P, reset_value, opacity, exp_avg, exp_avg_sq, (hipStream_t)stream));
    return TS2D_OK;
}

int tsm_max_vertex_distance(int32_t n_vertices, const float *vertex, const float *camera_center, float *out, void *stream)
{
    if (n_vertices < 0) return ts_fail(TS2D_ERR_INVALID, "n_vertices must be >= 0");
    if (!out || (n_vertices > 0 && (!vertex || !camera_center))) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    TS_HIP(ts_model_max_distance(n_vertices, vertex, camera_center, out, (hipStream_t)stream));
    return TS2D_OK;
}

int tsm_state_digest(int32_t num_segments, const void *const *segments, const uint64_t *num_words, uint64_t *digests, void *stream)
{
    if (num_segments < 0 || num_segments > TSM_DIGEST_MAX_SEGMENTS)
        return ts_fail(TS2D_ERR_INVALID, "num_segments must be in 0..%d (got %d)", TSM_DIGEST_MAX_SEGMENTS, (int)num_segments);
    if (num_segments == 0) return TS2D_OK;
    if (!segments || !num_words || !digests) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    for (int i = 0; i < num_segments; i++)
    {
        if (num_words[i] >= (1ull << 32)) return ts_fail(TS2D_ERR_INVALID, "segment %d: num_words must be below 2^32", i);
        if (num_words[i] && !segments[i]) return ts_fail(TS2D_ERR_INVALID, "segment %d: null pointer", i);
        if (num_words[i] && ((uintptr_t)segments[i] & 3)) return ts_fail(TS2D_ERR_INVALID, "segment %d: not aligned to 4 bytes", i);
    }
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("state_digest", s);
    TS_HIP(ts_model_state_digest(num_segments, segments, num_words, digests, s));
    return TS2D_OK;
}

// ---- include/ts_optim.h -----------------------------------------------------------------------------------------------
int tso_adam_step(const tso_adam_slice *slices, int32_t num_slices, double beta1, double beta2, double eps, void *stream)
{
    if (num_slices < 0 || num_slices > TSO_MAX_SLICES) return ts_fail(TS2D_ERR_INVALID, "num_slices must be in 0..%d", TSO_MAX_SLICES);
    if (num_slices > 0 && !slices) return ts_fail(TS2D_ERR_INVALID, "null slices");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return ts_fail(TS2D_ERR_INVALID, "betas must be in [0, 1)"); // torch/optim/adam.py
    if (!(eps >= 0.0)) return ts_fail(TS2D_ERR_INVALID, "Invalid epsilon value");
    for (int i = 0; i < num_slices; i++)
    {
        const tso_adam_slice &s = slices[i];
        if (s.count < 0) return ts_fail(TS2D_ERR_INVALID, "slice %d: count < 0", i);
        if (s.count > 0 && (!s.param || !s.grad || !s.exp_avg || !s.exp_avg_sq)) return ts_fail(TS2D_ERR_INVALID, "slice %d: null pointer", i);
        if (s.period < 0 || s.split < 0 || (s.period > 0 && s.split > s.period) || s.index0 < 0) return ts_fail(TS2D_ERR_INVALID, "slice %d: bad period / split / index0", i);
        if (!(s.bias2_sqrt > 0.0f)) return ts_fail(TS2D_ERR_INVALID, "slice %d: bias2_sqrt must be positive (step >= 1)", i);
    }
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("adam_step", st);
    TS_HIP(ts_optim_adam_step(slices, num_slices, beta1, beta2, eps, st));
    return TS2D_OK;
}

int tso_adam_step_sh_factored(const tso_sh_factored_step *a, double beta1, double beta2, double eps, void *stream)
{
    if (!a) return ts_fail(TS2D_ERR_INVALID, "null step");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return ts_fail(TS2D_ERR_INVALID, "betas must be in [0, 1)");
    if (!(eps >= 0.0)) return ts_fail(TS2D_ERR_INVALID, "Invalid epsilon value");
    if (a->P < 0 || a->V < 1) return ts_fail(TS2D_ERR_INVALID, "P must be >= 0 and V >= 1");
    if (a->M != 1 && a->M != 4 && a->M != 9 && a->M != 16) return ts_fail(TS2D_ERR_INVALID, "M must be 1, 4, 9 or 16");
    if (a->sh_degree < 0 || (a->sh_degree + 1) * (a->sh_degree + 1) > a->M) return ts_fail(TS2D_ERR_INVALID, "sh_degree does not fit M");
    if (a->P == 0) return TS2D_OK;
    if (!a->vertex || !a->campos || !a->dL_dcolor || !a->param_dc || !a->exp_avg_dc || !a->exp_avg_sq_dc) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (a->M > 1 && (!a->param_rest || !a->exp_avg_rest || !a->exp_avg_sq_rest)) return ts_fail(TS2D_ERR_INVALID, "null f_rest pointer");
    if (a->dc_stride < 3 || (a->M > 1 && a->rest_stride < 3 * (a->M - 1))) return ts_fail(TS2D_ERR_INVALID, "row strides too small");
    if (!(a->bias2_sqrt_dc > 0.0f) || (a->M > 1 && !(a->bias2_sqrt_rest > 0.0f))) return ts_fail(TS2D_ERR_INVALID, "bias2_sqrt must be positive (step >= 1)");
    if (a->num_rows < 0 || a->num_rows > TSO_SH_ROW_SLICES) return ts_fail(TS2D_ERR_INVALID, "num_rows must be in 0..%d", TSO_SH_ROW_SLICES);
    for (int r = 0; r < a->num_rows; r++)
    {
        if (!a->rows[r].param || !a->rows[r].grad || !a->rows[r].exp_avg || !a->rows[r].exp_avg_sq) return ts_fail(TS2D_ERR_INVALID, "row slice %d: null pointer", r);
        if (a->rows[r].floats_per_row < 1) return ts_fail(TS2D_ERR_INVALID, "row slice %d: floats_per_row must be >= 1", r);
        if (!(a->rows[r].bias2_sqrt > 0.0f)) return ts_fail(TS2D_ERR_INVALID, "row slice %d: bias2_sqrt must be positive (step >= 1)", r);
    }
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("adam_step_sh_factored", st);
    TS_HIP(ts_optim_adam_step_sh_factored(*a, beta1, beta2, eps, st));
    return TS2D_OK;
}

// ---- include/ts_knn.h -------------------------------------------------------------------------------------------------
size_t tsk_workspace_bytes(int32_t P) { return ts_knn_workspace_bytes(P); }

int tsk_mean_dist3(int32_t P, const float *points, float *mean_dist2, void *workspace, size_t workspace_bytes, void *stream)
{
    if (P < 0) return ts_fail(TS2D_ERR_INVALID, "P must be >= 0");
    if (P == 0) return TS2D_OK;
    if (!points || !mean_dist2) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (!workspace || workspace_bytes < ts_knn_workspace_bytes(P)) return ts_fail(TS2D_ERR_CAPACITY, "knn workspace too small");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("knn_mean_dist3", s);
    TS_HIP(ts_knn_mean_dist3(P, points, mean_dist2, workspace, s));
    return TS2D_OK;
}

int tsk_nearest_other(int32_t P, int32_t batch_size, const float *points, uint32_t *nearest, void *workspace,
                      size_t workspace_bytes, void *stream)
{
    if (P < 0) return ts_fail(TS2D_ERR_INVALID, "P must be >= 0");
    if (batch_size <= 0) return ts_fail(TS2D_ERR_INVALID, "batch_size must be greater than 0"); // interface.cu:30-33
    if (P % batch_size != 0) return ts_fail(TS2D_ERR_INVALID, "num_points % batch_size must be 0");
    if (P == 0) return TS2D_OK;
    if (!points || !nearest) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (!workspace || workspace_bytes < ts_knn_workspace_bytes(P)) return ts_fail(TS2D_ERR_CAPACITY, "knn workspace too small");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("knn_nearest_other", s);
    TS_HIP(ts_knn_nearest_other(P, batch_size, points, nearest, workspace, s));
    return TS2D_OK;
}
} // extern "C"
