// api_simplify.hip -- the C ABI of include/ts_simplify.h, the whole export list of libts_simplify.so.  The library links none of the other api
// units, so the error text lives here: one buffer per thread, like the last-error text of the other six libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_simplify.h"
#pragma GCC visibility pop
#include "ts_simplify_launch.h"

#include <cstdarg>
#include <cstdio>

namespace
{
thread_local char g_error[512] = "";
constexpr int32_t MAX_FACES = 715827882; // 3 F incidence slots stay below 2^31

int simp_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int simp_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

bool finite_f(float v) { return v >= -3.402823466e+38f && v <= 3.402823466e+38f; }

int counts_ok(int32_t V, int32_t F)
{
    if (V < 0 || F < 0) return simp_fail(TS2D_ERR_INVALID, "V and F must be >= 0, got %d and %d", (int)V, (int)F);
    if (F > MAX_FACES) return simp_fail(TS2D_ERR_CAPACITY, "F = %d exceeds %d faces", (int)F, (int)MAX_FACES);
    return TS2D_OK;
}

int grid_ok(float ox, float oy, float oz, float cell)
{
    if (!(cell > 0.0f) || !finite_f(cell)) return simp_fail(TS2D_ERR_INVALID, "cell must be finite and > 0, got %g", (double)cell);
    if (!finite_f(ox) || !finite_f(oy) || !finite_f(oz))
        return simp_fail(TS2D_ERR_INVALID, "origin must be finite, got (%g, %g, %g)", (double)ox, (double)oy, (double)oz);
    return TS2D_OK;
}

int workspace_ok(int32_t V, int32_t F, const void *workspace, size_t workspace_bytes)
{
    if (!workspace) return simp_fail(TS2D_ERR_INVALID, "workspace is null");
    if (workspace_bytes < tsq_workspace_bytes(V, F))
        return simp_fail(TS2D_ERR_INVALID, "simplify workspace too small: %zu < %zu", workspace_bytes, tsq_workspace_bytes(V, F));
    return TS2D_OK;
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : simp_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tsq_last_error(void) { return g_error; }

size_t tsq_workspace_bytes(int32_t V, int32_t F) { return ts_simplify_workspace_bytes(V, F > MAX_FACES ? MAX_FACES : F); }

int tsq_cluster_labels(int32_t V, const float *vertices, float ox, float oy, float oz, float cell, int32_t *label, void *workspace,
                       size_t workspace_bytes, void *stream)
{
    if (int rc = counts_ok(V, 0)) return rc;
    if (int rc = grid_ok(ox, oy, oz, cell)) return rc;
    if (V == 0) return TS2D_OK;
    if (!vertices || !label) return simp_fail(TS2D_ERR_INVALID, "vertices/label is null");
    if (int rc = workspace_ok(V, 0, workspace, workspace_bytes)) return rc;
    return enqueued(ts_simplify_labels(V, vertices, ox, oy, oz, cell, label, workspace, (hipStream_t)stream), "cluster_labels");
}

int tsq_place(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const int32_t *remap, float ox, float oy, float oz, float cell,
              float lambda, int32_t mode, const float *attributes, const uint8_t *attr_valid, int32_t C, float *out_vertices,
              float *out_attributes, uint8_t *out_valid, int32_t *member_count, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = counts_ok(V, F)) return rc;
    if (int rc = grid_ok(ox, oy, oz, cell)) return rc;
    if (!(lambda >= 0.0f) || !finite_f(lambda)) return simp_fail(TS2D_ERR_INVALID, "lambda must be finite and >= 0, got %g", (double)lambda);
    if (mode != TSQ_PLACE_MEAN && mode != TSQ_PLACE_QUADRIC)
        return simp_fail(TS2D_ERR_INVALID, "mode must be TSQ_PLACE_MEAN or TSQ_PLACE_QUADRIC, got %d", (int)mode);
    if (attributes && (C < 1 || C > TSQ_MAX_CHANNELS)) return simp_fail(TS2D_ERR_INVALID, "C must be 1 .. %d, got %d", TSQ_MAX_CHANNELS, (int)C);
    if (V == 0) return TS2D_OK;
    if (!vertices || !remap || !out_vertices || !member_count) return simp_fail(TS2D_ERR_INVALID, "vertices/remap/out_vertices/member_count is null");
    if (F > 0 && !faces) return simp_fail(TS2D_ERR_INVALID, "faces is null with F = %d", (int)F);
    if (attributes && (!out_attributes || !out_valid)) return simp_fail(TS2D_ERR_INVALID, "out_attributes/out_valid is null with attributes");
    if (int rc = workspace_ok(V, F, workspace, workspace_bytes)) return rc;
    return enqueued(ts_simplify_place(V, F, vertices, faces, remap, ox, oy, oz, cell, lambda, mode, attributes, attr_valid, C, out_vertices,
                                      out_attributes, out_valid, member_count, workspace, (hipStream_t)stream), "place");
}

int tsq_unique_faces(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep_in, uint8_t *keep_out, unsigned long long *counts,
                     void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = counts_ok(V, F)) return rc;
    if (!counts) return simp_fail(TS2D_ERR_INVALID, "counts is null");
    if (F > 0)
    {
        if (!faces || !keep_in || !keep_out) return simp_fail(TS2D_ERR_INVALID, "faces/keep_in/keep_out is null");
        if (keep_in == keep_out) return simp_fail(TS2D_ERR_INVALID, "keep_out may not alias keep_in");
        if (int rc = workspace_ok(V, F, workspace, workspace_bytes)) return rc;
    }
    return enqueued(ts_simplify_unique_faces(V, F, faces, keep_in, keep_out, counts, workspace, (hipStream_t)stream), "unique_faces");
}
} // extern "C"
