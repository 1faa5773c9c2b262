// api_winding.hip -- the C ABI of include/ts_winding.h, the whole export list of libts_winding.so.  The library links none of the other api
// units, so the error text lives here: one buffer per thread, like the last-error text of the other libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_winding.h"
#pragma GCC visibility pop
#include "ts_winding_launch.h"

#include <cstdarg>
#include <cstdio>

#define TSN_MAX_COUNT (0x7fffffff - 1024) /* the launchers round counts up to whole workgroups of up to 1024 in 32-bit integers */
#define TSN_MAX_FACES 0x00ffffff          /* 2^37 F units must stay below 2^61: the header's overflow bound */

namespace
{
thread_local char g_error[512] = "";

int winding_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int winding_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

int count_ok(const char *name, int32_t n)
{
    if (n < 0) return winding_fail(TS2D_ERR_INVALID, "%s must be >= 0", name);
    if (n > TSN_MAX_COUNT) return winding_fail(TS2D_ERR_INVALID, "%s must be at most %d", name, TSN_MAX_COUNT);
    return TS2D_OK;
}

int faces_ok(int32_t F)
{
    if (int rc = count_ok("F", F)) return rc;
    if (F > TSN_MAX_FACES)
        return winding_fail(TS2D_ERR_CAPACITY, "F must be at most %d: the int64 sum of the quantised terms must not wrap", TSN_MAX_FACES);
    return TS2D_OK;
}

int index_ok(int32_t F, const void *bvh, size_t bvh_bytes)
{
    if (!bvh) return winding_fail(TS2D_ERR_INVALID, "bvh is null");
    if (bvh_bytes < ts_winding_bvh_bytes(F)) return winding_fail(TS2D_ERR_INVALID, "bvh too small: %zu < %zu", bvh_bytes, ts_winding_bvh_bytes(F));
    return TS2D_OK;
}

int moments_ok(int32_t F, const void *moments, size_t moments_bytes)
{
    if (!moments) return winding_fail(TS2D_ERR_INVALID, "moments is null");
    if (moments_bytes < ts_winding_moments_bytes(F))
        return winding_fail(TS2D_ERR_INVALID, "moments too small: %zu < %zu", moments_bytes, ts_winding_moments_bytes(F));
    return TS2D_OK;
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : winding_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tsn_last_error(void) { return g_error; }

size_t tsn_moments_bytes(int32_t F) { return ts_winding_moments_bytes(F); }

size_t tsn_leaf_faces_bytes(int32_t F) { return ts_winding_leaf_faces_bytes(F); }

size_t tsn_winding_workspace_bytes(int32_t Q) { return ts_winding_workspace_bytes(Q); }

int tsn_moments(int32_t F, const void *bvh, size_t bvh_bytes, double *moments, size_t moments_bytes, int32_t *leaf_faces, size_t leaf_faces_bytes,
                void *stream)
{
    if (int rc = faces_ok(F)) return rc;
    if (F == 0) return TS2D_OK;
    if (int rc = index_ok(F, bvh, bvh_bytes)) return rc;
    if (int rc = moments_ok(F, moments, moments_bytes)) return rc;
    if (leaf_faces && leaf_faces_bytes < ts_winding_leaf_faces_bytes(F))
        return winding_fail(TS2D_ERR_INVALID, "leaf_faces too small: %zu < %zu", leaf_faces_bytes, ts_winding_leaf_faces_bytes(F));
    return enqueued(ts_winding_moments(F, bvh, moments, leaf_faces, (hipStream_t)stream), "moments");
}

int tsn_winding(int32_t Q, const float *points, double beta, int32_t F, const void *bvh, size_t bvh_bytes, const double *moments,
                size_t moments_bytes, int64_t *wq, int32_t *terms, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = count_ok("Q", Q)) return rc;
    if (int rc = faces_ok(F)) return rc;
    if (beta != beta) return winding_fail(TS2D_ERR_INVALID, "beta is NaN");
    if (beta < 1.0) return winding_fail(TS2D_ERR_INVALID, "beta must be at least 1 (+inf for the exact sum), got %g", beta);
    if (Q == 0) return TS2D_OK;
    if (!points || !wq) return winding_fail(TS2D_ERR_INVALID, "points/wq is null");
    if (F > 0)
    {
        if (int rc = index_ok(F, bvh, bvh_bytes)) return rc;
        if (int rc = moments_ok(F, moments, moments_bytes)) return rc;
        if (!workspace) return winding_fail(TS2D_ERR_INVALID, "workspace is null");
        if (workspace_bytes < ts_winding_workspace_bytes(Q))
            return winding_fail(TS2D_ERR_INVALID, "winding workspace too small: %zu < %zu", workspace_bytes, ts_winding_workspace_bytes(Q));
    }
    return enqueued(ts_winding_query(Q, points, beta * beta, F, bvh, moments, wq, terms, workspace, (hipStream_t)stream), "winding");
}

int tsn_sign_distance(int32_t Q, const double *dist2, const int64_t *wq, int64_t threshold, float *out, uint8_t *decided, void *stream)
{
    if (int rc = count_ok("Q", Q)) return rc;
    if (Q == 0) return TS2D_OK;
    if (!dist2 || !wq || !out || !decided) return winding_fail(TS2D_ERR_INVALID, "dist2/wq/out/decided is null");
    return enqueued(ts_winding_sign_distance(Q, dist2, wq, threshold, out, decided, (hipStream_t)stream), "sign_distance");
}
} // extern "C"
