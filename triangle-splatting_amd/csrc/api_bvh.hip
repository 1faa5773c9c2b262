// api_bvh.hip -- the C ABI of include/ts_bvh.h, the whole export list of libts_bvh.so.  The library links neither api.hip nor api_geom.hip, so
// the error text lives here: one buffer per thread, like the last-error text of the other two libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_bvh.h"
#pragma GCC visibility pop
#include "ts_bvh_launch.h"

#include <cstdarg>
#include <cstdio>

#define TSB_MAX_COUNT (0x7fffffff - 1024) /* the launchers round counts up to whole workgroups of up to 1024 in 32-bit integers */

namespace
{
thread_local char g_error[512] = "";

int bvh_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int bvh_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

int count_ok(const char *name, int32_t n)
{
    if (n < 0) return bvh_fail(TS2D_ERR_INVALID, "%s must be >= 0", name);
    if (n > TSB_MAX_COUNT) return bvh_fail(TS2D_ERR_INVALID, "%s must be at most %d", name, TSB_MAX_COUNT);
    return TS2D_OK;
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : bvh_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tsb_last_error(void) { return g_error; }

size_t tsb_bvh_bytes(int32_t F) { return ts_bvh_bytes(F); }

size_t tsb_build_workspace_bytes(int32_t F) { return ts_bvh_build_workspace_bytes(F); }

int tsb_build(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, void *bvh, size_t bvh_bytes, void *workspace,
              size_t workspace_bytes, void *stream)
{
    if (int rc = count_ok("V", V)) return rc;
    if (int rc = count_ok("F", F)) return rc;
    if (F == 0) return TS2D_OK;
    if (!faces || (V > 0 && !vertices)) return bvh_fail(TS2D_ERR_INVALID, "vertices/faces is null");
    if (!bvh) return bvh_fail(TS2D_ERR_INVALID, "bvh is null");
    if (bvh_bytes < ts_bvh_bytes(F)) return bvh_fail(TS2D_ERR_INVALID, "bvh too small: %zu < %zu", bvh_bytes, ts_bvh_bytes(F));
    if (!workspace) return bvh_fail(TS2D_ERR_INVALID, "workspace is null");
    if (workspace_bytes < ts_bvh_build_workspace_bytes(F))
        return bvh_fail(TS2D_ERR_INVALID, "build workspace too small: %zu < %zu", workspace_bytes, ts_bvh_build_workspace_bytes(F));
    return enqueued(ts_bvh_build(V, F, vertices, faces, keep, bvh, workspace, (hipStream_t)stream), "build");
}

size_t tsb_closest_workspace_bytes(int32_t Q) { return ts_bvh_closest_workspace_bytes(Q); }

int tsb_closest(int32_t Q, const float *queries, int32_t V, int32_t F, const float *vertices, const int32_t *faces, const void *bvh, size_t bvh_bytes,
                int32_t *face, double *dist2, float *point, unsigned long long *leaf_visits, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = count_ok("Q", Q)) return rc;
    if (int rc = count_ok("V", V)) return rc;
    if (int rc = count_ok("F", F)) return rc;
    if (Q == 0) return TS2D_OK;
    if (!queries || !face || !dist2) return bvh_fail(TS2D_ERR_INVALID, "queries/face/dist2 is null");
    if (F > 0)
    {
        if (!faces || (V > 0 && !vertices)) return bvh_fail(TS2D_ERR_INVALID, "vertices/faces is null");
        if (!bvh) return bvh_fail(TS2D_ERR_INVALID, "bvh is null");
        if (bvh_bytes < ts_bvh_bytes(F)) return bvh_fail(TS2D_ERR_INVALID, "bvh too small: %zu < %zu", bvh_bytes, ts_bvh_bytes(F));
        if (!workspace) return bvh_fail(TS2D_ERR_INVALID, "workspace is null");
        if (workspace_bytes < ts_bvh_closest_workspace_bytes(Q))
            return bvh_fail(TS2D_ERR_INVALID, "query workspace too small: %zu < %zu", workspace_bytes, ts_bvh_closest_workspace_bytes(Q));
    }
    return enqueued(ts_bvh_closest(Q, queries, F, bvh, face, dist2, point, leaf_visits, workspace, (hipStream_t)stream), "closest");
}
} // extern "C"
