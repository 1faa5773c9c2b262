// api_ray.hip -- the C ABI of include/ts_ray.h, the whole export list of libts_ray.so.  The library links none of the other api units, so the
// error text lives here: one buffer per thread, like the last-error text of the other three libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_ray.h"
#pragma GCC visibility pop
#include "ts_ray_launch.h"

#include <cstdarg>
#include <cstdio>

#define TSR_MAX_COUNT (0x7fffffff - 1024) /* the launchers round counts up to whole workgroups of up to 1024 in 32-bit integers */

namespace
{
thread_local char g_error[512] = "";

int ray_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int ray_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

int count_ok(const char *name, int32_t n)
{
    if (n < 0) return ray_fail(TS2D_ERR_INVALID, "%s must be >= 0", name);
    if (n > TSR_MAX_COUNT) return ray_fail(TS2D_ERR_INVALID, "%s must be at most %d", name, TSR_MAX_COUNT);
    return TS2D_OK;
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : ray_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tsr_last_error(void) { return g_error; }

size_t tsr_cast_workspace_bytes(int32_t Q) { return ts_ray_cast_workspace_bytes(Q); }

int tsr_cast(int32_t Q, const float *origins, const float *directions, const float *t_limit, double tmin, double tmax, int32_t cull_back, int32_t F,
             const void *bvh, size_t bvh_bytes, int32_t *face, double *t, float *bary, int8_t *side, unsigned long long *leaf_visits, void *workspace,
             size_t workspace_bytes, void *stream)
{
    if (int rc = count_ok("Q", Q)) return rc;
    if (int rc = count_ok("F", F)) return rc;
    if (tmin != tmin || tmax != tmax) return ray_fail(TS2D_ERR_INVALID, "tmin/tmax is NaN");
    if (tmin > tmax) return ray_fail(TS2D_ERR_INVALID, "tmin %g exceeds tmax %g", tmin, tmax);
    if (cull_back != 0 && cull_back != 1) return ray_fail(TS2D_ERR_INVALID, "cull_back must be 0 or 1, got %d", (int)cull_back);
    if (Q == 0) return TS2D_OK;
    if (!origins || !directions || !face || !t) return ray_fail(TS2D_ERR_INVALID, "origins/directions/face/t is null");
    if (F > 0)
    {
        if (!bvh) return ray_fail(TS2D_ERR_INVALID, "bvh is null");
        if (bvh_bytes < ts_ray_bvh_bytes(F)) return ray_fail(TS2D_ERR_INVALID, "bvh too small: %zu < %zu", bvh_bytes, ts_ray_bvh_bytes(F));
        if (!workspace) return ray_fail(TS2D_ERR_INVALID, "workspace is null");
        if (workspace_bytes < ts_ray_cast_workspace_bytes(Q))
            return ray_fail(TS2D_ERR_INVALID, "cast workspace too small: %zu < %zu", workspace_bytes, ts_ray_cast_workspace_bytes(Q));
    }
    return enqueued(ts_ray_cast(Q, origins, directions, t_limit, tmin, tmax, (int)cull_back, F, bvh, face, t, bary, side, leaf_visits, workspace,
                                (hipStream_t)stream), "cast");
}
} // extern "C"
