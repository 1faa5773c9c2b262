// api_inside.hip -- the C ABI of include/ts_inside.h, the whole export list of libts_inside.so.  The library links none of the other api
// units, so the error text lives here: one buffer per thread, like the last-error text of the other libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_inside.h"
#pragma GCC visibility pop
#include "ts_inside_launch.h"

#include <cstdarg>
#include <cstdio>

#define TSI_MAX_COUNT (0x7fffffff - 1024) /* the launchers round counts up to whole workgroups of up to 1024 in 32-bit integers */
#define TSI_MAX_FACES 0x3fffffff          /* 2 F half crossings must fit an int32 */

namespace
{
thread_local char g_error[512] = "";

int inside_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int inside_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

int count_ok(const char *name, int32_t n)
{
    if (n < 0) return inside_fail(TS2D_ERR_INVALID, "%s must be >= 0", name);
    if (n > TSI_MAX_COUNT) return inside_fail(TS2D_ERR_INVALID, "%s must be at most %d", name, TSI_MAX_COUNT);
    return TS2D_OK;
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : inside_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tsi_last_error(void) { return g_error; }

size_t tsi_crossings_workspace_bytes(int32_t Q) { return ts_inside_crossings_workspace_bytes(Q); }

int tsi_crossings(int32_t Q, const float *origins, const float *directions, int32_t shared_direction, const float *t_limit, double tmin, double tmax,
                  int32_t F, const void *bvh, size_t bvh_bytes, int32_t *hits, int32_t *winding2, int32_t *touches, unsigned long long *leaf_visits,
                  void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = count_ok("Q", Q)) return rc;
    if (int rc = count_ok("F", F)) return rc;
    if (F > TSI_MAX_FACES) return inside_fail(TS2D_ERR_CAPACITY, "F must be at most %d: twice as many half crossings must fit an int32", TSI_MAX_FACES);
    if (tmin != tmin || tmax != tmax) return inside_fail(TS2D_ERR_INVALID, "tmin/tmax is NaN");
    if (tmin > tmax) return inside_fail(TS2D_ERR_INVALID, "tmin %g exceeds tmax %g", tmin, tmax);
    if (shared_direction != 0 && shared_direction != 1)
        return inside_fail(TS2D_ERR_INVALID, "shared_direction must be 0 or 1, got %d", (int)shared_direction);
    if (Q == 0) return TS2D_OK;
    if (!origins || !directions || !hits || !winding2 || !touches)
        return inside_fail(TS2D_ERR_INVALID, "origins/directions/hits/winding2/touches is null");
    if (F > 0)
    {
        if (!bvh) return inside_fail(TS2D_ERR_INVALID, "bvh is null");
        if (bvh_bytes < ts_inside_bvh_bytes(F)) return inside_fail(TS2D_ERR_INVALID, "bvh too small: %zu < %zu", bvh_bytes, ts_inside_bvh_bytes(F));
        if (!workspace) return inside_fail(TS2D_ERR_INVALID, "workspace is null");
        if (workspace_bytes < ts_inside_crossings_workspace_bytes(Q))
            return inside_fail(TS2D_ERR_INVALID, "crossings workspace too small: %zu < %zu", workspace_bytes, ts_inside_crossings_workspace_bytes(Q));
    }
    return enqueued(ts_inside_crossings(Q, origins, directions, (int)shared_direction, t_limit, tmin, tmax, F, bvh, hits, winding2, touches, leaf_visits,
                                        workspace, (hipStream_t)stream), "crossings");
}

int tsi_signed_distance(int32_t Q, const double *dist2, const int32_t *winding2, const int32_t *touches, const int32_t *hits, int32_t rule,
                        int32_t only_undecided, float *out, uint8_t *decided, void *stream)
{
    if (int rc = count_ok("Q", Q)) return rc;
    if (rule < 0 || rule > 2) return inside_fail(TS2D_ERR_INVALID, "rule must be 0 (nonzero), 1 (odd) or 2 (positive), got %d", (int)rule);
    if (only_undecided != 0 && only_undecided != 1)
        return inside_fail(TS2D_ERR_INVALID, "only_undecided must be 0 or 1, got %d", (int)only_undecided);
    if (Q == 0) return TS2D_OK;
    if (!dist2 || !winding2 || !touches || !hits || !out || !decided)
        return inside_fail(TS2D_ERR_INVALID, "dist2/winding2/touches/hits/out/decided is null");
    return enqueued(ts_inside_signed_distance(Q, dist2, winding2, touches, hits, (int)rule, (int)only_undecided, out, decided, (hipStream_t)stream),
                    "signed_distance");
}
} // extern "C"
