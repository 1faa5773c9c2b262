// api_geom.hip -- the C ABI of include/ts_geom.h, the whole export list of libts_geom.so.  The library does not link api.hip, so the error
// text lives here: one buffer per thread, like the last-error text of libts2d.so.
#pragma GCC visibility push(default)
#include "../../include/ts_geom.h"
#pragma GCC visibility pop
#include "ts_geom_launch.h"

#include <cstdarg>
#include <cstdio>

#define TSG_MAX_COUNT (0x7fffffff - 1024) /* the launchers round counts up to whole workgroups of up to 1024 in 32-bit integers */

namespace
{
thread_local char g_error[512] = "";

int geom_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int geom_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

int count_ok(const char *name, int32_t n)
{
    if (n < 0) return geom_fail(TS2D_ERR_INVALID, "%s must be >= 0", name);
    if (n > TSG_MAX_COUNT) return geom_fail(TS2D_ERR_INVALID, "%s must be at most %d", name, TSG_MAX_COUNT);
    return TS2D_OK;
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : geom_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tsg_last_error(void) { return g_error; }

size_t tsg_cross_workspace_bytes(int32_t Q, int32_t R) { return ts_geom_cross_workspace_bytes(Q, R); }

int tsg_nearest_cross(int32_t Q, const float *queries, int32_t R, const float *refs, int32_t *nearest, float *dist2,
                      unsigned long long *box_visits, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = count_ok("Q", Q)) return rc;
    if (int rc = count_ok("R", R)) return rc;
    if (Q == 0) return TS2D_OK;
    if (!queries || !nearest || !dist2) return geom_fail(TS2D_ERR_INVALID, "queries/nearest/dist2 is null");
    if (R > 0 && !refs) return geom_fail(TS2D_ERR_INVALID, "refs is null");
    if (!workspace) return geom_fail(TS2D_ERR_INVALID, "workspace is null");
    if (workspace_bytes < ts_geom_cross_workspace_bytes(Q, R))
        return geom_fail(TS2D_ERR_INVALID, "search workspace too small: %zu < %zu", workspace_bytes, ts_geom_cross_workspace_bytes(Q, R));
    return enqueued(ts_geom_nearest_cross(Q, queries, R, refs, nearest, dist2, box_visits, workspace, (hipStream_t)stream), "nearest_cross");
}

size_t tsg_sample_workspace_bytes(int32_t F) { return ts_geom_sample_workspace_bytes(F); }

int tsg_face_areas(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, double *area, void *stream)
{
    if (int rc = count_ok("V", V)) return rc;
    if (int rc = count_ok("F", F)) return rc;
    if (F == 0) return TS2D_OK;
    if (!faces || !area || (V > 0 && !vertices)) return geom_fail(TS2D_ERR_INVALID, "vertices/faces/area is null");
    return enqueued(ts_geom_face_areas(V, F, vertices, faces, keep, area, (hipStream_t)stream), "face_areas");
}

int tsg_sample_surface(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const double *area, int32_t N, uint64_t seed,
                       float *points, int32_t *face, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = count_ok("V", V)) return rc;
    if (int rc = count_ok("F", F)) return rc;
    if (int rc = count_ok("N", N)) return rc;
    if (N == 0) return TS2D_OK;
    if (!points || !face) return geom_fail(TS2D_ERR_INVALID, "points/face is null");
    if (F > 0 && (!faces || !area || (V > 0 && !vertices))) return geom_fail(TS2D_ERR_INVALID, "vertices/faces/area is null");
    if (!workspace) return geom_fail(TS2D_ERR_INVALID, "workspace is null");
    if (workspace_bytes < ts_geom_sample_workspace_bytes(F))
        return geom_fail(TS2D_ERR_INVALID, "sampler workspace too small: %zu < %zu", workspace_bytes, ts_geom_sample_workspace_bytes(F));
    return enqueued(ts_geom_sample_surface(V, F, vertices, faces, area, N, seed, points, face, workspace, (hipStream_t)stream), "sample_surface");
}
} // extern "C"
