// api_manifold.hip -- the C ABI of include/ts_manifold.h, the whole export list of libts_manifold.so.  The library links none of the other
// api units, so the error text lives here: one buffer per thread, like the last-error text of the other nine libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_manifold.h"
#pragma GCC visibility pop
#include "ts_manifold_launch.h"

#include <cstdarg>
#include <cstdio>

namespace
{
thread_local char g_error[512] = "";
constexpr int32_t MAX_FACES = 715827882; // 3 F corners stay below 2^31; the sort's layout asks for no less (ts_smooth.h sorts as many records)

int manifold_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int manifold_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

int counts_ok(int32_t V, int32_t F)
{
    if (V < 0 || F < 0) return manifold_fail(TS2D_ERR_INVALID, "V and F must be >= 0, got %d and %d", (int)V, (int)F);
    if (F > MAX_FACES) return manifold_fail(TS2D_ERR_CAPACITY, "F = %d exceeds %d faces", (int)F, (int)MAX_FACES);
    return TS2D_OK;
}

int workspace_ok(int32_t V, int32_t F, const void *workspace, size_t workspace_bytes)
{
    if (!workspace) return manifold_fail(TS2D_ERR_INVALID, "workspace is null");
    if (workspace_bytes < tsf_workspace_bytes(V, F))
        return manifold_fail(TS2D_ERR_INVALID, "manifold workspace too small: %zu < %zu", workspace_bytes, tsf_workspace_bytes(V, F));
    return TS2D_OK;
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : manifold_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tsf_last_error(void) { return g_error; }

size_t tsf_workspace_bytes(int32_t V, int32_t F) { return ts_manifold_workspace_bytes(V, F > MAX_FACES ? MAX_FACES : F); }

int tsf_fans(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep, int32_t *corner_fan, int32_t *vertex_fans,
             unsigned long long *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = counts_ok(V, F)) return rc;
    if (!counts) return manifold_fail(TS2D_ERR_INVALID, "counts is null");
    if (V > 0 && !vertex_fans) return manifold_fail(TS2D_ERR_INVALID, "vertex_fans is null with V = %d", (int)V);
    if (F > 0)
    {
        if (!corner_fan) return manifold_fail(TS2D_ERR_INVALID, "corner_fan is null with F = %d", (int)F);
        if (V > 0)
        {
            if (!faces) return manifold_fail(TS2D_ERR_INVALID, "faces is null");
            if (int rc = workspace_ok(V, F, workspace, workspace_bytes)) return rc;
        }
    }
    return enqueued(ts_manifold_fans(V, F, faces, keep, corner_fan, vertex_fans, counts, workspace, (hipStream_t)stream), "fans");
}

int tsf_split(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep, const int32_t *corner_fan, int32_t capacity, int32_t *out_faces,
              int32_t *new_vertex_source, int32_t *new_vertex_fan, unsigned long long *totals, void *workspace, size_t workspace_bytes,
              void *stream)
{
    if (int rc = counts_ok(V, F)) return rc;
    if (capacity < 0) return manifold_fail(TS2D_ERR_INVALID, "capacity must be >= 0, got %d", (int)capacity);
    if ((long long)V + 3LL * F > 2147483647LL)
        return manifold_fail(TS2D_ERR_CAPACITY, "V + 3 F = %lld exceeds 2147483647, the index of the last new vertex", (long long)V + 3LL * F);
    if (!totals) return manifold_fail(TS2D_ERR_INVALID, "totals is null");
    if (capacity > 0 && (!new_vertex_source || !new_vertex_fan))
        return manifold_fail(TS2D_ERR_INVALID, "new_vertex_source/new_vertex_fan is null with capacity = %d", (int)capacity);
    if (F > 0)
    {
        if (!faces || !out_faces) return manifold_fail(TS2D_ERR_INVALID, "faces/out_faces is null with F = %d", (int)F);
        if (V > 0)
        {
            if (!corner_fan) return manifold_fail(TS2D_ERR_INVALID, "corner_fan is null");
            if (int rc = workspace_ok(V, F, workspace, workspace_bytes)) return rc;
        }
    }
    return enqueued(ts_manifold_split(V, F, faces, keep, corner_fan, capacity, out_faces, new_vertex_source, new_vertex_fan, totals, workspace,
                                      (hipStream_t)stream), "split");
}
} // extern "C"
