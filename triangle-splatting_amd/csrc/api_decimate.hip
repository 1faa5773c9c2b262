// api_decimate.hip -- the C ABI of include/ts_decimate.h, the whole export list of libts_decimate.so.  The library links none of the other api
// units, so the error text lives here: one buffer per thread, like the last-error text of the other libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_decimate.h"
#pragma GCC visibility pop
#include "ts_decimate_launch.h"

#include <cstdarg>
#include <cstdio>

namespace
{
thread_local char g_error[512] = "";
constexpr int32_t MAX_FACES = 536870911; // ts_collapse.h's: what can be collapsed by length can be decimated

int decimate_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int decimate_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

// the checks both calls share; 0 when they pass
int check_counts(int32_t V, int32_t F)
{
    if (V < 0 || F < 0) return decimate_fail(TS2D_ERR_INVALID, "V and F must be >= 0, got %d and %d", (int)V, (int)F);
    if (F > MAX_FACES) return decimate_fail(TS2D_ERR_CAPACITY, "F = %d exceeds %d faces: 3 F edges and 4 F faces must fit int32", (int)F, (int)MAX_FACES);
    if ((long long)V + 3LL * F > 2147483647LL)
        return decimate_fail(TS2D_ERR_CAPACITY, "V + 3 F = %lld exceeds 2147483647, the capacity of the edge split", (long long)V + 3LL * F);
    return TS2D_OK;
}

bool misaligned8(const void *p) { return ((size_t)p & 7) != 0; }
} // namespace

extern "C" {
const char *tsz_last_error(void) { return g_error; }

size_t tsz_workspace_bytes(int32_t V, int32_t F) { return ts_decimate_workspace_bytes(V, F > MAX_FACES ? MAX_FACES : F); }

int tsz_vertex_quadrics(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, double *out_quadrics,
                        void *workspace, size_t workspace_bytes, void *stream)
{
    if (const int rc = check_counts(V, F)) return rc;
    if (V > 0 && !vertices) return decimate_fail(TS2D_ERR_INVALID, "vertices is null");
    if (V > 0 && !out_quadrics) return decimate_fail(TS2D_ERR_INVALID, "out_quadrics is null");
    if (misaligned8(out_quadrics)) return decimate_fail(TS2D_ERR_INVALID, "out_quadrics is not 8-byte aligned");
    if (F > 0)
    {
        if (!faces) return decimate_fail(TS2D_ERR_INVALID, "faces is null with F = %d", (int)F);
        if (V > 0 && !workspace) return decimate_fail(TS2D_ERR_INVALID, "workspace is null");
        if (V > 0 && workspace_bytes < tsz_workspace_bytes(V, F))
            return decimate_fail(TS2D_ERR_INVALID, "decimate workspace too small: %zu < %zu", workspace_bytes, tsz_workspace_bytes(V, F));
    }
    const hipError_t e = ts_decimate_quadrics(V, F, vertices, faces, keep, out_quadrics, workspace, (hipStream_t)stream);
    return e == hipSuccess ? TS2D_OK : decimate_fail(TS2D_ERR_HIP, "vertex_quadrics: %s", hipGetErrorString(e));
}

int tsz_decimate(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, const uint8_t *pinned,
                 const double *quadrics, float max_cost, int32_t max_collapses, float max_edge, float min_cos, uint32_t seed,
                 int32_t *out_faces, uint8_t *out_keep, int32_t *vertex_target, double *out_quadrics, int32_t *edge_vertices,
                 uint8_t *edge_state, int32_t *edge_removed, uint8_t *edge_guard, double *edge_cost, unsigned long long *totals,
                 void *workspace, size_t workspace_bytes, void *stream)
{
    if (const int rc = check_counts(V, F)) return rc;
    if (max_collapses < 0) return decimate_fail(TS2D_ERR_INVALID, "max_collapses must be >= 0, got %d", (int)max_collapses);
    if (!(max_cost >= 0.0f)) return decimate_fail(TS2D_ERR_INVALID, "max_cost must be >= 0, got %g", (double)max_cost);
    if (!(max_edge > 0.0f)) return decimate_fail(TS2D_ERR_INVALID, "max_edge must be > 0, got %g", (double)max_edge);
    if (!(min_cos >= 0.0f && min_cos <= 1.0f)) return decimate_fail(TS2D_ERR_INVALID, "min_cos must lie in [0, 1], got %g", (double)min_cos);
    if (!totals) return decimate_fail(TS2D_ERR_INVALID, "totals is null");
    if (!out_faces != !out_keep || !out_faces != !vertex_target || !out_faces != !out_quadrics)
        return decimate_fail(TS2D_ERR_INVALID, "out_faces, out_keep, vertex_target and out_quadrics must all be given or all be null");
    if (V > 0 && !vertices) return decimate_fail(TS2D_ERR_INVALID, "vertices is null");
    if (V > 0 && !quadrics) return decimate_fail(TS2D_ERR_INVALID, "quadrics is null");
    if (misaligned8(quadrics)) return decimate_fail(TS2D_ERR_INVALID, "quadrics is not 8-byte aligned");
    if (misaligned8(out_quadrics)) return decimate_fail(TS2D_ERR_INVALID, "out_quadrics is not 8-byte aligned");
    if (misaligned8(edge_cost)) return decimate_fail(TS2D_ERR_INVALID, "edge_cost is not 8-byte aligned");
    if (F > 0)
    {
        if (!faces) return decimate_fail(TS2D_ERR_INVALID, "faces is null with F = %d", (int)F);
        if (!edge_vertices || !edge_state || !edge_removed || !edge_guard || !edge_cost)
            return decimate_fail(TS2D_ERR_INVALID, "edge_vertices/edge_state/edge_removed/edge_guard/edge_cost is null with F = %d", (int)F);
        if (!workspace) return decimate_fail(TS2D_ERR_INVALID, "workspace is null");
        if (workspace_bytes < tsz_workspace_bytes(V, F))
            return decimate_fail(TS2D_ERR_INVALID, "decimate workspace too small: %zu < %zu", workspace_bytes, tsz_workspace_bytes(V, F));
    }
    const hipError_t e = ts_decimate_round(V, F, vertices, faces, keep, pinned, quadrics, max_cost, max_collapses, max_edge, min_cos, seed, out_faces,
                                           out_keep, vertex_target, out_quadrics, edge_vertices, edge_state, edge_removed, edge_guard, edge_cost,
                                           totals, workspace, (hipStream_t)stream);
    return e == hipSuccess ? TS2D_OK : decimate_fail(TS2D_ERR_HIP, "decimate: %s", hipGetErrorString(e));
}
} // extern "C"
