// api_collapse.hip -- the C ABI of include/ts_collapse.h, the whole export list of libts_collapse.so.  The library links none of the other api
// units, so the error text lives here: one buffer per thread, like the last-error text of the other libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_collapse.h"
#pragma GCC visibility pop
#include "ts_collapse_launch.h"

#include <cstdarg>
#include <cstdio>

namespace
{
thread_local char g_error[512] = "";
constexpr int32_t MAX_FACES = 536870911; // ts_flip.h's: what can be split and flipped can be collapsed

int collapse_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int collapse_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}
} // namespace

extern "C" {
const char *tsp_last_error(void) { return g_error; }

size_t tsp_workspace_bytes(int32_t V, int32_t F) { return ts_collapse_workspace_bytes(V, F > MAX_FACES ? MAX_FACES : F); }

int tsp_collapse(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, const uint8_t *pinned, int32_t mode,
                 float min_edge, const float *vertex_limit, float max_edge, float min_cos, uint32_t seed, int32_t *out_faces,
                 uint8_t *out_keep, int32_t *vertex_target, int32_t *edge_vertices, uint8_t *edge_state, int32_t *edge_removed,
                 uint8_t *edge_guard, unsigned long long *totals, void *workspace, size_t workspace_bytes, void *stream)
{
    if (V < 0 || F < 0) return collapse_fail(TS2D_ERR_INVALID, "V and F must be >= 0, got %d and %d", (int)V, (int)F);
    if (F > MAX_FACES) return collapse_fail(TS2D_ERR_CAPACITY, "F = %d exceeds %d faces: 3 F edges and 4 F faces must fit int32", (int)F, (int)MAX_FACES);
    if ((long long)V + 3LL * F > 2147483647LL)
        return collapse_fail(TS2D_ERR_CAPACITY, "V + 3 F = %lld exceeds 2147483647, the capacity of the edge split", (long long)V + 3LL * F);
    if (mode != TSP_MARK_SHORTER && mode != TSP_MARK_VERTEX_LIMIT) return collapse_fail(TS2D_ERR_INVALID, "unknown mode %d", (int)mode);
    if (mode == TSP_MARK_SHORTER && !(min_edge >= 0.0f)) return collapse_fail(TS2D_ERR_INVALID, "min_edge must be >= 0, got %g", (double)min_edge);
    if (!(max_edge > 0.0f)) return collapse_fail(TS2D_ERR_INVALID, "max_edge must be > 0, got %g", (double)max_edge);
    if (!(min_cos >= 0.0f && min_cos <= 1.0f)) return collapse_fail(TS2D_ERR_INVALID, "min_cos must lie in [0, 1], got %g", (double)min_cos);
    if (!totals) return collapse_fail(TS2D_ERR_INVALID, "totals is null");
    if (!out_faces != !out_keep || !out_faces != !vertex_target)
        return collapse_fail(TS2D_ERR_INVALID, "out_faces, out_keep and vertex_target must all be given or all be null");
    if (V > 0 && !vertices) return collapse_fail(TS2D_ERR_INVALID, "vertices is null");
    if (V > 0 && mode == TSP_MARK_VERTEX_LIMIT && !vertex_limit) return collapse_fail(TS2D_ERR_INVALID, "vertex_limit is null in TSP_MARK_VERTEX_LIMIT");
    if (F > 0)
    {
        if (!faces) return collapse_fail(TS2D_ERR_INVALID, "faces is null with F = %d", (int)F);
        if (!edge_vertices || !edge_state || !edge_removed || !edge_guard)
            return collapse_fail(TS2D_ERR_INVALID, "edge_vertices/edge_state/edge_removed/edge_guard is null with F = %d", (int)F);
        if (!workspace) return collapse_fail(TS2D_ERR_INVALID, "workspace is null");
        if (workspace_bytes < tsp_workspace_bytes(V, F))
            return collapse_fail(TS2D_ERR_INVALID, "collapse workspace too small: %zu < %zu", workspace_bytes, tsp_workspace_bytes(V, F));
    }
    const hipError_t e = ts_collapse_round(V, F, vertices, faces, keep, pinned, mode, min_edge, vertex_limit, max_edge, min_cos, seed, out_faces,
                                           out_keep, vertex_target, edge_vertices, edge_state, edge_removed, edge_guard, totals, workspace,
                                           (hipStream_t)stream);
    return e == hipSuccess ? TS2D_OK : collapse_fail(TS2D_ERR_HIP, "collapse: %s", hipGetErrorString(e));
}
} // extern "C"
