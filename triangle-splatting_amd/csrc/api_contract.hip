// api_contract.hip -- the C ABI of include/ts_contract.h, the whole export list of libts_contract.so.  The library links none of the other api
// units, so the error text lives here: one buffer per thread, like the last-error text of the other libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_contract.h"
#pragma GCC visibility pop
#include "ts_contract_launch.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace
{
thread_local char g_error[512] = "";
constexpr int32_t MAX_FACES = 536870911; // ts_collapse.h's: what can be collapsed by length can be contracted

int contract_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int contract_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

bool misaligned8(const void *p) { return ((size_t)p & 7) != 0; }
} // namespace

extern "C" {
const char *tsu_last_error(void) { return g_error; }

size_t tsu_workspace_bytes(int32_t V, int32_t F) { return ts_contract_workspace_bytes(V, F > MAX_FACES ? MAX_FACES : F); }

int tsu_contract(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, const uint8_t *pinned,
                 const double *quadrics, float max_cost, int32_t max_collapses, float max_edge, float min_cos, float lambda, float reach,
                 uint32_t seed, int32_t *out_faces, uint8_t *out_keep, int32_t *vertex_target, float *out_vertices, double *out_quadrics,
                 double *vertex_blend, int32_t *edge_vertices, uint8_t *edge_state, int32_t *edge_removed, uint8_t *edge_guard,
                 double *edge_cost, float *edge_position, unsigned long long *totals, void *workspace, size_t workspace_bytes, void *stream)
{
    if (V < 0 || F < 0) return contract_fail(TS2D_ERR_INVALID, "V and F must be >= 0, got %d and %d", (int)V, (int)F);
    if (F > MAX_FACES) return contract_fail(TS2D_ERR_CAPACITY, "F = %d exceeds %d faces: 3 F edges and 4 F faces must fit int32", (int)F, (int)MAX_FACES);
    if ((long long)V + 3LL * F > 2147483647LL)
        return contract_fail(TS2D_ERR_CAPACITY, "V + 3 F = %lld exceeds 2147483647, the capacity of the edge split", (long long)V + 3LL * F);
    if (max_collapses < 0) return contract_fail(TS2D_ERR_INVALID, "max_collapses must be >= 0, got %d", (int)max_collapses);
    if (!(max_cost >= 0.0f)) return contract_fail(TS2D_ERR_INVALID, "max_cost must be >= 0, got %g", (double)max_cost);
    if (!(max_edge > 0.0f)) return contract_fail(TS2D_ERR_INVALID, "max_edge must be > 0, got %g", (double)max_edge);
    if (!(min_cos >= 0.0f && min_cos <= 1.0f)) return contract_fail(TS2D_ERR_INVALID, "min_cos must lie in [0, 1], got %g", (double)min_cos);
    if (!(std::isfinite(lambda) && lambda >= 0.0f)) return contract_fail(TS2D_ERR_INVALID, "lambda must be finite and >= 0, got %g", (double)lambda);
    if (!(std::isfinite(reach) && reach >= 0.0f)) return contract_fail(TS2D_ERR_INVALID, "reach must be finite and >= 0, got %g", (double)reach);
    if (!totals) return contract_fail(TS2D_ERR_INVALID, "totals is null");
    if (!out_faces != !out_keep || !out_faces != !vertex_target || !out_faces != !out_vertices || !out_faces != !out_quadrics ||
        !out_faces != !vertex_blend)
        return contract_fail(TS2D_ERR_INVALID,
                             "out_faces, out_keep, vertex_target, out_vertices, out_quadrics and vertex_blend must all be given or all be null");
    if (V > 0 && !vertices) return contract_fail(TS2D_ERR_INVALID, "vertices is null");
    if (V > 0 && !quadrics) return contract_fail(TS2D_ERR_INVALID, "quadrics is null");
    if (misaligned8(quadrics)) return contract_fail(TS2D_ERR_INVALID, "quadrics is not 8-byte aligned");
    if (misaligned8(out_quadrics)) return contract_fail(TS2D_ERR_INVALID, "out_quadrics is not 8-byte aligned");
    if (misaligned8(vertex_blend)) return contract_fail(TS2D_ERR_INVALID, "vertex_blend is not 8-byte aligned");
    if (misaligned8(edge_cost)) return contract_fail(TS2D_ERR_INVALID, "edge_cost is not 8-byte aligned");
    if (F > 0)
    {
        if (!faces) return contract_fail(TS2D_ERR_INVALID, "faces is null with F = %d", (int)F);
        if (!edge_vertices || !edge_state || !edge_removed || !edge_guard || !edge_cost || !edge_position)
            return contract_fail(TS2D_ERR_INVALID, "edge_vertices/edge_state/edge_removed/edge_guard/edge_cost/edge_position is null with F = %d",
                                 (int)F);
        if (!workspace) return contract_fail(TS2D_ERR_INVALID, "workspace is null");
        if (workspace_bytes < tsu_workspace_bytes(V, F))
            return contract_fail(TS2D_ERR_INVALID, "contract workspace too small: %zu < %zu", workspace_bytes, tsu_workspace_bytes(V, F));
    }
    const hipError_t e = ts_contract_round(V, F, vertices, faces, keep, pinned, quadrics, max_cost, max_collapses, max_edge, min_cos, lambda, reach,
                                           seed, out_faces, out_keep, vertex_target, out_vertices, out_quadrics, vertex_blend, edge_vertices,
                                           edge_state, edge_removed, edge_guard, edge_cost, edge_position, totals, workspace, (hipStream_t)stream);
    return e == hipSuccess ? TS2D_OK : contract_fail(TS2D_ERR_HIP, "contract: %s", hipGetErrorString(e));
}
} // extern "C"
