// api_subdivide.hip -- the C ABI of include/ts_subdivide.h, the whole export list of libts_subdivide.so.  The library links none of the other
// api units, so the error text lives here: one buffer per thread, like the last-error text of the other libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_subdivide.h"
#pragma GCC visibility pop
#include "ts_subdivide_launch.h"

#include <cstdarg>
#include <cstdio>

namespace
{
thread_local char g_error[512] = "";
constexpr int32_t MAX_FACES = 536870911; // 4 F output faces stay below 2^31, and the 3 F half-edges with them

int subdivide_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int subdivide_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

int counts_ok(int32_t V, int32_t F)
{
    if (V < 0 || F < 0) return subdivide_fail(TS2D_ERR_INVALID, "V and F must be >= 0, got %d and %d", (int)V, (int)F);
    if (F > MAX_FACES) return subdivide_fail(TS2D_ERR_CAPACITY, "F = %d exceeds %d faces: 3 F edges and 4 F faces must fit int32", (int)F, (int)MAX_FACES);
    if ((long long)V + 3LL * F > 2147483647LL)
        return subdivide_fail(TS2D_ERR_CAPACITY, "V + 3 F = %lld exceeds 2147483647, the index of the last new vertex", (long long)V + 3LL * F);
    return TS2D_OK;
}

int workspace_ok(int32_t V, int32_t F, const void *workspace, size_t workspace_bytes)
{
    if (!workspace) return subdivide_fail(TS2D_ERR_INVALID, "workspace is null");
    if (workspace_bytes < tsd_workspace_bytes(V, F))
        return subdivide_fail(TS2D_ERR_INVALID, "subdivide workspace too small: %zu < %zu", workspace_bytes, tsd_workspace_bytes(V, F));
    return TS2D_OK;
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : subdivide_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tsd_last_error(void) { return g_error; }

size_t tsd_workspace_bytes(int32_t V, int32_t F) { return ts_subdivide_workspace_bytes(V, F > MAX_FACES ? MAX_FACES : F); }

int tsd_edges(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, int32_t *edge_vertices,
              int32_t *edge_use, double *edge_length2, int32_t *half_edge_edge, unsigned long long *counts, void *workspace,
              size_t workspace_bytes, void *stream)
{
    if (int rc = counts_ok(V, F)) return rc;
    if (!counts) return subdivide_fail(TS2D_ERR_INVALID, "counts is null");
    if (F > 0)
    {
        if (!faces) return subdivide_fail(TS2D_ERR_INVALID, "faces is null with F = %d", (int)F);
        if (!edge_vertices || !edge_use || !half_edge_edge)
            return subdivide_fail(TS2D_ERR_INVALID, "edge_vertices/edge_use/half_edge_edge is null with F = %d", (int)F);
        if (edge_length2 && V > 0 && !vertices) return subdivide_fail(TS2D_ERR_INVALID, "vertices is null with edge_length2 given");
        if (int rc = workspace_ok(V, F, workspace, workspace_bytes)) return rc;
    }
    return enqueued(ts_subdivide_edges(V, F, vertices, faces, keep, edge_vertices, edge_use, edge_length2, half_edge_edge, counts, workspace,
                                       (hipStream_t)stream), "edges");
}

int tsd_split(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, int32_t mode, float max_edge,
              const float *vertex_limit, const float *attributes, const uint8_t *attr_valid, int32_t channels, float *new_vertices,
              float *new_attributes, uint8_t *new_attr_valid, int32_t *new_vertex_edge, int32_t *out_faces, int32_t *out_face_parent,
              unsigned long long *totals, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = counts_ok(V, F)) return rc;
    if (mode != TSD_MARK_ALL && mode != TSD_MARK_LONGER && mode != TSD_MARK_VERTEX_LIMIT)
        return subdivide_fail(TS2D_ERR_INVALID, "mode must be TSD_MARK_ALL, TSD_MARK_LONGER or TSD_MARK_VERTEX_LIMIT, got %d", (int)mode);
    if (mode == TSD_MARK_LONGER && !(max_edge >= 0.0f)) return subdivide_fail(TS2D_ERR_INVALID, "max_edge must be >= 0, got %g", (double)max_edge);
    if (channels < 0) return subdivide_fail(TS2D_ERR_INVALID, "channels must be >= 0, got %d", (int)channels);
    if (!totals) return subdivide_fail(TS2D_ERR_INVALID, "totals is null");
    if (F > 0)
    {
        if (!faces) return subdivide_fail(TS2D_ERR_INVALID, "faces is null with F = %d", (int)F);
        if (!new_vertices || !new_vertex_edge || !out_faces || !out_face_parent)
            return subdivide_fail(TS2D_ERR_INVALID, "new_vertices/new_vertex_edge/out_faces/out_face_parent is null with F = %d", (int)F);
        if (channels > 0 && (!new_attributes || !new_attr_valid))
            return subdivide_fail(TS2D_ERR_INVALID, "new_attributes/new_attr_valid is null with channels = %d", (int)channels);
        if (V > 0)
        {
            if (!vertices) return subdivide_fail(TS2D_ERR_INVALID, "vertices is null");
            if (mode == TSD_MARK_VERTEX_LIMIT && !vertex_limit) return subdivide_fail(TS2D_ERR_INVALID, "vertex_limit is null in TSD_MARK_VERTEX_LIMIT");
            if (channels > 0 && !attributes) return subdivide_fail(TS2D_ERR_INVALID, "attributes is null with channels = %d", (int)channels);
        }
        if (int rc = workspace_ok(V, F, workspace, workspace_bytes)) return rc;
    }
    return enqueued(ts_subdivide_split(V, F, vertices, faces, keep, mode, max_edge, vertex_limit, attributes, attr_valid, channels, new_vertices,
                                       new_attributes, new_attr_valid, new_vertex_edge, out_faces, out_face_parent, totals, workspace,
                                       (hipStream_t)stream), "split");
}
} // extern "C"
