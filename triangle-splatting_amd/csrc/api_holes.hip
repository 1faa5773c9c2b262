// api_holes.hip -- the C ABI of include/ts_holes.h, the whole export list of libts_holes.so.  The library links none of the other api
// units, so the error text lives here: one buffer per thread, like the last-error text of the other eight libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_holes.h"
#pragma GCC visibility pop
#include "ts_holes_launch.h"

#include <cstdarg>
#include <cstdio>

namespace
{
thread_local char g_error[512] = "";
constexpr int32_t MAX_FACES = 357913941; // 3 F half-edges, and the 6 F slots of ts_smooth.h's table, stay below 2^31

int holes_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int holes_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

int counts_ok(int32_t V, int32_t F)
{
    if (V < 0 || F < 0) return holes_fail(TS2D_ERR_INVALID, "V and F must be >= 0, got %d and %d", (int)V, (int)F);
    if (F > MAX_FACES) return holes_fail(TS2D_ERR_CAPACITY, "F = %d exceeds %d faces", (int)F, (int)MAX_FACES);
    return TS2D_OK;
}

int workspace_ok(int32_t V, int32_t F, const void *workspace, size_t workspace_bytes)
{
    if (!workspace) return holes_fail(TS2D_ERR_INVALID, "workspace is null");
    if (workspace_bytes < tsh_workspace_bytes(V, F))
        return holes_fail(TS2D_ERR_INVALID, "holes workspace too small: %zu < %zu", workspace_bytes, tsh_workspace_bytes(V, F));
    return TS2D_OK;
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : holes_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tsh_last_error(void) { return g_error; }

size_t tsh_workspace_bytes(int32_t V, int32_t F) { return ts_holes_workspace_bytes(V, F > MAX_FACES ? MAX_FACES : F); }

int tsh_loops(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep, const int32_t *offsets, const int32_t *neighbors,
              const int32_t *edge_faces, int32_t num_entries, int32_t *half_edge_loop, int32_t *loop_offsets, int32_t *loop_half_edges,
              unsigned long long *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = counts_ok(V, F)) return rc;
    if (num_entries < 0) return holes_fail(TS2D_ERR_INVALID, "num_entries must be >= 0, got %d", (int)num_entries);
    if (!counts) return holes_fail(TS2D_ERR_INVALID, "counts is null");
    if (!loop_offsets) return holes_fail(TS2D_ERR_INVALID, "loop_offsets is null");
    if (F > 0)
    {
        if (!half_edge_loop || !loop_half_edges) return holes_fail(TS2D_ERR_INVALID, "half_edge_loop/loop_half_edges is null with F = %d", (int)F);
        if (V > 0)
        {
            if (!faces || !offsets) return holes_fail(TS2D_ERR_INVALID, "faces/offsets is null");
            if (num_entries > 0 && (!neighbors || !edge_faces))
                return holes_fail(TS2D_ERR_INVALID, "neighbors/edge_faces is null with num_entries = %d", (int)num_entries);
            if (int rc = workspace_ok(V, F, workspace, workspace_bytes)) return rc;
        }
    }
    return enqueued(ts_holes_loops(V, F, faces, keep, offsets, neighbors, edge_faces, num_entries, half_edge_loop, loop_offsets, loop_half_edges,
                                   counts, workspace, (hipStream_t)stream), "loops");
}

int tsh_fill(int32_t V, int32_t F, const float *vertices, const int32_t *faces, int32_t num_loops, const int32_t *loop_offsets,
             const int32_t *loop_half_edges, int32_t num_members, int32_t max_loop_edges, const float *attributes, const uint8_t *attr_valid,
             int32_t channels, uint8_t *loop_status, float *new_vertices, float *new_attributes, uint8_t *new_attr_valid, int32_t *new_faces,
             int32_t *new_face_loop, unsigned long long *totals, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = counts_ok(V, F)) return rc;
    if (num_loops < 0 || num_members < 0 || channels < 0)
        return holes_fail(TS2D_ERR_INVALID, "num_loops, num_members and channels must be >= 0, got %d, %d and %d", (int)num_loops, (int)num_members,
                          (int)channels);
    if (max_loop_edges < 0) return holes_fail(TS2D_ERR_INVALID, "max_loop_edges must be >= 0, got %d", (int)max_loop_edges);
    if (num_loops > F || (long long)num_members > 3LL * F)
        return holes_fail(TS2D_ERR_INVALID, "num_loops = %d and num_members = %d exceed F = %d loops and 3 F members", (int)num_loops,
                          (int)num_members, (int)F);
    if (!totals) return holes_fail(TS2D_ERR_INVALID, "totals is null");
    if (num_members > 0 && (!new_faces || !new_face_loop)) return holes_fail(TS2D_ERR_INVALID, "new_faces/new_face_loop is null");
    if (num_loops > 0)
    {
        if (!loop_offsets || !loop_status || !new_vertices) return holes_fail(TS2D_ERR_INVALID, "loop_offsets/loop_status/new_vertices is null");
        if (num_members > 0 && (!loop_half_edges || !faces)) return holes_fail(TS2D_ERR_INVALID, "loop_half_edges/faces is null");
        if (V > 0 && !vertices) return holes_fail(TS2D_ERR_INVALID, "vertices is null");
        if (channels > 0 && (!new_attributes || !new_attr_valid || (V > 0 && !attributes)))
            return holes_fail(TS2D_ERR_INVALID, "attributes/new_attributes/new_attr_valid is null with channels = %d", (int)channels);
        if (int rc = workspace_ok(V, F, workspace, workspace_bytes)) return rc;
    }
    return enqueued(ts_holes_fill(V, F, vertices, faces, num_loops, loop_offsets, loop_half_edges, num_members, max_loop_edges, attributes,
                                  attr_valid, channels, loop_status, new_vertices, new_attributes, new_attr_valid, new_faces, new_face_loop, totals,
                                  workspace, (hipStream_t)stream), "fill");
}
} // extern "C"
