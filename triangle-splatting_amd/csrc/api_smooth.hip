// api_smooth.hip -- the C ABI of include/ts_smooth.h, the whole export list of libts_smooth.so.  The library links none of the other api
// units, so the error text lives here: one buffer per thread, like the last-error text of the other seven libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_smooth.h"
#pragma GCC visibility pop
#include "ts_smooth_launch.h"

#include <cstdarg>
#include <cstdio>

namespace
{
thread_local char g_error[512] = "";
constexpr int32_t MAX_FACES = 357913941; // 6 F adjacency slots stay below 2^31

int smooth_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int smooth_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

bool finite_f(float v) { return v >= -3.402823466e+38f && v <= 3.402823466e+38f; }

int counts_ok(int32_t V, int32_t F)
{
    if (V < 0 || F < 0) return smooth_fail(TS2D_ERR_INVALID, "V and F must be >= 0, got %d and %d", (int)V, (int)F);
    if (F > MAX_FACES) return smooth_fail(TS2D_ERR_CAPACITY, "F = %d exceeds %d faces", (int)F, (int)MAX_FACES);
    return TS2D_OK;
}

int workspace_ok(int32_t V, int32_t F, const void *workspace, size_t workspace_bytes)
{
    if (!workspace) return smooth_fail(TS2D_ERR_INVALID, "workspace is null");
    if (workspace_bytes < tss_workspace_bytes(V, F))
        return smooth_fail(TS2D_ERR_INVALID, "smooth workspace too small: %zu < %zu", workspace_bytes, tss_workspace_bytes(V, F));
    return TS2D_OK;
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : smooth_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tss_last_error(void) { return g_error; }

size_t tss_workspace_bytes(int32_t V, int32_t F) { return ts_smooth_workspace_bytes(V, F > MAX_FACES ? MAX_FACES : F); }

int tss_adjacency(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep, int32_t *offsets, int32_t *neighbors, int32_t *edge_faces,
                  uint8_t *vertex_class, unsigned long long *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = counts_ok(V, F)) return rc;
    if (!counts) return smooth_fail(TS2D_ERR_INVALID, "counts is null");
    if (V > 0)
    {
        if (!offsets || !vertex_class) return smooth_fail(TS2D_ERR_INVALID, "offsets/vertex_class is null");
        if (F > 0)
        {
            if (!faces || !neighbors || !edge_faces) return smooth_fail(TS2D_ERR_INVALID, "faces/neighbors/edge_faces is null with F = %d", (int)F);
            if (int rc = workspace_ok(V, F, workspace, workspace_bytes)) return rc;
        }
    }
    return enqueued(ts_smooth_adjacency(V, F, faces, keep, offsets, neighbors, edge_faces, vertex_class, counts, workspace, (hipStream_t)stream),
                    "adjacency");
}

int tss_smooth(int32_t V, const float *vertices, const int32_t *offsets, const int32_t *neighbors, const int32_t *edge_faces, int32_t num_entries,
               const uint8_t *vertex_class, const uint8_t *pinned, float lambda, float mu, int32_t iterations, int32_t boundary_mode,
               float max_move, float *out_vertices, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = counts_ok(V, 0)) return rc;
    if (num_entries < 0) return smooth_fail(TS2D_ERR_INVALID, "num_entries must be >= 0, got %d", (int)num_entries);
    if (!finite_f(lambda) || !finite_f(mu)) return smooth_fail(TS2D_ERR_INVALID, "lambda and mu must be finite, got %g and %g", (double)lambda, (double)mu);
    if (iterations < 0) return smooth_fail(TS2D_ERR_INVALID, "iterations must be >= 0, got %d", (int)iterations);
    if (!(max_move >= 0.0f)) return smooth_fail(TS2D_ERR_INVALID, "max_move must be >= 0 (+inf: no bound), got %g", (double)max_move);
    if (boundary_mode != TSS_BOUNDARY_FIXED && boundary_mode != TSS_BOUNDARY_CURVE && boundary_mode != TSS_BOUNDARY_FREE)
        return smooth_fail(TS2D_ERR_INVALID, "boundary_mode must be TSS_BOUNDARY_FIXED, _CURVE or _FREE, got %d", (int)boundary_mode);
    if (V == 0) return TS2D_OK;
    if (!vertices || !offsets || !vertex_class || !out_vertices) return smooth_fail(TS2D_ERR_INVALID, "vertices/offsets/vertex_class/out_vertices is null");
    if (num_entries > 0 && !neighbors) return smooth_fail(TS2D_ERR_INVALID, "neighbors is null with num_entries = %d", (int)num_entries);
    if (num_entries > 0 && boundary_mode == TSS_BOUNDARY_CURVE && !edge_faces)
        return smooth_fail(TS2D_ERR_INVALID, "edge_faces is null in TSS_BOUNDARY_CURVE");
    if (vertices == out_vertices) return smooth_fail(TS2D_ERR_INVALID, "out_vertices may not alias vertices");
    if (int rc = workspace_ok(V, 0, workspace, workspace_bytes)) return rc;
    return enqueued(ts_smooth_smooth(V, vertices, offsets, neighbors, edge_faces, num_entries, vertex_class, pinned, lambda, mu, iterations,
                                     boundary_mode, max_move, out_vertices, workspace, (hipStream_t)stream), "smooth");
}

int tss_face_normals(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, float *face_normal,
                     uint8_t *face_valid, void *stream)
{
    if (int rc = counts_ok(V, F)) return rc;
    if (F == 0) return TS2D_OK;
    if (!faces || !face_normal || !face_valid) return smooth_fail(TS2D_ERR_INVALID, "faces/face_normal/face_valid is null");
    if (V > 0 && !vertices) return smooth_fail(TS2D_ERR_INVALID, "vertices is null");
    return enqueued(ts_smooth_face_normals(V, F, vertices, faces, keep, face_normal, face_valid, (hipStream_t)stream), "face_normals");
}

int tss_vertex_normals(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, int32_t weighting,
                       float *vertex_normal, uint8_t *vertex_valid, double *normal_sum, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = counts_ok(V, F)) return rc;
    if (weighting != TSS_NORMAL_AREA && weighting != TSS_NORMAL_UNIFORM)
        return smooth_fail(TS2D_ERR_INVALID, "weighting must be TSS_NORMAL_AREA or TSS_NORMAL_UNIFORM, got %d", (int)weighting);
    if (V == 0) return TS2D_OK;
    if (!vertices || !vertex_normal || !vertex_valid) return smooth_fail(TS2D_ERR_INVALID, "vertices/vertex_normal/vertex_valid is null");
    if (F > 0 && !faces) return smooth_fail(TS2D_ERR_INVALID, "faces is null with F = %d", (int)F);
    if (int rc = workspace_ok(V, F, workspace, workspace_bytes)) return rc;
    return enqueued(ts_smooth_vertex_normals(V, F, vertices, faces, keep, weighting, vertex_normal, vertex_valid, normal_sum, workspace,
                                             (hipStream_t)stream), "vertex_normals");
}
} // extern "C"
