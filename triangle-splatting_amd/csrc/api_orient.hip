// api_orient.hip -- the C ABI of include/ts_orient.h, the whole export list of libts_orient.so.  The library links none of the other api
// units, so the error text lives here: one buffer per thread, like the last-error text of the other ten libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_orient.h"
#pragma GCC visibility pop
#include "ts_orient_launch.h"

#include <cstdarg>
#include <cstdio>

namespace
{
thread_local char g_error[512] = "";
constexpr int32_t MAX_FACES = 715827882; // 3 F half-edges stay below 2^31; the sort's layout asks for no less (ts_manifold.h sorts as many records)

int orient_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int orient_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}
} // namespace

extern "C" {
const char *tsw_last_error(void) { return g_error; }

size_t tsw_workspace_bytes(int32_t V, int32_t F) { return ts_orient_workspace_bytes(V, F > MAX_FACES ? MAX_FACES : F); }

int tsw_orient(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, int32_t mode, int32_t *face_piece,
               uint8_t *face_flip, int32_t *out_faces, unsigned long long *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    if (V < 0 || F < 0) return orient_fail(TS2D_ERR_INVALID, "V and F must be >= 0, got %d and %d", (int)V, (int)F);
    if (F > MAX_FACES) return orient_fail(TS2D_ERR_CAPACITY, "F = %d exceeds %d faces", (int)F, (int)MAX_FACES);
    if (mode < 0 || mode > 2) return orient_fail(TS2D_ERR_INVALID, "mode must be 0 (anchor), 1 (majority) or 2 (volume), got %d", (int)mode);
    if (mode == 2 && V > 0 && !vertices) return orient_fail(TS2D_ERR_INVALID, "vertices is null with mode 2 (volume)");
    if (!counts) return orient_fail(TS2D_ERR_INVALID, "counts is null");
    if (F > 0)
    {
        if (!faces || !out_faces) return orient_fail(TS2D_ERR_INVALID, "faces/out_faces is null with F = %d", (int)F);
        if (!face_piece || !face_flip) return orient_fail(TS2D_ERR_INVALID, "face_piece/face_flip is null with F = %d", (int)F);
        if (V > 0)
        {
            if (!workspace) return orient_fail(TS2D_ERR_INVALID, "workspace is null");
            if (workspace_bytes < tsw_workspace_bytes(V, F))
                return orient_fail(TS2D_ERR_INVALID, "orient workspace too small: %zu < %zu", workspace_bytes, tsw_workspace_bytes(V, F));
        }
    }
    const hipError_t e = ts_orient_faces(V, F, vertices, faces, keep, mode, face_piece, face_flip, out_faces, counts, workspace, (hipStream_t)stream);
    return e == hipSuccess ? TS2D_OK : orient_fail(TS2D_ERR_HIP, "orient: %s", hipGetErrorString(e));
}
} // extern "C"
