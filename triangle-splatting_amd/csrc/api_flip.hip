// api_flip.hip -- the C ABI of include/ts_flip.h, the whole export list of libts_flip.so.  The library links none of the other api units, so
// the error text lives here: one buffer per thread, like the last-error text of the other libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_flip.h"
#pragma GCC visibility pop
#include "ts_flip_launch.h"

#include <cstdarg>
#include <cstdio>

namespace
{
thread_local char g_error[512] = "";
constexpr int32_t MAX_FACES = 536870911; // ts_subdivide.h's: what can be split can be flipped

int flip_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int flip_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}
} // namespace

extern "C" {
const char *tse_last_error(void) { return g_error; }

size_t tse_workspace_bytes(int32_t V, int32_t F) { return ts_flip_workspace_bytes(V, F > MAX_FACES ? MAX_FACES : F); }

int tse_flip(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, float min_cos, uint32_t seed,
             int32_t *out_faces, uint8_t *face_flipped, int32_t *edge_vertices, uint8_t *edge_state, int32_t *edge_opposite,
             unsigned long long *totals, void *workspace, size_t workspace_bytes, void *stream)
{
    if (V < 0 || F < 0) return flip_fail(TS2D_ERR_INVALID, "V and F must be >= 0, got %d and %d", (int)V, (int)F);
    if (F > MAX_FACES) return flip_fail(TS2D_ERR_CAPACITY, "F = %d exceeds %d faces: 3 F edges and 4 F faces must fit int32", (int)F, (int)MAX_FACES);
    if ((long long)V + 3LL * F > 2147483647LL)
        return flip_fail(TS2D_ERR_CAPACITY, "V + 3 F = %lld exceeds 2147483647, the capacity of the edge split", (long long)V + 3LL * F);
    if (!(min_cos >= -1.0f && min_cos <= 1.0f)) return flip_fail(TS2D_ERR_INVALID, "min_cos must lie in [-1, 1], got %g", (double)min_cos);
    if (!totals) return flip_fail(TS2D_ERR_INVALID, "totals is null");
    if (!out_faces != !face_flipped) return flip_fail(TS2D_ERR_INVALID, "out_faces and face_flipped must both be given or both be null");
    if (F > 0)
    {
        if (!faces) return flip_fail(TS2D_ERR_INVALID, "faces is null with F = %d", (int)F);
        if (!edge_vertices || !edge_state || !edge_opposite)
            return flip_fail(TS2D_ERR_INVALID, "edge_vertices/edge_state/edge_opposite is null with F = %d", (int)F);
        if (V > 0 && !vertices) return flip_fail(TS2D_ERR_INVALID, "vertices is null");
        if (!workspace) return flip_fail(TS2D_ERR_INVALID, "workspace is null");
        if (workspace_bytes < tse_workspace_bytes(V, F))
            return flip_fail(TS2D_ERR_INVALID, "flip workspace too small: %zu < %zu", workspace_bytes, tse_workspace_bytes(V, F));
    }
    const hipError_t e = ts_flip_round(V, F, vertices, faces, keep, min_cos, seed, out_faces, face_flipped, edge_vertices, edge_state,
                                       edge_opposite, totals, workspace, (hipStream_t)stream);
    return e == hipSuccess ? TS2D_OK : flip_fail(TS2D_ERR_HIP, "flip: %s", hipGetErrorString(e));
}
} // extern "C"
