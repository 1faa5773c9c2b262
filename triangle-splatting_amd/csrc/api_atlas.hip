// api_atlas.hip -- the C ABI of include/ts_atlas.h, the whole export list of libts_atlas.so.  The library links none of the other api
// units, so the error text lives here: one buffer per thread, like the last-error text of the other libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_atlas.h"
#pragma GCC visibility pop
#include "ts_atlas_launch.h"

#include <cstdarg>
#include <cstdio>

namespace
{
thread_local char g_error[512] = "";
constexpr long long INT_LIMIT = 0x7fffffffll;

int atlas_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int atlas_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

int positive_ok(const char *name, float v)
{
    if (!(v > 0.0f) || !(v <= 3.402823466e+38f)) return atlas_fail(TS2D_ERR_INVALID, "%s must be finite and > 0, got %g", name, (double)v);
    return TS2D_OK;
}

int image_ok(int32_t W, int32_t H)
{
    if (W < 1 || H < 1) return atlas_fail(TS2D_ERR_INVALID, "W and H must be >= 1, got %d x %d", (int)W, (int)H);
    if ((long long)W * (long long)H > INT_LIMIT) return atlas_fail(TS2D_ERR_CAPACITY, "an image of %d x %d pixels exceeds 2^31 - 1", (int)W, (int)H);
    return TS2D_OK;
}

// F >= 0, 1 <= R <= 64, F T <= 2^31 - 1
int texels_ok(int32_t F, int32_t R)
{
    if (F < 0) return atlas_fail(TS2D_ERR_INVALID, "F must be >= 0, got %d", (int)F);
    if (R < 1 || R > TSA_MAX_RES) return atlas_fail(TS2D_ERR_INVALID, "R must lie in [1, %d], got %d", TSA_MAX_RES, (int)R);
    if ((long long)F * (long long)(R * (R + 1) / 2) > INT_LIMIT)
        return atlas_fail(TS2D_ERR_CAPACITY, "%d faces of %d texels exceed 2^31 - 1 texels", (int)F, (int)(R * (R + 1) / 2));
    return TS2D_OK;
}

// Cx >= 1, Cy >= 1, Cx Cy >= ceil(F / 2), Wa Ha <= 2^31 - 1 (F and R already checked)
int layout_ok(int32_t F, int32_t R, int32_t Cx, long long Cy)
{
    const long long K = ((long long)F + 1) / 2;
    if (Cx < 1 || Cy < 1) return atlas_fail(TS2D_ERR_INVALID, "Cx and Cy must be >= 1, got %d and %lld", (int)Cx, Cy);
    if (Cy > INT_LIMIT || (long long)Cx * (long long)(R + 1) > INT_LIMIT || Cy * (long long)R > INT_LIMIT ||
        (long long)Cx * (long long)(R + 1) > INT_LIMIT / (Cy * (long long)R))
        return atlas_fail(TS2D_ERR_CAPACITY, "an atlas of %d x %lld cells of %d x %d texels exceeds 2^31 - 1 texels", (int)Cx, Cy, (int)R + 1, (int)R);
    if ((long long)Cx * Cy < K) return atlas_fail(TS2D_ERR_INVALID, "%d x %lld cells do not hold %d faces", (int)Cx, Cy, (int)F);
    return TS2D_OK;
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : atlas_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tsa_last_error(void) { return g_error; }

int tsa_texel_index(const float *view, float tan_fovx, float tan_fovy, int32_t W, int32_t H, int32_t V, const float *vertices, int32_t F,
                    const int32_t *faces, const int32_t *face_idx, int32_t R, int32_t Cx, int32_t *texel_idx, int32_t *atlas_idx, float *bary,
                    void *stream)
{
    if (int rc = positive_ok("tan_fovx", tan_fovx)) return rc;
    if (int rc = positive_ok("tan_fovy", tan_fovy)) return rc;
    if (int rc = image_ok(W, H)) return rc;
    if (V < 0) return atlas_fail(TS2D_ERR_INVALID, "V must be >= 0, got %d", (int)V);
    if (int rc = texels_ok(F, R)) return rc;
    if (Cx < 1) return atlas_fail(TS2D_ERR_INVALID, "Cx must be >= 1, got %d", (int)Cx);
    const long long K = ((long long)F + 1) / 2, rows = (K + Cx - 1) / Cx;
    if (int rc = layout_ok(F, R, Cx, rows > 1 ? rows : 1)) return rc;
    if (!view || !face_idx || !texel_idx) return atlas_fail(TS2D_ERR_INVALID, "view/face_idx/texel_idx is null");
    if (V > 0 && !vertices) return atlas_fail(TS2D_ERR_INVALID, "vertices is null with V = %d", (int)V);
    if (F > 0 && !faces) return atlas_fail(TS2D_ERR_INVALID, "faces is null with F = %d", (int)F);
    return enqueued(ts_atlas_texel_index(view, tan_fovx, tan_fovy, W, H, V, vertices, F, faces, face_idx, R, Cx, texel_idx, atlas_idx, bary,
                                         (hipStream_t)stream), "texel_index");
}

int tsa_face_totals(int32_t F, int32_t R, const unsigned long long *texels, unsigned long long *face_totals, void *stream)
{
    if (int rc = texels_ok(F, R)) return rc;
    if (F > 0 && (!texels || !face_totals)) return atlas_fail(TS2D_ERR_INVALID, "texels/face_totals is null with F = %d", (int)F);
    return enqueued(ts_atlas_face_totals(F, R, texels, face_totals, (hipStream_t)stream), "face_totals");
}

int tsa_resolve(int32_t F, int32_t R, int32_t Cx, int32_t Cy, const unsigned long long *texels, const unsigned long long *face_totals,
                int32_t min_count, const float *face_fallback, const float *fill, float *image, uint8_t *state, uint8_t *rgb8, void *stream)
{
    if (int rc = texels_ok(F, R)) return rc;
    if (int rc = layout_ok(F, R, Cx, Cy)) return rc;
    if (min_count < 1) return atlas_fail(TS2D_ERR_INVALID, "min_count must be >= 1, got %d", (int)min_count);
    if (!fill || !image || !state) return atlas_fail(TS2D_ERR_INVALID, "fill/image/state is null");
    if (F > 0 && (!texels || !face_totals)) return atlas_fail(TS2D_ERR_INVALID, "texels/face_totals is null with F = %d", (int)F);
    return enqueued(ts_atlas_resolve(F, R, Cx, Cy, texels, face_totals, min_count, face_fallback, fill[0], fill[1], fill[2], image, state, rgb8,
                                     (hipStream_t)stream), "resolve");
}

int tsa_render(int32_t W, int32_t H, int32_t Wa, int32_t Ha, const int32_t *atlas_idx, const float *image, const float *background, float *out,
               void *stream)
{
    if (int rc = image_ok(W, H)) return rc;
    if (Wa < 1 || Ha < 1) return atlas_fail(TS2D_ERR_INVALID, "Wa and Ha must be >= 1, got %d x %d", (int)Wa, (int)Ha);
    if ((long long)Wa * (long long)Ha > INT_LIMIT) return atlas_fail(TS2D_ERR_CAPACITY, "an atlas of %d x %d texels exceeds 2^31 - 1", (int)Wa, (int)Ha);
    if (!atlas_idx || !image || !background || !out) return atlas_fail(TS2D_ERR_INVALID, "atlas_idx/image/background/out is null");
    return enqueued(ts_atlas_render(W, H, Wa, Ha, atlas_idx, image, background, out, (hipStream_t)stream), "render");
}
} // extern "C"
