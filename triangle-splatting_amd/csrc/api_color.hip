// api_color.hip -- the C ABI of include/ts_color.h, the whole export list of libts_color.so.  The library links none of the other api
// units, so the error text lives here: one buffer per thread, like the last-error text of the other five libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_color.h"
#pragma GCC visibility pop
#include "ts_color_launch.h"

#include <cstdarg>
#include <cstdio>

namespace
{
thread_local char g_error[512] = "";

int col_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int col_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

// the grid: every dimension at least 1, at most TSC_MAX_SAMPLES samples in all
int grid_ok(int32_t nx, int32_t ny, int32_t nz)
{
    if (nx < 1 || ny < 1 || nz < 1) return col_fail(TS2D_ERR_INVALID, "nx, ny, nz must be >= 1, got %d x %d x %d", (int)nx, (int)ny, (int)nz);
    if ((unsigned long long)nx * (unsigned long long)ny > (unsigned long long)TSC_MAX_SAMPLES ||
        (unsigned long long)nx * (unsigned long long)ny * (unsigned long long)nz > (unsigned long long)TSC_MAX_SAMPLES)
        return col_fail(TS2D_ERR_CAPACITY, "a grid of %d x %d x %d samples exceeds 2^27", (int)nx, (int)ny, (int)nz);
    return TS2D_OK;
}

int positive_ok(const char *name, float v)
{
    if (!(v > 0.0f) || !(v <= 3.402823466e+38f)) return col_fail(TS2D_ERR_INVALID, "%s must be finite and > 0, got %g", name, (double)v);
    return TS2D_OK;
}

int image_ok(int32_t W, int32_t H)
{
    if (W < 1 || H < 1) return col_fail(TS2D_ERR_INVALID, "W and H must be >= 1, got %d x %d", (int)W, (int)H);
    if ((long long)W * (long long)H > 0x7fffffffll) return col_fail(TS2D_ERR_CAPACITY, "an image of %d x %d pixels exceeds 2^31 - 1", (int)W, (int)H);
    return TS2D_OK;
}

int channels_ok(int32_t C)
{
    if (C < 1 || C > TSC_MAX_CHANNELS) return col_fail(TS2D_ERR_INVALID, "C must lie in [1, %d], got %d", TSC_MAX_CHANNELS, (int)C);
    return TS2D_OK;
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : col_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tsc_last_error(void) { return g_error; }

int tsc_integrate(int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz, float h, float trunc, const float *view, float tan_fovx,
                  float tan_fovy, int32_t W, int32_t H, const float *depth, const uint8_t *mask, const float *image, int64_t *csum,
                  int32_t *cweight, unsigned long long *updated, void *stream)
{
    if (int rc = grid_ok(nx, ny, nz)) return rc;
    if (int rc = positive_ok("h", h)) return rc;
    if (int rc = positive_ok("trunc", trunc)) return rc;
    if (int rc = positive_ok("tan_fovx", tan_fovx)) return rc;
    if (int rc = positive_ok("tan_fovy", tan_fovy)) return rc;
    if (int rc = image_ok(W, H)) return rc;
    if (!view || !depth || !image || !csum || !cweight) return col_fail(TS2D_ERR_INVALID, "view/depth/image/csum/cweight is null");
    return enqueued(ts_color_integrate(nx, ny, nz, ox, oy, oz, h, trunc, view, tan_fovx, tan_fovy, W, H, depth, mask, image, (long long *)csum, cweight,
                                       updated, (hipStream_t)stream), "integrate");
}

int tsc_color_field(int32_t nx, int32_t ny, int32_t nz, const int64_t *csum, const int32_t *cweight, int32_t min_weight, float *field, void *stream)
{
    if (int rc = grid_ok(nx, ny, nz)) return rc;
    if (min_weight < 1) return col_fail(TS2D_ERR_INVALID, "min_weight must be >= 1, got %d", (int)min_weight);
    if (!csum || !cweight || !field) return col_fail(TS2D_ERR_INVALID, "csum/cweight/field is null");
    return enqueued(ts_color_field(nx * ny * nz, (const long long *)csum, cweight, min_weight, field, (hipStream_t)stream), "color_field");
}

int tsc_sample(int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz, float h, int32_t C, const float *grid, int32_t N,
               const float *points, float *out, uint8_t *valid, void *stream)
{
    if (int rc = grid_ok(nx, ny, nz)) return rc;
    if (int rc = positive_ok("h", h)) return rc;
    if (int rc = channels_ok(C)) return rc;
    if (N < 0) return col_fail(TS2D_ERR_INVALID, "N must be >= 0, got %d", (int)N);
    if (N == 0) return TS2D_OK;
    if (!grid || !points || !out || !valid) return col_fail(TS2D_ERR_INVALID, "grid/points/out/valid is null");
    return enqueued(ts_color_sample(nx, ny, nz, ox, oy, oz, h, C, grid, N, points, out, valid, (hipStream_t)stream), "sample");
}

int tsc_interpolate(const float *view, float tan_fovx, float tan_fovy, int32_t W, int32_t H, int32_t V, const float *vertices, int32_t F,
                    const int32_t *faces, const int32_t *face_idx, int32_t C, const float *attributes, const float *background, float *out,
                    float *bary, void *stream)
{
    if (int rc = positive_ok("tan_fovx", tan_fovx)) return rc;
    if (int rc = positive_ok("tan_fovy", tan_fovy)) return rc;
    if (int rc = image_ok(W, H)) return rc;
    if (int rc = channels_ok(C)) return rc;
    if (V < 0 || F < 0) return col_fail(TS2D_ERR_INVALID, "V and F must be >= 0, got %d and %d", (int)V, (int)F);
    if (!view || !face_idx || !background || !out) return col_fail(TS2D_ERR_INVALID, "view/face_idx/background/out is null");
    if (V > 0 && (!vertices || !attributes)) return col_fail(TS2D_ERR_INVALID, "vertices/attributes is null with V = %d", (int)V);
    if (F > 0 && !faces) return col_fail(TS2D_ERR_INVALID, "faces is null with F = %d", (int)F);
    return enqueued(ts_color_interpolate(view, tan_fovx, tan_fovy, W, H, V, vertices, F, faces, face_idx, C, attributes, background, out, bary,
                                         (hipStream_t)stream), "interpolate");
}
} // extern "C"
