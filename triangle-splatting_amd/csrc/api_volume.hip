// api_volume.hip -- the C ABI of include/ts_volume.h, the whole export list of libts_volume.so.  The library links none of the other api
// units, so the error text lives here: one buffer per thread, like the last-error text of the other four libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_volume.h"
#pragma GCC visibility pop
#include "ts_volume_launch.h"

#include <cstdarg>
#include <cstdio>

namespace
{
thread_local char g_error[512] = "";

int vol_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int vol_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

// the grid: every dimension at least 1, at most TSV_MAX_SAMPLES samples in all
int grid_ok(int32_t nx, int32_t ny, int32_t nz)
{
    if (nx < 1 || ny < 1 || nz < 1) return vol_fail(TS2D_ERR_INVALID, "nx, ny, nz must be >= 1, got %d x %d x %d", (int)nx, (int)ny, (int)nz);
    if ((unsigned long long)nx * (unsigned long long)ny > (unsigned long long)TSV_MAX_SAMPLES ||
        (unsigned long long)nx * (unsigned long long)ny * (unsigned long long)nz > (unsigned long long)TSV_MAX_SAMPLES)
        return vol_fail(TS2D_ERR_CAPACITY, "a grid of %d x %d x %d samples exceeds 2^27", (int)nx, (int)ny, (int)nz);
    return TS2D_OK;
}

int positive_ok(const char *name, float v)
{
    if (!(v > 0.0f) || !(v <= 3.402823466e+38f)) return vol_fail(TS2D_ERR_INVALID, "%s must be finite and > 0, got %g", name, (double)v);
    return TS2D_OK;
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : vol_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tsv_last_error(void) { return g_error; }

int tsv_integrate(int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz, float h, float trunc, const float *view, float tan_fovx,
                  float tan_fovy, int32_t W, int32_t H, const float *depth, const uint8_t *mask, int32_t flags, int64_t *sum, int32_t *weight,
                  unsigned long long *updated, void *stream)
{
    if (int rc = grid_ok(nx, ny, nz)) return rc;
    if (int rc = positive_ok("h", h)) return rc;
    if (int rc = positive_ok("trunc", trunc)) return rc;
    if (int rc = positive_ok("tan_fovx", tan_fovx)) return rc;
    if (int rc = positive_ok("tan_fovy", tan_fovy)) return rc;
    if (W < 1 || H < 1) return vol_fail(TS2D_ERR_INVALID, "W and H must be >= 1, got %d x %d", (int)W, (int)H);
    if ((long long)W * (long long)H > 0x7fffffffll) return vol_fail(TS2D_ERR_CAPACITY, "an image of %d x %d pixels exceeds 2^31 - 1", (int)W, (int)H);
    if (flags & ~TSV_CARVE_UNCOVERED) return vol_fail(TS2D_ERR_INVALID, "flags must be 0 or TSV_CARVE_UNCOVERED, got %d", (int)flags);
    if (!view || !depth || !sum || !weight) return vol_fail(TS2D_ERR_INVALID, "view/depth/sum/weight is null");
    return enqueued(ts_volume_integrate(nx, ny, nz, ox, oy, oz, h, trunc, view, tan_fovx, tan_fovy, W, H, depth, mask, flags & TSV_CARVE_UNCOVERED,
                                        (long long *)sum, weight, updated, (hipStream_t)stream), "integrate");
}

int tsv_field(int32_t nx, int32_t ny, int32_t nz, const int64_t *sum, const int32_t *weight, int32_t min_weight, float *field, void *stream)
{
    if (int rc = grid_ok(nx, ny, nz)) return rc;
    if (min_weight < 1) return vol_fail(TS2D_ERR_INVALID, "min_weight must be >= 1, got %d", (int)min_weight);
    if (!sum || !weight || !field) return vol_fail(TS2D_ERR_INVALID, "sum/weight/field is null");
    return enqueued(ts_volume_field(nx * ny * nz, (const long long *)sum, weight, min_weight, field, (hipStream_t)stream), "field");
}

size_t tsv_extract_workspace_bytes(int32_t nx, int32_t ny, int32_t nz)
{
    if (nx < 1 || ny < 1 || nz < 1) return ts_volume_extract_workspace_bytes(0);
    return ts_volume_extract_workspace_bytes((size_t)nx * (size_t)ny * (size_t)nz);
}

int tsv_extract(int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz, float h, const float *field, float iso, int64_t capacity,
                float *triangles, int32_t *cell, int64_t *total, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = grid_ok(nx, ny, nz)) return rc;
    if (int rc = positive_ok("h", h)) return rc;
    if (!(iso >= -3.402823466e+38f && iso <= 3.402823466e+38f)) return vol_fail(TS2D_ERR_INVALID, "iso must be finite, got %g", (double)iso);
    if (capacity < 0) return vol_fail(TS2D_ERR_INVALID, "capacity must be >= 0, got %lld", (long long)capacity);
    if (!field || !total) return vol_fail(TS2D_ERR_INVALID, "field/total is null");
    if (capacity > 0 && !triangles) return vol_fail(TS2D_ERR_INVALID, "triangles is null with capacity %lld", (long long)capacity);
    if (!workspace) return vol_fail(TS2D_ERR_INVALID, "workspace is null");
    if (workspace_bytes < tsv_extract_workspace_bytes(nx, ny, nz))
        return vol_fail(TS2D_ERR_INVALID, "extract workspace too small: %zu < %zu", workspace_bytes, tsv_extract_workspace_bytes(nx, ny, nz));
    return enqueued(ts_volume_extract(nx, ny, nz, ox, oy, oz, h, field, iso, (long long)capacity, triangles, cell, (long long *)total, workspace,
                                      (hipStream_t)stream), "extract");
}
} // extern "C"
