// api_overlap.hip -- the C ABI of include/ts_overlap.h, the whole export list of libts_overlap.so.  The library links none of the other api
// units, so the error text lives here: one buffer per thread, like the last-error text of the other libraries.
#pragma GCC visibility push(default)
#include "../../include/ts_overlap.h"
#pragma GCC visibility pop
#include "ts_overlap_launch.h"

#include <cstdarg>
#include <cstdio>

#define TSX_MAX_COUNT (0x7fffffff - 1024) /* the launchers round counts up to whole workgroups of up to 1024 in 32-bit integers */

namespace
{
thread_local char g_error[512] = "";

int overlap_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int overlap_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

int count_ok(const char *name, int32_t n)
{
    if (n < 0) return overlap_fail(TS2D_ERR_INVALID, "%s must be >= 0", name);
    if (n > TSX_MAX_COUNT) return overlap_fail(TS2D_ERR_INVALID, "%s must be at most %d", name, TSX_MAX_COUNT);
    return TS2D_OK;
}

int index_ok(const char *name, int32_t F, const void *bvh, size_t bvh_bytes)
{
    if (F == 0) return TS2D_OK;
    if (!bvh) return overlap_fail(TS2D_ERR_INVALID, "%s is null", name);
    if (bvh_bytes < ts_overlap_bvh_bytes(F))
        return overlap_fail(TS2D_ERR_INVALID, "%s too small: %zu < %zu", name, bvh_bytes, ts_overlap_bvh_bytes(F));
    return TS2D_OK;
}

int bits_ok(const char *name, int32_t bits)
{
    return bits >= 1 && bits <= 31 ? TS2D_OK : overlap_fail(TS2D_ERR_INVALID, "%s must lie in [1, 31], got %d", name, bits);
}

int enqueued(hipError_t e, const char *what)
{
    return e == hipSuccess ? TS2D_OK : overlap_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
} // namespace

extern "C" {
const char *tsx_last_error(void) { return g_error; }

size_t tsx_sort_workspace_bytes(int32_t P) { return ts_overlap_sort_workspace_bytes(P); }

int tsx_overlap(int32_t FA, const void *bvh_a, size_t bvh_a_bytes, const int32_t *faces, int32_t FB, const void *bvh_b, size_t bvh_b_bytes,
                int32_t *count_a, int32_t *count_b, uint64_t *stats, int32_t capacity, int32_t *pairs, uint8_t *kind,
                unsigned long long *leaf_visits, void *stream)
{
    if (int rc = count_ok("FA", FA)) return rc;
    if (int rc = count_ok("FB", FB)) return rc;
    if (int rc = count_ok("capacity", capacity)) return rc;
    if (faces && (bvh_b || FB != 0 || count_b))
        return overlap_fail(TS2D_ERR_INVALID, "self mode (faces given) takes no second mesh: bvh_b and count_b must be null and FB 0");
    if (!stats) return overlap_fail(TS2D_ERR_INVALID, "stats is null");
    if (FA > 0 && !count_a) return overlap_fail(TS2D_ERR_INVALID, "count_a is null");
    if (capacity > 0 && (!pairs || !kind)) return overlap_fail(TS2D_ERR_INVALID, "pairs/kind is null with capacity %d", capacity);
    if (int rc = index_ok("bvh_a", FA, bvh_a, bvh_a_bytes)) return rc;
    if (!faces)
        if (int rc = index_ok("bvh_b", FB, bvh_b, bvh_b_bytes)) return rc;
    return enqueued(ts_overlap_query(FA, bvh_a, faces, FB, bvh_b, count_a, count_b, stats, capacity, pairs, kind, leaf_visits, (hipStream_t)stream),
                    "overlap");
}

int tsx_sort_pairs(int32_t P, int32_t bits_first, int32_t bits_second, int32_t *pairs, uint8_t *kind, void *workspace, size_t workspace_bytes,
                   void *stream)
{
    if (int rc = count_ok("P", P)) return rc;
    if (int rc = bits_ok("bits_first", bits_first)) return rc;
    if (int rc = bits_ok("bits_second", bits_second)) return rc;
    if (P == 0) return TS2D_OK;
    if (!pairs || !kind) return overlap_fail(TS2D_ERR_INVALID, "pairs/kind is null");
    if (!workspace) return overlap_fail(TS2D_ERR_INVALID, "workspace is null");
    if (workspace_bytes < ts_overlap_sort_workspace_bytes(P))
        return overlap_fail(TS2D_ERR_INVALID, "sort workspace too small: %zu < %zu", workspace_bytes, ts_overlap_sort_workspace_bytes(P));
    return enqueued(ts_overlap_sort_pairs(P, bits_first, bits_second, pairs, kind, workspace, (hipStream_t)stream), "sort_pairs");
}
} // extern "C"
