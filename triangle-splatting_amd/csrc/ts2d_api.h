// ts2d_api.h -- what the C ABI files (api.hip, api_loss.hip, api_model.hip, api_mesh.hip) share, and nothing else includes: the error
// string and the per-kernel profiler behind every entry point, the early read-back of the instance count and the ordering chain that the
// rasterizer and the opaque mesh renderer both run.  Everything here is internal (the library is built with -fvisibility=hidden) and is
// defined ONCE, in api.hip.  Include it after the public headers the file implements (those go inside #pragma GCC visibility push(default)).
#ifndef TS2D_API_H
#define TS2D_API_H

#include "../../include/ts2d.h"
#include "ts2d_common.h"

#pragma GCC visibility push(hidden)
// Stores the formatted message as the calling thread's ts2d_last_error() and returns `code`.
int ts_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define TS_HIP(expr)                                                                                                   \
    do                                                                                                                 \
    {                                                                                                                  \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess) return ts_fail(TS2D_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));           \
    } while (0)

// R2D's CHECK_CUDA(debug) (auxiliary.h:358-367): with the debug flag, synchronise and surface errors per kernel.
#define TS_CHECK(flags, stream, what)                                                                                  \
    do                                                                                                                 \
    {                                                                                                                  \
        hipError_t e_ = hipGetLastError();                                                                             \
        if (e_ == hipSuccess && ((flags)&TS2D_FLAG_DEBUG)) e_ = hipStreamSynchronize(stream);                          \
        if (e_ != hipSuccess) return ts_fail(TS2D_ERR_HIP, "%s: %s", what, hipGetErrorString(e_));                     \
    } while (0)

// Optional per-kernel timing with HIP events on the caller's stream (ts2d_profile_*): a scope is one row of the table, by name.
struct ProfScope
{
    hipStream_t s;
    int row = -1;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(const char *name, hipStream_t stream);
    ~ProfScope();
};

// Early read-back of the instance count (ts2d_radix.h, publish_instance_count): a pinned host word + an event per call in flight
struct EarlyCount
{
    unsigned long long *host = nullptr;
    hipEvent_t ev = nullptr;
};
bool acquire_early_count(EarlyCount &e);
// The instance count of a forward whose triangle half is queued on `s`, for the host: the early read-back (early != nullptr) or, when there is
// no pinned word (allocation refused), a copy behind everything that was queued -- slower, same results.  Stored in *num_rendered.
int wait_instance_count(int P, const ts2d_state *state, const EarlyCount *early, hipStream_t s, int64_t *num_rendered);

// ---- the ordering chain, behind a renderer's own per-triangle kernel and in front of its per-pixel kernel ------------------------------
// Triangle half: depth census (publishes the instance count to early->host), the event behind it, depth sort, scan of the instance offsets.
int ts_order_triangles(uint32_t flags, const GeometryStateView &g, int P, const EarlyCount *early, hipStream_t s);
// Instance half: emission of the (tile, value) pairs -- with P == 0 nobody else clears the tile ranges, so they are zeroed instead -- then,
// for N > 0 instance slots, the tile sort and the tile ranges.  n_dev != nullptr: the count is known on the device only and N is the capacity
// the binning state was carved for.  contrib_sum / contrib_max: cleared by the emission kernel when given.
int ts_order_instances(uint32_t flags, int P, int grid_x, int ntiles, const GeometryStateView &g, const BinningStateView &b, const ImageStateView &im,
                       float *contrib_sum, float *contrib_max, int64_t N, const unsigned long long *n_dev, const QuadMaskArgs &quad, hipStream_t s);

#pragma GCC visibility pop
#endif // TS2D_API_H
