// mesh_census.hip -- the per-face census over a face_idx image of the opaque mesh renderer (include/ts_mesh.h: ts2d_mesh_census_add).
//
// For every counted pixel the row of its face gains {1, q(r), q(g), q(b)}, q = the target's channel in Q16 fixed point.  Every sum is an
// integer, so the accumulator after any number of views is a pure function of the inputs: no arrival order, wave order or view order shows.
//
// Shape: a linear sweep, one pixel per lane, 256 pixels per workgroup; the four planes (face_idx, three target planes, optionally the mask)
// are read as whole 256-byte wave rows.  Neighbouring pixels of an image row mostly share a face, so equal-index runs are combined inside the
// wavefront first:
//   1. a lane is a run's head when its left neighbour holds another key (key = the face, or -1 for a pixel that is not counted);
//   2. every lane learns where its run ends from the ballot of the heads, and a segmented suffix sum over 1, 2, ... 32 lanes leaves the run's
//      three Q16 sums in its head (at most 64 x 65536 = 2^22: 32-bit arithmetic); the run's pixel count is its length, no sum needed;
//   3. the heads of counted runs leave {count, r, g, b} and the face in the wavefront's LDS slots, compacted by their rank among the heads;
//   4. the wavefront then issues the 64-bit atomics FOUR LANES PER RUN, lane 4 h + w adding word w of run h: a run's row is one aligned
//      32-byte segment of one wave-instruction instead of four instructions with one 8-byte word per row each (the memory side executes
//      atomics per 64-byte request; one lane per row is the slowest shape the float-atomic measurements know).  Zero words are not sent.
// Runs that straddle two wavefronts or two image rows are simply two runs.  No float atomics, no ordered hand-off, no scratch.
#include "ts2d_common.h"
#include "ts2d_wave.h"

namespace
{
// Q16 of a target channel: clamp to [0, 1] (a NaN counts as 0), times 2^16 (exact in fp32), round to nearest even.
__device__ __forceinline__ uint32_t census_q16(float c)
{
    const float x = c > 0.0f ? fminf(c, 1.0f) : 0.0f; // NaN > 0 is false
    return (uint32_t)rintf(x * 65536.0f);
}

__global__ void __launch_bounds__(256) mesh_census_kernel(size_t npix, int F, const int32_t *__restrict__ face_idx,
                                                          const float *__restrict__ target, const float *__restrict__ pixel_mask,
                                                          unsigned long long *census)
{
    __shared__ uint32_t s_sum[4][64 * 4];
    __shared__ int32_t s_face[4][64];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const size_t p = (size_t)blockIdx.x * 256 + t;
    int32_t key = -1;
    uint32_t r = 0, g = 0, b = 0;
    if (p < npix)
    {
        const int32_t f = face_idx[p];
        if ((uint32_t)f < (uint32_t)F && (!pixel_mask || pixel_mask[p] > 0.0f)) // the only indices that ever address the census
        {
            key = f;
            if (target)
            {
                r = census_q16(target[p]);
                g = census_q16(target[npix + p]);
                b = census_q16(target[2 * npix + p]);
            }
        }
    }
    const int32_t left = __shfl_up(key, 1);
    const bool head = lane == 0 || left != key;
    const uint64_t heads = __ballot(head);
    const uint64_t after = lane == 63 ? 0ull : heads >> (lane + 1);
    const int end = after ? lane + 1 + __builtin_ctzll(after) : 64; // one past the run's last lane
    if (target) // wave-uniform
    {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1)
        {
            const uint32_t tr = __shfl_down(r, d), tg = __shfl_down(g, d), tb = __shfl_down(b, d);
            if (lane + d < end) { r += tr; g += tg; b += tb; } // lane + d lies in this run and holds the sum of [lane + d, min(lane + 2 d, end))
        }
    }
    const bool emit = head && key >= 0;
    const uint64_t emits = __ballot(emit);
    if (emits == 0ull) return; // wave-uniform; the kernel has no workgroup barrier
    if (emit)
    {
        const int slot = __popcll(emits & ((1ull << lane) - 1ull));
        uint32_t *o = s_sum[wave] + 4 * slot;
        o[0] = (uint32_t)(end - lane); o[1] = r; o[2] = g; o[3] = b;
        s_face[wave][slot] = key;
    }
    wave_lds_order();
    const int n = 4 * __popcll(emits);
    for (int i = lane; i < n; i += 64)
    {
        const uint32_t v = s_sum[wave][i];
        if (v) __hip_atomic_fetch_add(census + 4 * (size_t)s_face[wave][i >> 2] + (i & 3), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
} // namespace

void ts_launch_mesh_census(int W, int H, int F, const int32_t *face_idx, const float *target, const float *pixel_mask, unsigned long long *census,
                           hipStream_t s)
{
    const size_t npix = (size_t)W * (size_t)H;
    if (F <= 0 || npix == 0) return;
    hipLaunchKernelGGL(mesh_census_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, npix, F, face_idx, target, pixel_mask, census);
}
