// ts_knn_front.h -- the front half of the box searches: bounding box, 30-bit Morton codes, radix sort of (code, index), the sorted points
// gathered into a float4 array (xyz + original index) and the min/max box of every 1024 of them.  Shared by knn.hip (nearest neighbours,
// include/ts_knn.h) and mesh_weld.hip (the radius search of the vertex weld, include/ts_weld.h); every translation unit that includes it gets
// its own internal copy of the kernels.
//
// FINITE_ONLY = false is the reference's behaviour (SK = submodules/simple-knn/simple_knn.cu): every point enters the bounding box, whose
// reductions are seeded with the origin.  FINITE_ONLY = true (the weld) keeps a point with a NaN or infinite coordinate out of the bounding
// box and out of the 1024-point boxes, seeds nothing, and stores such a point as three NaNs in the sorted array, so that every distance
// test against it fails.
#pragma once
#include "ts2d_common.h"

#include <cfloat>

namespace
{
constexpr int BOX = 1024; // SK/auxiliary.h:3
constexpr int TPB = 256, PPT = BOX / TPB;

struct Box { float mnx, mny, mnz, mxx, mxy, mxz; };

__device__ __forceinline__ float block_reduce(float v, float *red, bool is_max)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        const float w = __shfl_xor(v, o);
        v = is_max ? fmaxf(v, w) : fminf(v, w);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int i = 1; i < TPB / 64; i++) r = is_max ? fmaxf(r, red[i]) : fminf(r, red[i]);
    return r;
}

__device__ __forceinline__ bool all_finite(float x, float y, float z)
{
    return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX; // false for NaN and for +-inf
}

// per-block partial bounding boxes of the raw points
template <bool FINITE_ONLY>
__global__ void __launch_bounds__(TPB) bbox_partial_kernel(int P, const float *__restrict__ pts, Box *__restrict__ partial)
{
    __shared__ float red[TPB / 64];
    Box me = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = blockIdx.x * TPB + threadIdx.x; i < P; i += gridDim.x * TPB)
    {
        const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        if (FINITE_ONLY && !all_finite(x, y, z)) continue;
        me.mnx = fminf(me.mnx, x); me.mny = fminf(me.mny, y); me.mnz = fminf(me.mnz, z);
        me.mxx = fmaxf(me.mxx, x); me.mxy = fmaxf(me.mxy, y); me.mxz = fmaxf(me.mxz, z);
    }
    Box r;
    r.mnx = block_reduce(me.mnx, red, false); r.mny = block_reduce(me.mny, red, false); r.mnz = block_reduce(me.mnz, red, false);
    r.mxx = block_reduce(me.mxx, red, true); r.mxy = block_reduce(me.mxy, red, true); r.mxz = block_reduce(me.mxz, red, true);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

template <bool FINITE_ONLY>
__global__ void __launch_bounds__(64) bbox_finish_kernel(int n, const Box *__restrict__ partial, Box *__restrict__ out)
{
    // the reductions of the reference start from init = {0, 0, 0} (SK:240,245,249): the box always contains the origin
    Box me = {0, 0, 0, 0, 0, 0};
    if (FINITE_ONLY) me = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = threadIdx.x; i < n; i += 64)
    {
        const Box b = partial[i];
        me.mnx = fminf(me.mnx, b.mnx); me.mny = fminf(me.mny, b.mny); me.mnz = fminf(me.mnz, b.mnz);
        me.mxx = fmaxf(me.mxx, b.mxx); me.mxy = fmaxf(me.mxy, b.mxy); me.mxz = fmaxf(me.mxz, b.mxz);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        me.mnx = fminf(me.mnx, __shfl_xor(me.mnx, o)); me.mny = fminf(me.mny, __shfl_xor(me.mny, o));
        me.mnz = fminf(me.mnz, __shfl_xor(me.mnz, o)); me.mxx = fmaxf(me.mxx, __shfl_xor(me.mxx, o));
        me.mxy = fmaxf(me.mxy, __shfl_xor(me.mxy, o)); me.mxz = fmaxf(me.mxz, __shfl_xor(me.mxz, o));
    }
    if (threadIdx.x == 0) *out = me;
}

__device__ __forceinline__ uint32_t prep_morton(uint32_t x) // SK:49-56
{
    x = (x | (x << 16)) & 0x030000FF;
    x = (x | (x << 8)) & 0x0300F00F;
    x = (x | (x << 4)) & 0x030C30C3;
    x = (x | (x << 2)) & 0x09249249;
    return x;
}

__device__ __forceinline__ uint32_t quantise(float v, float lo, float hi)
{
    const float t = ((v - lo) / (hi - lo)) * 1023.0f; // SK:60
    return (t >= 0.0f) ? (uint32_t)fminf(t, 4294967040.0f) : 0u; // NaN / negative -> 0 (CUDA float->uint saturation)
}

__global__ void __launch_bounds__(TPB) morton_kernel(int P, const float *__restrict__ pts, const Box *__restrict__ bb,
                                                      uint32_t *__restrict__ codes, uint32_t *__restrict__ ids)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= P) return;
    const Box b = *bb;
    const uint32_t x = prep_morton(quantise(pts[3 * (size_t)i], b.mnx, b.mxx));
    const uint32_t y = prep_morton(quantise(pts[3 * (size_t)i + 1], b.mny, b.mxy));
    const uint32_t z = prep_morton(quantise(pts[3 * (size_t)i + 2], b.mnz, b.mxz));
    codes[i] = x | (y << 1) | (z << 2); // SK:64
    ids[i] = (uint32_t)i;
}

// sorted points as float4 (xyz, original index bits) + the min/max box of every 1024 of them (SK:82-121)
template <bool FINITE_ONLY>
__global__ void __launch_bounds__(TPB) gather_boxes_kernel(int P, const float *__restrict__ pts, const uint32_t *__restrict__ ids_sorted,
                                                            float4 *__restrict__ sp, Box *__restrict__ boxes)
{
    __shared__ float red[TPB / 64];
    Box me = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
#pragma unroll
    for (int q = 0; q < PPT; q++)
    {
        const int i = blockIdx.x * BOX + q * TPB + threadIdx.x;
        if (i < P)
        {
            const uint32_t id = ids_sorted[i];
            const float x = pts[3 * (size_t)id], y = pts[3 * (size_t)id + 1], z = pts[3 * (size_t)id + 2];
            if (FINITE_ONLY && !all_finite(x, y, z))
            {
                const float nan = __uint_as_float(0x7FC00000u);
                sp[i] = make_float4(nan, nan, nan, __uint_as_float(id));
                continue;
            }
            sp[i] = make_float4(x, y, z, __uint_as_float(id));
            me.mnx = fminf(me.mnx, x); me.mny = fminf(me.mny, y); me.mnz = fminf(me.mnz, z);
            me.mxx = fmaxf(me.mxx, x); me.mxy = fmaxf(me.mxy, y); me.mxz = fmaxf(me.mxz, z);
        }
    }
    Box r;
    r.mnx = block_reduce(me.mnx, red, false); r.mny = block_reduce(me.mny, red, false); r.mnz = block_reduce(me.mnz, red, false);
    r.mxx = block_reduce(me.mxx, red, true); r.mxy = block_reduce(me.mxy, red, true); r.mxz = block_reduce(me.mxz, red, true);
    if (threadIdx.x == 0) boxes[blockIdx.x] = r;
}

struct KnnCarve
{
    uint32_t *codes, *codes_sorted, *ids, *ids_sorted;
    float4 *sp;
    Box *boxes, *partial, *bbox;
    void *sort_temp;
    size_t sort_temp_bytes, bytes;
    int nboxes, npartial;
};

KnnCarve knn_carve(void *ws, int P)
{
    KnnCarve c;
    const size_t n = (size_t)(P > 0 ? P : 0);
    c.nboxes = (int)((n + BOX - 1) / BOX);
    c.npartial = 256;
    char *p = (char *)ts_align_up((size_t)ws);
    auto take = [&](size_t bytes) { char *q = p; p += ts_align_up(bytes); return q; };
    c.codes = (uint32_t *)take(n * 4); c.codes_sorted = (uint32_t *)take(n * 4);
    c.ids = (uint32_t *)take(n * 4); c.ids_sorted = (uint32_t *)take(n * 4);
    c.sp = (float4 *)take(n * 16);
    c.boxes = (Box *)take((size_t)c.nboxes * sizeof(Box));
    c.partial = (Box *)take((size_t)c.npartial * sizeof(Box));
    c.bbox = (Box *)take(sizeof(Box));
    c.sort_temp_bytes = ts_radix_scratch_bytes(n); // the hand-written radix sort of radix_sort.hip
    c.sort_temp = take(c.sort_temp_bytes);
    c.bytes = (size_t)(p - (char *)ws);
    return c;
}

template <bool FINITE_ONLY>
hipError_t knn_prepare(int P, const float *points, const KnnCarve &c, hipStream_t s)
{
    hipLaunchKernelGGL(bbox_partial_kernel<FINITE_ONLY>, dim3(c.npartial), dim3(TPB), 0, s, P, points, c.partial);
    hipLaunchKernelGGL(bbox_finish_kernel<FINITE_ONLY>, dim3(1), dim3(64), 0, s, c.npartial, c.partial, c.bbox);
    hipLaunchKernelGGL(morton_kernel, dim3((P + TPB - 1) / TPB), dim3(TPB), 0, s, P, points, c.bbox, c.codes, c.ids);
    uint32_t *const k[2] = {c.codes, c.codes_sorted}, *const v[2] = {c.ids, c.ids_sorted};
    const int at = ts_radix_sort_pairs(k, v, (size_t)P, 30, c.sort_temp, s); // 30-bit Morton codes: four 8-bit passes, stable
    hipLaunchKernelGGL(gather_boxes_kernel<FINITE_ONLY>, dim3(c.nboxes), dim3(TPB), 0, s, P, points, v[at], c.sp, c.boxes);
    return hipGetLastError();
}
} // namespace
