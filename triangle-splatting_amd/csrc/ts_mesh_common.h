// ts_mesh_common.h -- what the indexed-mesh units (mesh_weld.hip, mesh_simplify.hip, mesh_smooth.hip, mesh_holes.hip, mesh_manifold.hip,
// mesh_orient.hip, mesh_subdivide.hip, mesh_flip.hip) share besides their scans (ts_mesh_scan.h), their run bounds (ts_mesh_runs.h) and
// the sort-by-edge front (ts_mesh_edges.h), single-sourced; mesh_overlap.hip and mesh_distance.hip include it for its fill and its copy
// alone.  Host and device helpers, every one with internal linkage: the units live in different libraries,
// so each gets its own copy.  The only kernels defined here are the fill and the copy below, as templates: an unreferenced kernel is still
// emitted, a template that nobody launches is not, and not every unit launches both.
#pragma once
#include "ts2d_common.h"

#include <algorithm>

namespace
{
inline unsigned blocks256(size_t n) { return (unsigned)((n + 255) / 256); }

inline int bit_length(uint32_t v)
{
    int n = 1; // at least one pass bit
    while (n < 32 && (v >> n)) n++;
    return n;
}

__device__ __forceinline__ bool finite32(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ bool finite64(double x) { return ((unsigned long long)__double_as_longlong(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }

__device__ __forceinline__ uint32_t next_corner(uint32_t c) { return c % 3u == 2u ? c - 2u : c + 1u; }

// the wave's sum of n, added to *counter by its first lane
__device__ __forceinline__ void count_into(unsigned long long *counter, uint32_t n)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63) == 0 && n) __hip_atomic_fetch_add(counter, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The 256-lane workgroup's sums of c[0 .. 3], added to counts[0 .. 3] by its first four lanes: one atomic per counter and workgroup.  Every
// lane of the workgroup calls this together, once per kernel (it synchronises and owns its LDS words).
__device__ __forceinline__ void count4_into(unsigned long long *counts, uint32_t (&c)[4])
{
    __shared__ uint32_t red[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o);
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 4; k++) red[threadIdx.x >> 6][k] = c[k];
    __syncthreads();
    if (threadIdx.x < 4)
    {
        const uint32_t t = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (t) __hip_atomic_fetch_add(counts + threadIdx.x, (unsigned long long)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- which faces count --------------------------------------------------------------------------------------------------------------------
// Kept (keep may be null: every face is) and the three indices in [0, V).  f < F.  v holds the indices of a kept face, zeros otherwise.
__device__ __forceinline__ bool face_in_range(int V, size_t f, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep, int32_t (&v)[3])
{
    v[0] = v[1] = v[2] = 0;
    if (keep && !keep[f]) return false;
    v[0] = faces[3 * f]; v[1] = faces[3 * f + 1]; v[2] = faces[3 * f + 2];
    return (uint32_t)v[0] < (uint32_t)V && (uint32_t)v[1] < (uint32_t)V && (uint32_t)v[2] < (uint32_t)V;
}

// ts_smooth.h's rule: kept, the three indices in [0, V) and pairwise distinct.  f < F.
__device__ __forceinline__ bool face_takes_part(int V, size_t f, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep, int32_t (&v)[3])
{
    return face_in_range(V, f, faces, keep, v) && v[0] != v[1] && v[1] != v[2] && v[0] != v[2];
}

// ---- runs of equal edges ------------------------------------------------------------------------------------------------------------------
// The edges (lo[j], hi[j]), j < N, ascending, the sentinels (lo = V) last.  0 unless position j heads a run of a real edge; otherwise the
// run's length, cut at 3: 1 = used once, 2 = exactly twice, 3 = three times or more.  Every index read is j, j - 1, j + 1 or j + 2 checked
// against N.
__device__ __forceinline__ int edge_run_head(int V, size_t N, size_t j, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi)
{
    if (j >= N) return 0;
    const uint32_t a = lo[j], b = hi[j];
    if (a >= (uint32_t)V || (j > 0 && lo[j - 1] == a && hi[j - 1] == b)) return 0;
    const bool two = j + 1 < N && lo[j + 1] == a && hi[j + 1] == b;
    const bool three = two && j + 2 < N && lo[j + 2] == a && hi[j + 2] == b;
    return three ? 3 : two ? 2 : 1;
}

// ---- fills and copies --------------------------------------------------------------------------------------------------------------------
// A hipMemsetAsync or a device-to-device hipMemcpyAsync that is captured into a graph does not reliably run where stream order put it on
// this stack ("Stream order of the mesh entry points"): the mesh units clear and copy with these two kernels instead, after
// the model of ts_launch_zero_words.  Any address, any length; whole 32-bit words where the addresses allow, the odd bytes one by one.
template <int = 0>
__global__ void __launch_bounds__(256) mesh_fill_kernel(uint8_t *__restrict__ p, size_t bytes, uint32_t word)
{
    const size_t stride = (size_t)gridDim.x * 256, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (((size_t)p & 3) == 0)
    {
        const size_t words = bytes / 4;
        for (size_t j = i; j < words; j += stride) ((uint32_t *)p)[j] = word;
        if (i < (bytes & 3)) p[4 * words + i] = (uint8_t)word;
    }
    else
        for (size_t j = i; j < bytes; j += stride) p[j] = (uint8_t)word;
}

template <int = 0>
__global__ void __launch_bounds__(256) mesh_copy_kernel(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, size_t bytes)
{
    const size_t stride = (size_t)gridDim.x * 256, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if ((((size_t)dst | (size_t)src) & 3) == 0)
    {
        const size_t words = bytes / 4;
        for (size_t j = i; j < words; j += stride) ((uint32_t *)dst)[j] = ((const uint32_t *)src)[j];
        if (i < (bytes & 3)) dst[4 * words + i] = src[4 * words + i];
    }
    else
        for (size_t j = i; j < bytes; j += stride) dst[j] = src[j];
}

inline unsigned fill_blocks(size_t bytes, bool by_words)
{
    const size_t units = by_words ? std::max(bytes / 4, (size_t)1) : bytes; // one block at least: it also writes the odd bytes behind the words
    return (unsigned)std::min((units + 255) / 256, (size_t)1 << 20);        // the kernels stride: a count beyond 2^28 units is covered too
}

// p[0 .. bytes) = the low byte of `value`, enqueued on s: hipMemsetAsync's arguments and meaning, as a kernel launch
inline hipError_t mesh_fill(void *p, int value, size_t bytes, hipStream_t s)
{
    if (bytes == 0) return hipSuccess;
    const bool by_words = ((size_t)p & 3) == 0;
    hipLaunchKernelGGL(mesh_fill_kernel<0>, dim3(fill_blocks(bytes, by_words)), dim3(256), 0, s, (uint8_t *)p, bytes, (uint32_t)(value & 0xFF) * 0x01010101u);
    return hipGetLastError();
}

// dst[0 .. bytes) = src[0 .. bytes), device to device, the ranges disjoint, enqueued on s
inline hipError_t mesh_copy(void *dst, const void *src, size_t bytes, hipStream_t s)
{
    if (bytes == 0) return hipSuccess;
    const bool by_words = (((size_t)dst | (size_t)src) & 3) == 0;
    hipLaunchKernelGGL(mesh_copy_kernel<0>, dim3(fill_blocks(bytes, by_words)), dim3(256), 0, s, (uint8_t *)dst, (const uint8_t *)src, bytes);
    return hipGetLastError();
}

// ---- workspace ----------------------------------------------------------------------------------------------------------------------------
// the radix sort's tables shrink where its chunk length grows (TS_RS_SMALL_BELOW): never less than just below that size
inline size_t sort_scratch_bytes(size_t n)
{
    size_t b = ts_radix_scratch_bytes(n);
    if (n > (size_t)TS_RS_SMALL_BELOW) b = std::max(b, ts_radix_scratch_bytes((size_t)TS_RS_SMALL_BELOW));
    return b;
}

struct Carver // addresses as integers: the size queries carve from a null workspace, where pointer arithmetic would be undefined
{
    size_t p, base;
    explicit Carver(void *ws) : p(ts_align_up((size_t)ws)), base((size_t)ws) {}
    uint32_t *words(size_t n) { return (uint32_t *)bytes(n * 4); }
    void *bytes(size_t n) { const size_t q = p; p += ts_align_up(n); return (void *)q; }
    size_t used() const { return p - base; }
};
} // namespace
