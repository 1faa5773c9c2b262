// ts_mesh_scan.h -- the exclusive prefix sum of the mesh units in block-sum form, single-sourced: per-block sums (tiles of SCAN_TILE
// elements, SCAN_PER per lane), one workgroup turns them into offsets, then every block ranks its own elements behind the sum in front of
// it (nobody waits for anybody).  mesh_manifold.hip and mesh_holes.hip scan stored columns with the three kernels below (scan_columns);
// mesh_weld.hip and mesh_smooth.hip compute their flags on the fly and do other work in the apply pass, so their count and apply kernels
// stay with them, on block_scan256 and scan_offsets_kernel.  The kernels are templates: a unit emits what it launches.
#pragma once
#include "ts_mesh_common.h"

namespace
{
constexpr int SCAN_PER = 8, SCAN_TILE = 256 * SCAN_PER;

inline size_t scan_blocks(size_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

// exclusive scan of one value per lane over the 256-lane workgroup; returns the lane's offset, *total the sum.  lds: 4 words; the first
// barrier comes before they are written, so a second call may follow at once.
__device__ __forceinline__ uint32_t block_scan256(uint32_t v, uint32_t *lds, uint32_t *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
        const uint32_t t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    __syncthreads();
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (int w = 0; w < 4; w++) { const uint32_t t = lds[w]; if (w < wave) base += t; all += t; }
    *total = all;
    return base + incl - v;
}

// One workgroup: the sums of nb blocks, COLS interleaved columns of them, become their exclusive offsets in place; the COLS totals go to
// total[0 .. COLS).  A lane owns `span` consecutive blocks, more than one from 257 blocks on; lo <= hi <= nb bound every index.
template <int COLS>
__global__ void __launch_bounds__(256) scan_offsets_kernel(int nb, uint32_t *block_sum, uint32_t *__restrict__ total)
{
    __shared__ uint32_t lds[4];
    const int span = (nb + 255) / 256, lo = min(nb, (int)threadIdx.x * span), hi = min(nb, lo + span);
    uint32_t run[COLS];
#pragma unroll
    for (int c = 0; c < COLS; c++)
    {
        uint32_t sum = 0, all;
        for (int i = lo; i < hi; i++) sum += block_sum[COLS * (size_t)i + c];
        run[c] = block_scan256(sum, lds, &all);
        if (threadIdx.x == 0) total[c] = all;
    }
    for (int i = lo; i < hi; i++)
    {
#pragma unroll
        for (int c = 0; c < COLS; c++)
        {
            const uint32_t x = block_sum[COLS * (size_t)i + c];
            block_sum[COLS * (size_t)i + c] = run[c];
            run[c] += x;
        }
    }
}

// ---- stored columns ----------------------------------------------------------------------------------------------------------------------
template <int COLS>
struct ScanColumns
{
    uint32_t *col[COLS]; // n words each
};

template <int COLS>
__global__ void __launch_bounds__(256) scan_count_kernel(size_t n, ScanColumns<COLS> in, uint32_t *__restrict__ block_sum)
{
    __shared__ uint32_t lds[4];
    uint32_t sum[COLS] = {};
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++)
    {
        if (base + k >= n) continue;
#pragma unroll
        for (int c = 0; c < COLS; c++) sum[c] += in.col[c][base + k];
    }
#pragma unroll
    for (int c = 0; c < COLS; c++)
    {
        uint32_t all;
        block_scan256(sum[c], lds, &all);
        if (threadIdx.x == 0) block_sum[COLS * (size_t)blockIdx.x + c] = all;
    }
}

// every column becomes its exclusive prefix sum, in place: a thread reads its own eight elements before it writes them, nobody else's
template <int COLS>
__global__ void __launch_bounds__(256) scan_apply_kernel(size_t n, ScanColumns<COLS> io, const uint32_t *__restrict__ block_offset)
{
    __shared__ uint32_t lds[4];
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
    uint32_t v[COLS][SCAN_PER], run[COLS] = {};
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++)
    {
#pragma unroll
        for (int c = 0; c < COLS; c++)
        {
            v[c][k] = base + k < n ? io.col[c][base + k] : 0u;
            run[c] += v[c][k];
        }
    }
#pragma unroll
    for (int c = 0; c < COLS; c++)
    {
        uint32_t all;
        run[c] = block_offset[COLS * (size_t)blockIdx.x + c] + block_scan256(run[c], lds, &all);
    }
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++)
    {
#pragma unroll
        for (int c = 0; c < COLS; c++)
        {
            if (base + k < n) io.col[c][base + k] = run[c];
            run[c] += v[c][k];
        }
    }
}

// the three launches; block_sum: COLS * scan_blocks(n) words, total: COLS words
template <int COLS>
inline void scan_columns(size_t n, const ScanColumns<COLS> &io, uint32_t *block_sum, uint32_t *total, hipStream_t s)
{
    const unsigned nb = (unsigned)scan_blocks(n);
    hipLaunchKernelGGL(scan_count_kernel<COLS>, dim3(nb), dim3(256), 0, s, n, io, block_sum);
    hipLaunchKernelGGL(scan_offsets_kernel<COLS>, dim3(1), dim3(256), 0, s, (int)nb, block_sum, total);
    hipLaunchKernelGGL(scan_apply_kernel<COLS>, dim3(nb), dim3(256), 0, s, n, io, block_sum);
}
} // namespace
