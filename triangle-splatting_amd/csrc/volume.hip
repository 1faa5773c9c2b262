// volume.hip -- TSDF integration in integers, the volume's field, and marching tetrahedra on any fp32 grid (include/ts_volume.h).
//
// Built with -ffp-contract=off: every float64 operation of the header rounds, so the state, the field and the extracted vertices are
// bit-identical to tests/ref_volume.py.
//
// Integration and field: one thread per sample.  A sample outside the frustum, behind the surface or on a skipped pixel touches neither
// state array; an updated one reads and writes its 12 bytes.
//
// Extraction: one thread per sample index, which is the index of the cell whose corner 0 it is (a sample on a far face owns no cell and
// counts 0).  Three levels of sums, no workgroup waits on another:
//   count   per-cell triangle count (a byte) and the sum of each block of TPB cells
//   scan1   exclusive scan of CHUNK consecutive block sums in place, the chunk's sum
//   scan2   one block: exclusive scan of the chunk sums in place (at most 2^27 / TPB / CHUNK = 512 of them), the total
//   emit    block-local exclusive scan of the counts + the two offsets = the first triangle of the cell; the cell is evaluated again
// The case table (which edges carry the vertices of each of the 16 inside masks of a tetrahedron) and the orientation bits are the ones
// tests/ref_volume.py derives; tests/test_volume_cpu.py compares the constants below with it.
#include "ts_volume_launch.h"

#include <float.h>

namespace
{
constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int CHUNK = 1024; // block sums per scan1 block: TPB threads x 4

// per inside mask: up to two triangles of three vertices; a vertex is 4 bits, the edge (lo | hi << 2) of tetrahedron positions lo < hi
__constant__ const uint32_t CASE_EDGES[16] = {0x000000, 0x000c84, 0x000d94, 0x9d8dc8, 0x000e98, 0x9e4ec4, 0x8e4ed4, 0x000edc,
                                              0x000edc, 0xde4e84, 0xce4e94, 0x000e98, 0xcd8d98, 0x000d94, 0x000c84, 0x000000};
// per tetrahedron: bit `mask` set iff the case's triangles swap their 2nd and 3rd vertices (normal from inside to outside)
constexpr uint32_t FLIP_BITS[6] = {0x4d24, 0x32da, 0x32da, 0x4d24, 0x4d24, 0x32da};
constexpr uint32_t CASE_COUNTS = 0x16696994u; // 2 bits per mask: its number of triangles
// the six tetrahedra, 4 bits per corner, position 0 lowest
constexpr uint32_t TET_CORNERS[6] = {0x7310, 0x7510, 0x7320, 0x7620, 0x7540, 0x7640};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= FLT_MAX; }
__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= DBL_MAX; }

// exclusive scan of one value per thread over the block; `total` = the block's sum.  lds: WAVES words, free again on return.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t &total, uint32_t *lds)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w)
    {
        const uint32_t s = lds[w];
        if (w < wave) base += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

__global__ void __launch_bounds__(TPB) integrate_kernel(int nx, int ny, int n, float ox, float oy, float oz, float h, float trunc,
                                                         const float *__restrict__ view, float tan_fovx, float tan_fovy, int W, int H,
                                                         const float *__restrict__ depth, const uint8_t *__restrict__ mask, int carve,
                                                         long long *__restrict__ sum, int32_t *__restrict__ weight,
                                                         unsigned long long *__restrict__ updated)
{
    __shared__ uint32_t counts[WAVES];
    const int idx = blockIdx.x * TPB + threadIdx.x;
    bool update = false;
    if (idx < n)
    {
        const int i = idx % nx, r = idx / nx, j = r % ny, k = r / ny;
        const double hd = (double)h;
        const double p0 = (double)ox + hd * (double)i, p1 = (double)oy + hd * (double)j, p2 = (double)oz + hd * (double)k;
        const double v0 = ((p0 * (double)view[0] + p1 * (double)view[4]) + p2 * (double)view[8]) + (double)view[12];
        const double v1 = ((p0 * (double)view[1] + p1 * (double)view[5]) + p2 * (double)view[9]) + (double)view[13];
        const double z = ((p0 * (double)view[2] + p1 * (double)view[6]) + p2 * (double)view[10]) + (double)view[14];
        if (finite_d(z) && z > 0.0)
        {
            const double col = floor((v0 / (z * (double)tan_fovx) + 1.0) * (0.5 * (double)W));
            const double row = floor((v1 / (z * (double)tan_fovy) + 1.0) * (0.5 * (double)H));
            if (col >= 0.0 && col < (double)W && row >= 0.0 && row < (double)H) // a NaN fails
            {
                const size_t pix = (size_t)(int)row * (size_t)W + (size_t)(int)col;
                if (!mask || mask[pix] != 0)
                {
                    const float d = depth[pix];
                    long long q = 1048576;
                    bool ok = finite_f(d) && !(d < 0.0f);
                    if (ok && d == 0.0f) ok = carve != 0; // an uncovered pixel: free space, or nothing
                    else if (ok)
                    {
                        const double sd = (double)d - z, tr = (double)trunc;
                        if (sd < -tr) ok = false;
                        else
                        {
                            const double sr = sd / tr, s = sr < 1.0 ? sr : 1.0;
                            q = (long long)rint(s * 1048576.0);
                        }
                    }
                    if (ok)
                    {
                        const int32_t w = weight[idx];
                        if (w != INT32_MAX)
                        {
                            sum[idx] += q;
                            weight[idx] = w + 1;
                            update = true;
                        }
                    }
                }
            }
        }
    }
    if (updated) // one atomic per block that updated anything
    {
        const unsigned long long ballot = __ballot(update);
        if ((threadIdx.x & 63) == 0) counts[threadIdx.x >> 6] = (uint32_t)__popcll(ballot);
        __syncthreads();
        if (threadIdx.x == 0)
        {
            uint32_t c = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) c += counts[w];
            if (c) atomicAdd(updated, (unsigned long long)c);
        }
    }
}

__global__ void __launch_bounds__(TPB) field_kernel(int n, const long long *__restrict__ sum, const int32_t *__restrict__ weight, int min_weight,
                                                     float *__restrict__ field)
{
    const int idx = blockIdx.x * TPB + threadIdx.x;
    if (idx >= n) return;
    const int32_t w = weight[idx];
    field[idx] = w >= min_weight ? (float)((double)sum[idx] / ((double)w * 1048576.0)) : __uint_as_float(0x7FC00000u);
}

// ---- marching tetrahedra ----------------------------------------------------------------------------------------------------------------
struct Cell
{
    float f[8];
    uint32_t inside; // bit c: corner c is inside
    bool crossed;    // active, and neither all inside nor all outside
};

__device__ __forceinline__ Cell load_cell(const float *__restrict__ field, int nx, int ny, int nz, int idx, float iso, int &i, int &j, int &k)
{
    Cell c;
    c.inside = 0;
    c.crossed = false;
    i = idx % nx;
    const int r = idx / nx;
    j = r % ny;
    k = r / ny;
    if (i >= nx - 1 || j >= ny - 1 || k >= nz - 1) return c; // a sample on a far face owns no cell
    const size_t sy = (size_t)nx, sz = (size_t)nx * (size_t)ny;
    bool active = true;
#pragma unroll
    for (int q = 0; q < 8; ++q)
    {
        c.f[q] = field[(size_t)idx + (q & 1) + ((q >> 1) & 1) * sy + ((q >> 2) & 1) * sz];
        active = active && finite_f(c.f[q]);
        c.inside |= (c.f[q] < iso ? 1u : 0u) << q;
    }
    c.crossed = active && c.inside != 0 && c.inside != 0xFFu;
    return c;
}

template <int T>
__device__ __forceinline__ uint32_t tet_mask(uint32_t inside)
{
    uint32_t m = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) m |= ((inside >> ((TET_CORNERS[T] >> (4 * p)) & 7)) & 1u) << p;
    return m;
}

__device__ __forceinline__ uint32_t cell_count(uint32_t inside)
{
    return ((CASE_COUNTS >> (2 * tet_mask<0>(inside))) & 3) + ((CASE_COUNTS >> (2 * tet_mask<1>(inside))) & 3) +
           ((CASE_COUNTS >> (2 * tet_mask<2>(inside))) & 3) + ((CASE_COUNTS >> (2 * tet_mask<3>(inside))) & 3) +
           ((CASE_COUNTS >> (2 * tet_mask<4>(inside))) & 3) + ((CASE_COUNTS >> (2 * tet_mask<5>(inside))) & 3);
}

__global__ void __launch_bounds__(TPB) count_kernel(int nx, int ny, int nz, int n, const float *__restrict__ field, float iso,
                                                     uint8_t *__restrict__ counts, uint32_t *__restrict__ block_sums)
{
    __shared__ uint32_t lds[WAVES];
    const int idx = blockIdx.x * TPB + threadIdx.x;
    uint32_t c = 0;
    if (idx < n)
    {
        int i, j, k;
        const Cell cell = load_cell(field, nx, ny, nz, idx, iso, i, j, k);
        if (cell.crossed) c = cell_count(cell.inside);
        counts[idx] = (uint8_t)c;
    }
    uint32_t total;
    block_exclusive_scan(c, total, lds);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// in place: block_sums[e] becomes the sum of the entries before it in its chunk; chunk_sums[chunk] = the chunk's sum
__global__ void __launch_bounds__(TPB) scan1_kernel(int nblocks, uint32_t *__restrict__ block_sums, uint32_t *__restrict__ chunk_sums)
{
    __shared__ uint32_t lds[WAVES];
    const int e0 = blockIdx.x * CHUNK + threadIdx.x * 4;
    uint32_t v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = e0 + q < nblocks ? block_sums[e0 + q] : 0u;
    uint32_t total;
    uint32_t run = block_exclusive_scan(v[0] + v[1] + v[2] + v[3], total, lds);
#pragma unroll
    for (int q = 0; q < 4; ++q)
    {
        if (e0 + q < nblocks) block_sums[e0 + q] = run;
        run += v[q];
    }
    if (threadIdx.x == 0) chunk_sums[blockIdx.x] = total;
}

// one block, in place: chunk_sums[c] becomes the sum of the chunks before it; *total = the sum of all
__global__ void __launch_bounds__(TPB) scan2_kernel(int nchunks, uint32_t *__restrict__ chunk_sums, long long *__restrict__ total)
{
    __shared__ uint32_t lds[WAVES];
    uint32_t carry = 0;
    for (int c0 = 0; c0 < nchunks; c0 += TPB)
    {
        const int c = c0 + threadIdx.x;
        const uint32_t v = c < nchunks ? chunk_sums[c] : 0u;
        uint32_t tile;
        const uint32_t ex = block_exclusive_scan(v, tile, lds);
        if (c < nchunks) chunk_sums[c] = carry + ex;
        carry += tile;
    }
    if (threadIdx.x == 0) *total = (long long)carry;
}

struct Grid
{
    double ox, oy, oz, h, iso;
};

// the vertex of the edge between tetrahedron positions lo < hi: corners ca < cb, so sample index a < b (nx, ny >= 2 where a cell exists)
__device__ __forceinline__ void edge_vertex(const Grid &g, int i, int j, int k, int ca, int cb, float fa, float fb, float *out)
{
    const double t = (g.iso - (double)fa) / ((double)fb - (double)fa);
    const double ax = (double)(i + (ca & 1)), ay = (double)(j + ((ca >> 1) & 1)), az = (double)(k + ((ca >> 2) & 1));
    const double bx = (double)(i + (cb & 1)), by = (double)(j + ((cb >> 1) & 1)), bz = (double)(k + ((cb >> 2) & 1));
    out[0] = (float)(g.ox + g.h * (ax + t * (bx - ax)));
    out[1] = (float)(g.oy + g.h * (ay + t * (by - ay)));
    out[2] = (float)(g.oz + g.h * (az + t * (bz - az)));
}

template <int T>
__device__ __forceinline__ void emit_tet(const Cell &cell, const Grid &g, int i, int j, int k, int idx, long long &at, long long capacity,
                                         float *__restrict__ triangles, int32_t *__restrict__ cells)
{
    const uint32_t mask = tet_mask<T>(cell.inside);
    const int ntri = (CASE_COUNTS >> (2 * mask)) & 3;
    if (ntri == 0) return;
    constexpr int c0 = TET_CORNERS[T] & 7, c1 = (TET_CORNERS[T] >> 4) & 7, c2 = (TET_CORNERS[T] >> 8) & 7, c3 = (TET_CORNERS[T] >> 12) & 7;
    const float f0 = cell.f[c0], f1 = cell.f[c1], f2 = cell.f[c2], f3 = cell.f[c3];
    const bool flip = (FLIP_BITS[T] >> mask) & 1;
    uint32_t edges = CASE_EDGES[mask];
    for (int tri = 0; tri < ntri && at < capacity; ++tri, ++at)
    {
        float *out = triangles + 9 * (size_t)at;
#pragma unroll
        for (int v = 0; v < 3; ++v, edges >>= 4)
        {
            const int lo = edges & 3, hi = (edges >> 2) & 3; // lo in 0..2, hi in 1..3
            const int ca = lo == 0 ? c0 : lo == 1 ? c1 : c2, cb = hi == 1 ? c1 : hi == 2 ? c2 : c3;
            const float fa = lo == 0 ? f0 : lo == 1 ? f1 : f2, fb = hi == 1 ? f1 : hi == 2 ? f2 : f3;
            const int slot = v == 0 ? 0 : (flip ? 3 - v : v);
            edge_vertex(g, i, j, k, ca, cb, fa, fb, out + 3 * slot);
        }
        if (cells) cells[at] = idx;
    }
}

__global__ void __launch_bounds__(TPB) emit_kernel(int nx, int ny, int nz, int n, float ox, float oy, float oz, float h, const float *__restrict__ field,
                                                    float iso, const uint8_t *__restrict__ counts, const uint32_t *__restrict__ block_offsets,
                                                    const uint32_t *__restrict__ chunk_offsets, long long capacity, float *__restrict__ triangles,
                                                    int32_t *__restrict__ cells)
{
    __shared__ uint32_t lds[WAVES];
    const int idx = blockIdx.x * TPB + threadIdx.x;
    const uint32_t c = idx < n ? counts[idx] : 0u;
    uint32_t total;
    const uint32_t local = block_exclusive_scan(c, total, lds);
    if (c == 0) return;
    long long at = (long long)chunk_offsets[blockIdx.x / CHUNK] + (long long)block_offsets[blockIdx.x] + (long long)local;
    if (at >= capacity) return;
    int i, j, k;
    const Cell cell = load_cell(field, nx, ny, nz, idx, iso, i, j, k);
    const Grid g = {(double)ox, (double)oy, (double)oz, (double)h, (double)iso};
    emit_tet<0>(cell, g, i, j, k, idx, at, capacity, triangles, cells);
    emit_tet<1>(cell, g, i, j, k, idx, at, capacity, triangles, cells);
    emit_tet<2>(cell, g, i, j, k, idx, at, capacity, triangles, cells);
    emit_tet<3>(cell, g, i, j, k, idx, at, capacity, triangles, cells);
    emit_tet<4>(cell, g, i, j, k, idx, at, capacity, triangles, cells);
    emit_tet<5>(cell, g, i, j, k, idx, at, capacity, triangles, cells);
}

struct ExtractCarve
{
    uint8_t *counts;
    uint32_t *block_sums, *chunk_sums;
    int nblocks, nchunks;
    size_t bytes;
};

ExtractCarve extract_carve(void *ws, size_t n)
{
    ExtractCarve c;
    c.nblocks = (int)((n + TPB - 1) / TPB);
    c.nchunks = (c.nblocks + CHUNK - 1) / CHUNK;
    char *p = (char *)ws;
    c.counts = (uint8_t *)p;
    p += ts_align_up(n);
    c.block_sums = (uint32_t *)p;
    p += ts_align_up((size_t)c.nblocks * sizeof(uint32_t));
    c.chunk_sums = (uint32_t *)p;
    p += ts_align_up((size_t)c.nchunks * sizeof(uint32_t));
    c.bytes = (size_t)(p - (char *)ws);
    return c;
}
} // namespace

hipError_t ts_volume_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float h, float trunc, const float *view, float tan_fovx,
                               float tan_fovy, int W, int H, const float *depth, const uint8_t *mask, int carve, long long *sum, int32_t *weight,
                               unsigned long long *updated, hipStream_t s)
{
    const int n = nx * ny * nz; // at most 2^27 (api_volume.hip)
    hipLaunchKernelGGL(integrate_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, s, nx, ny, n, ox, oy, oz, h, trunc, view, tan_fovx,
                       tan_fovy, W, H, depth, mask, carve, sum, weight, updated);
    return hipGetLastError();
}

hipError_t ts_volume_field(int n, const long long *sum, const int32_t *weight, int min_weight, float *field, hipStream_t s)
{
    hipLaunchKernelGGL(field_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, s, n, sum, weight, min_weight, field);
    return hipGetLastError();
}

size_t ts_volume_extract_workspace_bytes(size_t n) { return extract_carve(nullptr, n).bytes + TS_ALIGN; }

hipError_t ts_volume_extract(int nx, int ny, int nz, float ox, float oy, float oz, float h, const float *field, float iso, long long capacity,
                             float *triangles, int32_t *cell, long long *total, void *ws, hipStream_t s)
{
    const int n = nx * ny * nz;
    const ExtractCarve c = extract_carve((void *)ts_align_up((size_t)ws), (size_t)n);
    hipLaunchKernelGGL(count_kernel, dim3((unsigned)c.nblocks), dim3(TPB), 0, s, nx, ny, nz, n, field, iso, c.counts, c.block_sums);
    hipLaunchKernelGGL(scan1_kernel, dim3((unsigned)c.nchunks), dim3(TPB), 0, s, c.nblocks, c.block_sums, c.chunk_sums);
    hipLaunchKernelGGL(scan2_kernel, dim3(1), dim3(TPB), 0, s, c.nchunks, c.chunk_sums, total);
    if (capacity > 0)
        hipLaunchKernelGGL(emit_kernel, dim3((unsigned)c.nblocks), dim3(TPB), 0, s, nx, ny, nz, n, ox, oy, oz, h, field, iso, c.counts, c.block_sums,
                           c.chunk_sums, capacity, triangles, cell);
    return hipGetLastError();
}
