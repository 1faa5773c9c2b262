// mesh_distance.hip -- the exact nearest-neighbour search between two point sets and the area-weighted surface sampler (include/ts_geom.h).
//
// Built with -ffp-contract=off: the distance (dx*dx + dy*dy) + dz*dz rounds every operation, and so do the two bounds below, the float64
// face areas and the fp32 sample points.
//
// Search.  Both sets go through knn.hip's front half (ts_knn_front.h, FINITE_ONLY), each with its own carve: Morton-sorted points gathered
// as float4 (xyz, original index) and the min/max box of every 1024 of them; a point with a NaN or infinite coordinate stays out of every
// box and is stored as three NaNs, so every comparison against it fails.  One 256-lane workgroup owns 1024 sorted queries (4 per lane) and
// writes its results back by original index.  There is no "own box" among the refs to seed the radius with, so the workgroup first scans
// the ref box with the smallest box-to-box bound to its query box (ties: the lowest box index), then sweeps every other ref box whose bound
// does not exceed the workgroup's worst current distance.  A visited box is staged through LDS (every lane reads the same candidate: LDS
// broadcast) and a lane skips the queries whose box-to-point bound is above their current best.
//   Exactness.  Both bounds have the distance's expression shape -- one difference of two coordinates per axis, then the squares, then the
//   same sum order (x*x + y*y) + z*z -- and the differences they take are never larger in magnitude than the pair's; rounding is monotonic,
//   so a bound is never above the d of a pair it covers.  Pruning is on strict `>` only: a ref at an EQUAL distance with a smaller index in
//   a later box is still visited, so the tie rule (smallest ref index) holds whatever the visiting order.  The best pair starts as
//   (+inf, 0xFFFFFFFF): a ref whose d overflowed to +inf still beats it by its index, and while a query's best is +inf nothing is pruned.
//
// Sampler.  amax by integer atomicMax on the bit patterns of the non-negative doubles (order-free), integer weights
// floor(area / amax * 2^32), their inclusive 64-bit prefix sum by a hand-written three-launch scan (1024 faces per workgroup, one workgroup
// over the block sums, offsets added back: integer sums, exact in any order), then one lane per sample: splitmix64 words from counters, a
// stratified position in [0, W), a binary search in the prefix sums, barycentrics from 24-bit integers.  No float atomics, no rocPRIM.
#include "ts_knn_front.h"
#include "ts_geom_launch.h"
#include "ts_mesh_common.h"

#include <algorithm>

namespace
{
// ---- nearest search ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dist_sum(float dx, float dy, float dz) { return (dx * dx + dy * dy) + dz * dz; }

// one axis of a bound: the gap between [amn, amx] and [bmn, bmx], a single difference of two of the four coordinates, 0 when they overlap
__device__ __forceinline__ float axis_gap(float amn, float amx, float bmn, float bmx)
{
    return amn > bmx ? amn - bmx : (bmn > amx ? bmn - amx : 0.0f);
}

__device__ __forceinline__ float bound_box_box(const Box &a, const Box &b)
{
    return dist_sum(axis_gap(a.mnx, a.mxx, b.mnx, b.mxx), axis_gap(a.mny, a.mxy, b.mny, b.mxy), axis_gap(a.mnz, a.mxz, b.mnz, b.mxz));
}

__device__ __forceinline__ float bound_box_point(const Box &b, float px, float py, float pz)
{
    return dist_sum(axis_gap(px, px, b.mnx, b.mxx), axis_gap(py, py, b.mny, b.mxy), axis_gap(pz, pz, b.mnz, b.mxz));
}

__global__ void __launch_bounds__(TPB) cross_search_kernel(int Q, int R, int nrboxes, const float4 *__restrict__ qsp, const Box *__restrict__ qboxes,
                                                            const float4 *__restrict__ rsp, const Box *__restrict__ rboxes,
                                                            int32_t *__restrict__ nearest, float *__restrict__ dist2, unsigned long long *box_visits)
{
    __shared__ float4 cand[BOX];
    __shared__ float red[TPB / 64];
    const int mybox = blockIdx.x, tid = threadIdx.x;
    const Box bme = qboxes[mybox];
    const float inf = __uint_as_float(0x7F800000u);

    float px[PPT], py[PPT], pz[PPT], best[PPT];
    uint32_t pid[PPT], bestid[PPT];
    bool inside[PPT], have[PPT];
#pragma unroll
    for (int q = 0; q < PPT; q++)
    {
        const int i = mybox * BOX + q * TPB + tid;
        const float nan = __uint_as_float(0x7FC00000u);
        inside[q] = i < Q;
        const float4 p = inside[q] ? qsp[i] : make_float4(nan, nan, nan, 0.0f);
        px[q] = p.x; py[q] = p.y; pz[q] = p.z; pid[q] = __float_as_uint(p.w);
        have[q] = inside[q] && p.x == p.x; // a non-finite query was stored as NaNs
        best[q] = inf; bestid[q] = 0xFFFFFFFFu;
    }

    unsigned visited = 0;
    auto scan_box = [&](int b) {
        visited++;
        const Box bb = rboxes[b];
        const int n = min(BOX, R - b * BOX);
        __syncthreads(); // previous users of `cand` are done
        for (int i = tid; i < n; i += TPB) cand[i] = rsp[(size_t)b * BOX + i];
        __syncthreads();
        bool act[PPT], any = false;
#pragma unroll
        for (int q = 0; q < PPT; q++)
        {
            act[q] = have[q] && !(bound_box_point(bb, px[q], py[q], pz[q]) > best[q]); // strict: an equal bound may hide a smaller index
            any |= act[q];
        }
        if (!any) return;
        for (int i = 0; i < n; i++)
        {
            const float4 c = cand[i];
            const uint32_t cid = __float_as_uint(c.w);
#pragma unroll
            for (int q = 0; q < PPT; q++)
            {
                if (!act[q]) continue;
                const float d = dist_sum(px[q] - c.x, py[q] - c.y, pz[q] - c.z); // NaN for a non-finite ref: both tests fail
                if (d < best[q] || (d == best[q] && cid < bestid[q])) { best[q] = d; bestid[q] = cid; }
            }
        }
    };
    auto worst_radius = [&]() {
        float worst = 0.0f;
#pragma unroll
        for (int q = 0; q < PPT; q++)
            if (have[q]) worst = fmaxf(worst, best[q]);
        return block_reduce(worst, red, true);
    };

    if (bme.mnx <= bme.mxx) // workgroup-uniform: the query box is not empty, i.e. some query here is finite
    {
        int seed = 0;
        float nearest_gap = inf;
        for (int b = 0; b < nrboxes; b++)
        {
            const float g = bound_box_box(bme, rboxes[b]);
            if (g < nearest_gap) { nearest_gap = g; seed = b; } // strict: the lowest box index among equals
        }
        scan_box(seed);
        float radius = worst_radius();
        for (int b = 0; b < nrboxes; b++)
        {
            if (b == seed) continue;
            if (bound_box_box(bme, rboxes[b]) > radius) continue; // workgroup-uniform: nobody here can gain from box b
            scan_box(b);
            radius = worst_radius();
        }
    }
#pragma unroll
    for (int q = 0; q < PPT; q++)
    {
        if (!inside[q]) continue;
        nearest[pid[q]] = bestid[q] == 0xFFFFFFFFu ? -1 : (int32_t)bestid[q];
        dist2[pid[q]] = have[q] ? best[q] : __uint_as_float(0x7FC00000u);
    }
    if (box_visits && tid == 0 && visited) atomicAdd(box_visits, (unsigned long long)visited);
}

// R == 0: nobody has a neighbour
__global__ void __launch_bounds__(256) no_refs_kernel(int Q, const float *__restrict__ queries, int32_t *__restrict__ nearest, float *__restrict__ dist2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    const bool finite = all_finite(queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2]);
    nearest[i] = -1;
    dist2[i] = __uint_as_float(finite ? 0x7F800000u : 0x7FC00000u);
}

size_t carve_bytes_monotone(int n)
{
    // the radix sort's tables shrink where its chunk length grows (TS_RS_SMALL_BELOW): never report less than just below that size
    const size_t b = knn_carve(nullptr, n).bytes;
    return n > TS_RS_SMALL_BELOW ? std::max(b, knn_carve(nullptr, TS_RS_SMALL_BELOW).bytes) : b;
}

// ---- face areas ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) face_areas_kernel(int V, int F, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                          const uint8_t *__restrict__ keep, double *__restrict__ area)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    double a = 0.0;
    const int32_t i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if ((!keep || keep[f]) && (uint32_t)i0 < (uint32_t)V && (uint32_t)i1 < (uint32_t)V && (uint32_t)i2 < (uint32_t)V)
    {
        const float *p0 = vertices + 3 * (size_t)i0, *p1 = vertices + 3 * (size_t)i1, *p2 = vertices + 3 * (size_t)i2;
        const float x0 = p0[0], y0 = p0[1], z0 = p0[2], x1 = p1[0], y1 = p1[1], z1 = p1[2], x2 = p2[0], y2 = p2[1], z2 = p2[2];
        if (all_finite(x0, y0, z0) && all_finite(x1, y1, z1) && all_finite(x2, y2, z2))
        {
            const double ax = (double)x1 - (double)x0, ay = (double)y1 - (double)y0, az = (double)z1 - (double)z0;
            const double bx = (double)x2 - (double)x0, by = (double)y2 - (double)y0, bz = (double)z2 - (double)z0;
            const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
            a = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
        }
    }
    area[f] = a;
}

// ---- sampler ------------------------------------------------------------------------------------------------------------------------------
constexpr int SCAN_BLOCK = 1024; // faces per workgroup of the prefix sum, 4 consecutive ones per lane

__device__ __forceinline__ unsigned long long wave_inclusive(unsigned long long v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
        const unsigned long long w = __shfl_up(v, o);
        if (lane >= o) v += w;
    }
    return v;
}

// inclusive sum over the 256 lanes of a workgroup; *total = the workgroup's sum
__device__ __forceinline__ unsigned long long block_inclusive(unsigned long long v, unsigned long long *wave_sums, unsigned long long *total)
{
    const unsigned long long inc = wave_inclusive(v);
    __syncthreads(); // previous users of `wave_sums` are done
    if ((threadIdx.x & 63) == 63) wave_sums[threadIdx.x >> 6] = inc;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; w++)
    {
        const unsigned long long t = wave_sums[w];
        if (w < (int)(threadIdx.x >> 6)) before += t;
        all += t;
    }
    *total = all;
    return inc + before;
}

__global__ void __launch_bounds__(256) area_max_kernel(int F, const double *__restrict__ area, unsigned long long *amax_bits)
{
    unsigned long long m = 0;
    for (size_t f = (size_t)blockIdx.x * 256 + threadIdx.x; f < (size_t)F; f += (size_t)gridDim.x * 256)
    {
        const unsigned long long b = (unsigned long long)__double_as_longlong(area[f]);
        m = b > m ? b : m; // non-negative doubles order like their bit patterns
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        const unsigned long long w = __shfl_xor(m, o);
        m = w > m ? w : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(amax_bits, m);
}

__device__ __forceinline__ unsigned long long face_weight(double a, double amax)
{
    const double x = floor(a / amax * 4294967296.0);
    return x >= 1.0 ? (x >= 4294967296.0 ? 4294967296ull : (unsigned long long)x) : 0ull; // a NaN or negative area weighs nothing
}

__global__ void __launch_bounds__(256) weight_scan_kernel(int F, const double *__restrict__ area, const unsigned long long *__restrict__ amax_bits,
                                                           unsigned long long *__restrict__ C, unsigned long long *__restrict__ block_sum)
{
    __shared__ unsigned long long wave_sums[4];
    const double amax = __longlong_as_double((long long)*amax_bits);
    const size_t f0 = (size_t)blockIdx.x * SCAN_BLOCK + 4 * (size_t)threadIdx.x;
    unsigned long long w[4], mine = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        w[k] = (f0 + k < (size_t)F && amax > 0.0) ? face_weight(area[f0 + k], amax) : 0ull;
        mine += w[k];
        w[k] = mine;
    }
    unsigned long long total;
    const unsigned long long before = block_inclusive(mine, wave_sums, &total) - mine;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (f0 + k < (size_t)F) C[f0 + k] = before + w[k];
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// one workgroup: block_sum[0 .. nb) -> its exclusive prefix, in place
__global__ void __launch_bounds__(256) block_sum_scan_kernel(int nb, unsigned long long *block_sum)
{
    __shared__ unsigned long long wave_sums[4];
    unsigned long long carry = 0;
    for (int base = 0; base < nb; base += 256)
    {
        const int i = base + threadIdx.x;
        const unsigned long long v = i < nb ? block_sum[i] : 0ull;
        unsigned long long total;
        const unsigned long long inc = block_inclusive(v, wave_sums, &total);
        if (i < nb) block_sum[i] = carry + inc - v;
        carry += total;
    }
}

__global__ void __launch_bounds__(256) add_offsets_kernel(int F, unsigned long long *__restrict__ C, const unsigned long long *__restrict__ block_sum)
{
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f < (size_t)F) C[f] += block_sum[f / SCAN_BLOCK];
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t seed, uint64_t k)
{
    uint64_t z = seed + (k + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256) sample_kernel(int V, int F, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                      const unsigned long long *__restrict__ C, int N, uint64_t seed, float *__restrict__ points,
                                                      int32_t *__restrict__ face)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= N) return;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    int32_t chosen = -1;
    const uint64_t W = F > 0 ? C[F - 1] : 0ull;
    if (W > 0) // amax > 0: then W >= 2^32 > N and no stratum is empty
    {
        const uint64_t qn = W / (uint64_t)N, rem = W % (uint64_t)N, us = (uint64_t)s;
        const uint64_t start = us * qn + (us < rem ? us : rem), len = qn + (us < rem ? 1 : 0);
        const uint64_t t = start + splitmix64(seed, 2 * us) % len, r1 = splitmix64(seed, 2 * us + 1);
        uint32_t lo = 0, hi = (uint32_t)F - 1; // the smallest f with C[f] > t; t < W = C[F - 1]
        while (lo < hi)
        {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (C[mid] > t) hi = mid;
            else lo = mid + 1;
        }
        chosen = (int32_t)lo;
        const int32_t i0 = faces[3 * (size_t)lo], i1 = faces[3 * (size_t)lo + 1], i2 = faces[3 * (size_t)lo + 2];
        if ((uint32_t)i0 < (uint32_t)V && (uint32_t)i1 < (uint32_t)V && (uint32_t)i2 < (uint32_t)V)
        {
            uint32_t iu = (uint32_t)(r1 >> 40), iv = (uint32_t)(r1 >> 16) & 0xFFFFFFu;
            if (iu + iv > (1u << 24)) { iu = (1u << 24) - iu; iv = (1u << 24) - iv; }
            const float u = (float)iu * 5.9604644775390625e-8f, v = (float)iv * 5.9604644775390625e-8f; // 2^-24: exact
            const float *p0 = vertices + 3 * (size_t)i0, *p1 = vertices + 3 * (size_t)i1, *p2 = vertices + 3 * (size_t)i2;
            x = (p0[0] + u * (p1[0] - p0[0])) + v * (p2[0] - p0[0]);
            y = (p0[1] + u * (p1[1] - p0[1])) + v * (p2[1] - p0[1]);
            z = (p0[2] + u * (p1[2] - p0[2])) + v * (p2[2] - p0[2]);
        }
    }
    face[s] = chosen;
    points[3 * (size_t)s] = x; points[3 * (size_t)s + 1] = y; points[3 * (size_t)s + 2] = z;
}

struct SampleCarve
{
    unsigned long long *C, *block_sum, *amax_bits;
    int nb;
    size_t bytes;
};

SampleCarve sample_carve(void *ws, int F)
{
    SampleCarve c;
    const size_t n = (size_t)(F > 0 ? F : 0);
    c.nb = (int)((n + SCAN_BLOCK - 1) / SCAN_BLOCK);
    char *p = (char *)ts_align_up((size_t)ws);
    auto take = [&](size_t bytes) { char *q = p; p += ts_align_up(bytes); return q; };
    c.C = (unsigned long long *)take(n * 8);
    c.block_sum = (unsigned long long *)take(((size_t)c.nb + 1) * 8);
    c.amax_bits = (unsigned long long *)take(8);
    c.bytes = (size_t)(p - (char *)ws);
    return c;
}
} // namespace

size_t ts_geom_cross_workspace_bytes(int Q, int R) { return carve_bytes_monotone(Q) + carve_bytes_monotone(R) + TS_ALIGN; }

hipError_t ts_geom_nearest_cross(int Q, const float *queries, int R, const float *refs, int32_t *nearest, float *dist2,
                                 unsigned long long *box_visits, void *ws, hipStream_t s)
{
    if (Q <= 0) return hipSuccess;
    if (R <= 0)
    {
        hipLaunchKernelGGL(no_refs_kernel, dim3((Q + 255) / 256), dim3(256), 0, s, Q, queries, nearest, dist2);
        return hipGetLastError();
    }
    char *base = (char *)ts_align_up((size_t)ws);
    const KnnCarve cq = knn_carve(base, Q);
    const KnnCarve cr = knn_carve(base + cq.bytes, R); // cq.bytes is a multiple of TS_ALIGN: `base` is aligned and so is every piece
    hipError_t e = knn_prepare<true>(Q, queries, cq, s);
    if (e != hipSuccess) return e;
    e = knn_prepare<true>(R, refs, cr, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cross_search_kernel, dim3(cq.nboxes), dim3(TPB), 0, s, Q, R, cr.nboxes, cq.sp, cq.boxes, cr.sp, cr.boxes, nearest, dist2,
                       box_visits);
    return hipGetLastError();
}

size_t ts_geom_sample_workspace_bytes(int F) { return sample_carve(nullptr, F).bytes + TS_ALIGN; }

hipError_t ts_geom_face_areas(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, double *area, hipStream_t s)
{
    if (F <= 0) return hipSuccess;
    hipLaunchKernelGGL(face_areas_kernel, dim3((F + 255) / 256), dim3(256), 0, s, V, F, vertices, faces, keep, area);
    return hipGetLastError();
}

hipError_t ts_geom_sample_surface(int V, int F, const float *vertices, const int32_t *faces, const double *area, int N, uint64_t seed,
                                  float *points, int32_t *face, void *ws, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const SampleCarve c = sample_carve(ws, F);
    if (F > 0)
    {
        hipError_t e = mesh_fill(c.amax_bits, 0, 8, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(area_max_kernel, dim3(std::min(c.nb, 1024)), dim3(256), 0, s, F, area, c.amax_bits);
        hipLaunchKernelGGL(weight_scan_kernel, dim3(c.nb), dim3(256), 0, s, F, area, c.amax_bits, c.C, c.block_sum);
        hipLaunchKernelGGL(block_sum_scan_kernel, dim3(1), dim3(256), 0, s, c.nb, c.block_sum);
        hipLaunchKernelGGL(add_offsets_kernel, dim3((unsigned)(((size_t)F + 255) / 256)), dim3(256), 0, s, F, c.C, c.block_sum);
    }
    hipLaunchKernelGGL(sample_kernel, dim3((N + 255) / 256), dim3(256), 0, s, V, F, vertices, faces, c.C, N, seed, points, face);
    return hipGetLastError();
}
