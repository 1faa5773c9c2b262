// depth_order.hip -- steps 1 and 2 of the binning (overview: ts2d_radix.h): the triangles in (depth, id) order, their tile counts in that order,
// the raw block sums, and N.
// Step 1 has three forms, chosen by depth_form(): the LSD passes of ts2d_radix.h / radix_sort.hip; below ~9 k triangles the whole order in one
// launch (depth_order_small_kernel); up to 500 k sampled splitters + per-bucket sorts in LDS (K0-K3 below).  Every form leaves the same order.
#include "ts2d_radix.h"

namespace
{
bool g_force_pass4 = false; // lab-library switch like radix_sort.hip's (ts2d_lab_force_depth_pass4): the depth sort never skips its fourth pass

// The depth sort's first histogram, ticket-free like rs_hist_direct_kernel, with the census riding along: a block leaves its part of N and of the
// key-bit OR / AND as three per-chunk words; block 0 of the scatter kernel that follows adds them up and publishes N (device
// word + pinned host word) and the top-byte verdict (`top_const`).  No ticket at all: electing a publisher HERE costs one same-address
// atomic per block, and 488 of those in a row take longer (17 us) than the histogram itself.  Large scenes (more than
// TS_DIRECT_MAX_SLABS slabs) keep rs_hist_kernel<true>.
template <int CH>
__global__ void __launch_bounds__(256) rs_hist_census_direct_kernel(const uint32_t *__restrict__ keys, int64_t n, uint32_t mask, RadixScratchView r,
                                                                     uint32_t *__restrict__ acc, DepthCensus census)
{
    __shared__ uint32_t bins[NB];
    __shared__ unsigned long long csum[4];
    __shared__ uint32_t cor[4], cand[4];
    const int t = threadIdx.x, chunk = rs_chunk_of_block(r.chunks);
    if (chunk < 0) return;
    bins[t] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)chunk * CH;
    KeyCensus mine;
#pragma unroll
    for (int b = 0; b < CH / 256; b++)
    {
        const int64_t i = base + 256 * b + t;
        if (i < n)
        {
            const uint32_t k = keys[i];
            atomicAdd(&bins[k & mask], 1u);
            mine.add(k, census.tiles_touched[i]);
        }
    }
    mine.wave_fold();
    mine.park(csum, cor, cand);
    __syncthreads();
    const uint32_t c = bins[t];
    r.table[(size_t)chunk * NB + t] = c;
    if (c) __hip_atomic_fetch_add(acc + (size_t)(chunk >> 6) * NB + t, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 0)
    {
        const KeyCensus all = KeyCensus::gather<4>(csum, cor, cand);
        census.chunk_sum[chunk] = all.tiles;
        census.chunk_or[chunk] = all.kor;
        census.chunk_and[chunk] = all.kand;
    }
}

// ---- step 2: tiles_sorted = tiles_touched[perm], 64-bit block sums, their prefix, N ---------------------------------------
// The block sums stay RAW and nobody waits for a last block (round 3): every emission block adds up the sums in front of it itself
// (blocksum[nblocks] = N is already there from the depth sort's census): up to 2048 of them (2 M triangles), eight loads per thread.  Beyond
// that (round 4) a second level `supersum` holds the sum of every 64 consecutive block sums (fire-and-forget 64-bit atomics, zeroed by the
// step's first launch), so an emission block adds at most nblocks / 64 + 63 values at any size.  Until then such scenes fell back to an
// elected block that turned the sums into their prefix -- one same-address ticket atomic per block, 4883 in a row at 5 M triangles: scan
// 0.113 -> 0.087 ms there.  (Below 2048 blocks the atomics cost more than they save: 13 -> 18 us at 1 M triangles, hence the two forms.)
__global__ void __launch_bounds__(256) gather_blocksum_kernel(int P, GeometryStateView g, bool two_level)
{
    __shared__ unsigned long long wsum[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i0 = blockIdx.x * SB + 4 * t;
    const uint32_t *ids = sorted_ids(g);
    uint32_t v[4];
    unsigned long long sum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        v[k] = (i0 + k < P) ? g.tiles_touched[ids[i0 + k]] : 0u;
        sum += v[k];
    }
    if (i0 + 3 < P) *(uint4 *)(g.tiles_sorted + i0) = make_uint4(v[0], v[1], v[2], v[3]);
    else
        for (int k = 0; k < 4; k++)
            if (i0 + k < P) g.tiles_sorted[i0 + k] = v[k];
    // block sum: tile counts are < 2^32 each, a block's sum may not be
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) wsum[wave] = sum;
    __syncthreads();
    if (t == 0)
    {
        const unsigned long long total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        g.blocksum[blockIdx.x] = total;
        if (two_level && total) __hip_atomic_fetch_add((unsigned long long *)g.supersum + (blockIdx.x >> 6), total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- small scenes: the whole depth order in ONE launch ------------------------------------------------------------------------------
// Up to TS_DEPTH_SMALL_MAX triangles the eight launches of the depth sort and the launch of the block sums order a few thousand keys in 4-9 us
// each -- dependent launches, each one a load -> LDS -> barrier -> store chain with a handful of workgroups on the chip (BASELINE configs[0],
// 10 k triangles: 47 + 7 of the step's 166 us).  Here ONE workgroup of 16 waves keeps the (key, id) pairs in registers (wave w: a contiguous
// range of `per` <= 1024 positions, 64 consecutive pairs per step), ranks them pass by pass (lsd_rank_pass), exchanges them through LDS after
// every pass, and then does what the census, publish_census and gather_blocksum_kernel do: N to the device word and the pinned host word,
// tiles_sorted, the raw block sums.  Same passes (the fourth skipped under the same condition), same stable order,
// so sv[1] holds exactly the ids the multi-launch path leaves in sorted_ids(); top_const stays 0 (the order is always in sk[1] / sv[1]).
constexpr int TS_DEPTH_SMALL_MAX = 12288; // the kernel's capacity (level with the LSD passes of 1024-pair chunks at ~12 k triangles: 34 us either way); used up to TS_DEPTH_SMALL_USE
constexpr int DS_WAVES = 16, DS_KB = TS_DEPTH_SMALL_MAX / (64 * DS_WAVES);
// The one-launch form lives on gfx950's 160 KB of LDS per workgroup (two stages of TS_DEPTH_SMALL_MAX words + the per-wave digit table): 64 KB
// parts cannot hold it, and nothing else in the library may quietly push it over
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "depth_order_small_kernel is sized for gfx950 (160 KB LDS per workgroup)"
#endif
static_assert(2 * TS_DEPTH_SMALL_MAX * 4 + DS_WAVES * NB * 4 + DS_WAVES * 8 + (TS_DEPTH_SMALL_MAX / SB) * 8 + 2 * DS_WAVES * 4 + 16 <= 160 * 1024 - 8 * 1024,
              "depth_order_small_kernel: static LDS must leave 8 KB of the 160 KB for the runtime / alignment");
__global__ void __launch_bounds__(64 * DS_WAVES) depth_order_small_kernel(int P, GeometryStateView g, unsigned long long *host_out)
{
    __shared__ __attribute__((aligned(16))) uint32_t stage_k[TS_DEPTH_SMALL_MAX], stage_v[TS_DEPTH_SMALL_MAX];
    __shared__ uint32_t wcnt[DS_WAVES][NB]; // per-wave digit counts, then the start of the (wave, digit) run
    __shared__ uint32_t wtot[4];
    __shared__ unsigned long long csum[DS_WAVES], bsum[TS_DEPTH_SMALL_MAX / SB];
    __shared__ uint32_t cor[DS_WAVES], cand[DS_WAVES];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int per = ((P + 64 * DS_WAVES - 1) / (64 * DS_WAVES)) * 64; // positions per wave
    const int base = wave * per;
    const int mine = P - base < per ? (P - base > 0 ? P - base : 0) : per;
    const uint32_t *keys = (const uint32_t *)g.depth;
    uint32_t key[DS_KB], val[DS_KB], rk[DS_KB];
    KeyCensus census;
    if (t < TS_DEPTH_SMALL_MAX / SB) bsum[t] = 0ull;
#pragma unroll
    for (int b = 0; b < DS_KB; b++) // branch-free: the register arrays stay scalars the compiler can place one by one
    {
        const int i = 64 * b + lane;
        const bool in = i < mine;
        const int src = in ? base + i : 0;
        const uint32_t k = keys[src], tt = g.tiles_touched[src];
        key[b] = in ? k : 0xFFFFFFFFu;
        val[b] = (uint32_t)src;
        census.add(in ? k : 0u, in ? tt : 0u);
    }
    census.wave_fold();
    census.park(csum, cor, cand);
    __syncthreads();
    census = KeyCensus::gather<DS_WAVES>(csum, cor, cand);
    const unsigned long long N = census.tiles;
    const int passes = census.top_byte_constant() ? 3 : 4; // the passes of the multi-launch forms, the fourth under the same condition
#pragma nounroll
    for (int pass = 0; pass < passes; pass++)
    {
        uint32_t unused;
        lsd_rank_pass<DS_KB, DS_WAVES>(key, rk, 8 * pass, per, mine, wcnt, wtot, unused);
#pragma unroll
        for (int b = 0; b < DS_KB; b++)
            if (64 * b + lane < mine) { stage_k[rk[b]] = key[b]; stage_v[rk[b]] = val[b]; }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < DS_KB; b++) // (positions past `mine` hold stale pairs that nothing uses)
        {
            key[b] = stage_k[base + 64 * b + lane];
            val[b] = stage_v[base + 64 * b + lane];
        }
    }
    // the order, the tile counts in that order, their raw sums per scan block (64 consecutive positions never straddle a block of SB)
#pragma unroll
    for (int b = 0; b < DS_KB; b++)
    {
        if (64 * b >= per) continue;
        const int i = base + 64 * b + lane;
        unsigned long long tiles = 0;
        if (64 * b + lane < mine)
        {
            const uint32_t tt = g.tiles_touched[val[b]];
            g.sk[1][i] = key[b];
            g.sv[1][i] = val[b];
            g.tiles_sorted[i] = tt;
            tiles = tt;
        }
        tiles = wave_sum64(tiles);
        if (lane == 0 && tiles) atomicAdd(&bsum[(base + 64 * b) / SB], tiles);
    }
    __syncthreads();
    const int nblocks = (P + SB - 1) / SB;
    if (t < nblocks) g.blocksum[t] = bsum[t];
    if (t == 0) publish_instance_count(N, (unsigned long long *)g.blocksum + nblocks, g.top_const, false, host_out); // (= DepthCensus::n_out)
}

// ---- mid-sized scenes: the depth order by SAMPLED SPLITTERS + per-bucket sorts in LDS (round 6) -------------------------------------------------
// Above TS_DEPTH_SMALL_MAX triangles the LSD sort above is eight dependent launches (census histogram, four scatters, three histograms; the fourth
// pair returns at once on most scenes) + the launch of the block sums: 57 us for 0.7 MB of pairs at 93 k triangles, 59 at 300 k, 75 at 1 M --
// launch and load -> LDS -> store latency, not bytes.  Four launches instead:
//   K0  depth_split_sample_kernel   4096 keys taken at equal index strides (1024 below 150 k triangles: -2 us, and the buckets are small against K3's capacity
//                                   whatever their balance); workgroup b finds splitter b (the sample of rank 16 b + 15) by a radix select.
//                                   (Splitters from a SAMPLE, not from the key range: the buckets hold P / 256 +- 25 % pairs whatever the depth
//                                   distribution is -- a far background, an object that fills one octave -- where equal slices of the bit range
//                                   would put most of the scene into a few of them.)
//   K1  depth_split_hist_kernel     bucket(key) = number of splitters below the key (8-step search in LDS) -> a byte per key, the chunk's bucket
//                                   counts (table + per-slab totals, like rs_hist_direct_kernel), the chunk's part of N
//   K2  depth_split_scatter_kernel  a stable ticket-free scatter like rs_scatter_body's, with those bytes as the digit: (key, id) pairs bucket by
//                                   bucket in sk[0] / sv[0]; chunk 0 leaves the 256 bucket starts and publishes N (device word + pinned host word)
//   K3  depth_bucket_sort_kernel    one workgroup per bucket (4 waves below 300 k triangles, 16 above): its pairs in registers, a stable LSD sort in
//                                   LDS (lsd_rank_pass) on the bits of (key - smallest visible key of the bucket) that vary inside the bucket (13 of
//                                   them = two passes where the full key needs three or four), then what gather_blocksum_kernel did:
//                                   tiles_sorted and the raw block sums (64-bit atomics; the sums were cleared by K0).
// bucket() is monotone in the key and K2 is stable, K3 is a stable sort by the full key inside a bucket: sk[1] / sv[1] hold exactly the (key, id)
// order of the LSD passes -- checked form against form in tests/test_parity_gpu.py::test_split_depth_order_equals_the_multi_launch_forms.  A bucket
// larger than K3's registers (16 384 pairs: many equal or nearly equal depths) is sorted by the same workgroup through global memory, tile by tile --
// slow, correct.
// Measured against the LSD passes alternating on one box (profiles/r06_depth_split.txt): 93 k triangles 57 -> 43 us (step 0.335 -> 0.321 ms), 300 k
// 59 -> 47 (0.613 -> 0.605), 1 M 75 -> 65 us of kernels and NO difference in the step (the largest bucket holds 7 500 pairs = 8 steps x 2 passes of
// a ranking that is issue-bound with 16 waves on the compute unit: K3 takes 35 us there) -- hence the switch-over below.
#ifndef TS_DEPTH_SPLIT_MAX_VALUE // (variant builds: build.py --variant TAG --unit depth_order=-DTS_DEPTH_SPLIT_MAX_VALUE=1600000)
#define TS_DEPTH_SPLIT_MAX_VALUE 500000
#endif
constexpr int TS_DEPTH_SPLIT_MAX = TS_DEPTH_SPLIT_MAX_VALUE; // the product's switch-over: measured level with the LSD passes at 1 M triangles, ahead below
constexpr int TS_DEPTH_SPLIT_HARD_MAX = 1600000; // what the form supports (buckets of P / 256 pairs on average against DB_CAP = 16384): lab library, mode 2
constexpr int DSPL_SAMPLES = 4096, DSPL_SAMPLES_SMALL = 1024, DSPL_SMALL_BELOW = 150000; // below: P / 256 < 600 pairs per bucket against K3's 4096
constexpr int DB_WAVES = 16, DB_KB = 16, DB_CAP = 64 * DB_WAVES * DB_KB; // the large form of depth_bucket_sort_kernel
#ifndef TS_DB_SMALL_BELOW_VALUE
#define TS_DB_SMALL_BELOW_VALUE 300000
#endif
constexpr int DB_SMALL_WAVES = 4, DB_SMALL_BELOW = TS_DB_SMALL_BELOW_VALUE; // below: buckets of P / 256 < 1200 pairs on average against 4096
int g_depth_split_mode = 0; // lab library: 0 = by size, 1 = never (the LSD passes), 2 = up to TS_DEPTH_SPLIT_HARD_MAX
int g_depth_bucket_cap = DB_CAP; // lab library: a smaller register capacity sends ordinary buckets through K3's global-memory path

struct DepthSplit
{
    uint32_t *splitters;           // 256 words: splitter b, b < 255; [255] = ~0
    uint32_t *bucket_start;        // 256 words
    unsigned long long *chunk_sum; // per chunk: sum of tiles_touched
    uint8_t *digit;                // P bytes (lives in sv[1] until K3 overwrites it)
};
__host__ __device__ inline DepthSplit depth_split_of(const GeometryStateView &g)
{
    // scratch inside the state: `offsets` is written by scan_emit_kernel, after K3 (P > TS_DEPTH_SMALL_MAX words: room for 1024 + 2 chunks)
    DepthSplit d;
    d.splitters = g.offsets;
    d.bucket_start = g.offsets + NB;
    d.chunk_sum = (unsigned long long *)(g.offsets + 1024);
    d.digit = (uint8_t *)g.sv[1];
    return d;
}

// Depth keys are positive floats' bit patterns, and 0 for culled triangles.  Inside K0 and K3 the keys are taken relative to the smallest VISIBLE key
// (monotone; culled stay 0): the bytes that all visible keys share -- and that 0 does not -- then cost no pass.
__device__ __forceinline__ uint32_t depth_key_adjust(uint32_t key, uint32_t kmin_visible) { return key ? key - kmin_visible + 1u : 0u; }
__device__ __forceinline__ uint32_t depth_key_restore(uint32_t adj, uint32_t kmin_visible) { return adj ? adj - 1u + kmin_visible : 0u; }

// K0: workgroup b finds splitter b = the sample of rank DSPL_PER b + DSPL_PER - 1 by a radix SELECT over the samples it holds in registers
// (most-significant-digit passes: histogram of the candidates' digit in LDS, scan, the digit whose run holds the rank) -- 255 independent
// workgroups on an otherwise idle chip.  The select runs on (sample - smallest sample) and only over the bytes the samples' range needs: depth keys
// share their top bytes, and a pass on a byte that every sample shares is 4096 atomic adds on ONE LDS word (the same select over all four bytes
// of the raw keys: 12 us; one workgroup sorting the samples with a bitonic network: 13; eight workgroups ranking them by counting: 53).
template <int SAMPLES> // 4096, or 1024 for scenes whose buckets are small against K3's capacity whatever their balance
__global__ void __launch_bounds__(256) depth_split_sample_kernel(int P, GeometryStateView g, DepthSplit ds)
{
    constexpr int DSPL_SAMPLES = SAMPLES, DSPL_PER = SAMPLES / NB;
    __shared__ uint32_t hist[NB], wtot[4], pick[2], rmin[4], rmax[4];
    constexpr int K = DSPL_SAMPLES / 256;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t *keys = (const uint32_t *)g.depth;
    const int nblocks = (P + SB - 1) / SB;
    for (int i = blockIdx.x * 256 + t; i < nblocks; i += gridDim.x * 256) g.blocksum[i] = 0ull; // K3 adds into them
    uint32_t smp[K];
#pragma unroll
    for (int k = 0; k < K; k++) smp[k] = keys[(int)(((unsigned long long)(t + 256 * k) * (unsigned long long)P) / DSPL_SAMPLES)];
    // culled triangles carry key 0: they stay 0, the visible ones become key - (smallest visible key) + 1 (monotone)
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
    for (int k = 0; k < K; k++) { kmin = min(kmin, smp[k] ? smp[k] : 0xFFFFFFFFu); kmax = max(kmax, smp[k]); }
    for (int o = 32; o > 0; o >>= 1) { kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o)); kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o)); }
    if (lane == 0) { rmin[wave] = kmin; rmax[wave] = kmax; }
    __syncthreads();
    kmin = min(min(rmin[0], rmin[1]), min(rmin[2], rmin[3]));
    kmax = max(max(rmax[0], rmax[1]), max(rmax[2], rmax[3]));
    const uint32_t range = kmax ? kmax - kmin + 1u : 0u; // of the adjusted samples (no visible sample: all 0)
    const int top = range == 0u ? -8 : 8 * ((31 - __clz((int)range)) / 8); // shift of the highest byte in which two samples differ
#pragma unroll
    for (int k = 0; k < K; k++) smp[k] = depth_key_adjust(smp[k], kmin);
    uint32_t r = (uint32_t)(DSPL_PER * blockIdx.x + DSPL_PER - 1), prefix = 0u, mask = 0u;
#pragma unroll 1
    for (int shift = top; shift >= 0; shift -= 8)
    {
        hist[t] = 0u;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; k++)
            if ((smp[k] & mask) == prefix) atomicAdd(&hist[(smp[k] >> shift) & 0xFFu], 1u);
        __syncthreads();
        const uint32_t c = hist[t];
        const uint32_t inc = wave_inclusive_scan(c, lane);
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        uint32_t excl = inc - c;
        for (int w = 0; w < wave; w++) excl += wtot[w];
        if (excl <= r && r < excl + c) { pick[0] = (uint32_t)t; pick[1] = r - excl; } // exactly one digit's run holds the rank
        __syncthreads();
        prefix |= pick[0] << shift;
        mask |= 0xFFu << shift;
        r = pick[1];
    }
    if (t == 0) ds.splitters[blockIdx.x] = depth_key_restore(prefix, kmin);
    if (blockIdx.x == 0 && t == 1) ds.splitters[NB - 1] = 0xFFFFFFFFu;
}

// number of splitters below the key: the first index whose splitter is >= key (sp[255] = ~0 stops every search)
__device__ __forceinline__ uint32_t depth_bucket_of(const uint32_t *sp, uint32_t key)
{
    uint32_t lo = 0u;
#pragma unroll
    for (int step = NB / 2; step > 0; step >>= 1)
        lo += (sp[lo + step - 1] < key) ? step : 0u;
    return lo;
}

template <int CH>
__global__ void __launch_bounds__(256) depth_split_hist_kernel(int64_t n, GeometryStateView g, RadixScratchView r, uint32_t *__restrict__ acc, DepthSplit ds)
{
    __shared__ uint32_t bins[NB], sp[NB];
    __shared__ unsigned long long csum[4];
    const int t = threadIdx.x, chunk = rs_chunk_of_block(r.chunks);
    if (chunk < 0) return;
    bins[t] = 0u;
    sp[t] = ds.splitters[t];
    __syncthreads();
    const uint32_t *keys = (const uint32_t *)g.depth;
    const int64_t base = (int64_t)chunk * CH;
    unsigned long long tsum = 0;
#pragma unroll
    for (int b = 0; b < CH / 256; b++)
    {
        const int64_t i = base + 256 * b + t;
        if (i < n)
        {
            const uint32_t d = depth_bucket_of(sp, keys[i]);
            ds.digit[i] = (uint8_t)d;
            atomicAdd(&bins[d], 1u);
            tsum += g.tiles_touched[i];
        }
    }
    for (int o = 32; o > 0; o >>= 1) tsum += __shfl_xor(tsum, o);
    if ((t & 63) == 0) csum[t >> 6] = tsum;
    __syncthreads();
    const uint32_t c = bins[t];
    r.table[(size_t)chunk * NB + t] = c;
    if (c) __hip_atomic_fetch_add(acc + (size_t)(chunk >> 6) * NB + t, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 0) ds.chunk_sum[chunk] = csum[0] + csum[1] + csum[2] + csum[3];
}

// The digit is K1's byte (parked in LDS beside the pair, for the way out); the values are the ids
template <int CH>
__global__ void __launch_bounds__(256) depth_split_scatter_kernel(int64_t n, GeometryStateView g, RadixScratchView r, const uint32_t *__restrict__ acc, DepthSplit ds,
                                                                   unsigned long long *host_out)
{
    constexpr int KB = CH / 256;
    constexpr int SK = CH < 8 * NB ? 8 * NB : CH, SV = CH < 4 * NB ? 4 * NB : CH;
    __shared__ __attribute__((aligned(16))) uint32_t stage_k[SK], stage_v[SV];
    __shared__ uint8_t stage_d[CH];
    __shared__ uint32_t wcnt[4][NB];
    __shared__ int32_t gdelta[NB];
    __shared__ uint32_t wtot[4], gtot[4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int chunk = rs_chunk_of_block(r.chunks);
    if (chunk < 0) return;
    const uint32_t *kin = (const uint32_t *)g.depth;
    const int64_t base = (int64_t)chunk * CH + (int64_t)wave * (CH / 4);
    const int64_t here = n - base;
    const int mine = here >= CH / 4 ? CH / 4 : (here > 0 ? (int)here : 0);
    uint32_t key[KB], dg[KB], rk[KB];
#pragma unroll
    for (int b = 0; b < KB; b++)
    {
        const int i = 64 * b + lane;
        key[b] = 0xFFFFFFFFu;
        dg[b] = 0u;
        if (i < mine) { key[b] = kin[base + i]; dg[b] = ds.digit[base + i]; }
    }
    DirectPrefix prefix;
    prefix.load(r, acc, chunk, wave, lane);
#pragma unroll
    for (int k = 0; k < NB / 64; k++) wcnt[wave][lane + 64 * k] = 0u;
    wave_lds_order();
#pragma unroll
    for (int b = 0; b < KB; b++) rk[b] = wave_match_rank(dg[b], 64 * b + lane < mine, wcnt[wave]);
    prefix.park(stage_k, stage_v, wave, lane);
    __syncthreads();
    {
        uint32_t d_earlier, d_total, tot; // thread t = bucket t
        DirectPrefix::fold(stage_k, stage_v, t, d_earlier, d_total);
        const uint32_t dbase = digit_run_starts<4>(wcnt, wtot, wave, lane, tot);
        const uint32_t gbase = digit_exclusive_prefix<4>(d_total, gtot, wave, lane);
        gdelta[t] = (int32_t)(gbase + d_earlier - dbase);
        if (chunk == 0) ds.bucket_start[t] = gbase; // where bucket t begins in sk[0] / sv[0]
    }
    __syncthreads();
    const int64_t left = n - (int64_t)chunk * CH;
    const int count = left < CH ? (int)left : CH;
#pragma unroll
    for (int b = 0; b < KB; b++)
        if (64 * b + lane < mine)
        {
            const uint32_t p = wcnt[wave][dg[b]] + rk[b];
            stage_k[p] = key[b];
            stage_v[p] = (uint32_t)(base + 64 * b + lane);
            stage_d[p] = (uint8_t)dg[b];
        }
    __syncthreads();
    for (int p = t; p < count; p += 256)
    {
        const int64_t dst = (int64_t)gdelta[stage_d[p]] + p;
        g.sk[0][dst] = stage_k[p];
        g.sv[0][dst] = stage_v[p];
    }
    if (chunk == 0) // N = the chunks' sums of K1 (what publish_census does in the LSD form); the order is always in sk[1] / sv[1]: top_const = 0
    {
        __shared__ unsigned long long psum[4];
        unsigned long long sum = 0;
        for (int c = t; c < r.chunks; c += 256) sum += ds.chunk_sum[c];
        sum = wave_sum64(sum);
        if (lane == 0) psum[wave] = sum;
        __syncthreads();
        // behind the block sums K3 adds up (= DepthCensus::n_out)
        if (t == 0) publish_instance_count(psum[0] + psum[1] + psum[2] + psum[3], (unsigned long long *)g.blocksum + ((int)n + SB - 1) / SB, g.top_const, false, host_out);
    }
}

// What gather_blocksum_kernel does, for 64 consecutive depth-order positions (first one `pos0`, this lane's `pos`): the tile counts in depth order
// and their sums per scan block -- 64 consecutive positions meet at most two blocks; the sums were cleared by K0.
// `lsum` (fast path): the workgroup's scan-block sums in LDS, entry 0 = the block of the bucket's first position; they leave as ONE global atomic
// per (bucket, scan block) at the end (2 k atomics at 1 M triangles instead of 16 k, one or two per wave and step).  Null: straight to memory.
__device__ __forceinline__ void bucket_emit_tiles(const GeometryStateView &g, int pos0, int pos, bool in, uint32_t tt, int lane, uint32_t *lsum = nullptr,
                                                  int lblk0 = 0)
{
    if (in) g.tiles_sorted[pos] = tt;
    // 64 tile counts fit 32 bits together (their sum is at most N, and a forward with N >= 2^31 is refused on the host).  The positions grow with
    // the lane, so the lanes of the first scan block are a prefix of the wave: its sum is the inclusive scan at the last of them, the second block's
    // the rest -- one DPP scan (a 64-bit butterfly per block took 24 ds_bpermute per step).
    const int blk0 = pos0 / SB;
    const uint32_t inc = wave_inclusive_scan(in ? tt : 0u, lane);
    const int nfirst = min(64, (blk0 + 1) * SB - pos0); // lanes whose position lies in blk0 (>= 1)
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63), a = (uint32_t)__builtin_amdgcn_readlane((int)inc, nfirst - 1);
    if (lane == 0)
    {
        if (lsum)
        {
            if (a) atomicAdd(&lsum[blk0 - lblk0], a);
            if (total - a) atomicAdd(&lsum[blk0 - lblk0 + 1], total - a);
        }
        else
        {
            if (a) __hip_atomic_fetch_add((unsigned long long *)g.blocksum + blk0, (unsigned long long)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (total - a) __hip_atomic_fetch_add((unsigned long long *)g.blocksum + blk0 + 1, (unsigned long long)(total - a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

static_assert(2 * DB_CAP * 4 + DB_WAVES * NB * 4 + 1024 <= 160 * 1024 - 8 * 1024, "depth_bucket_sort_kernel: static LDS must leave 8 KB of the 160 KB");
// W waves per workgroup: 16 (64 KB + 64 KB of staging, one workgroup per compute unit) for buckets of thousands of pairs, 4 for the buckets of a
// few hundred that scenes below DB_SMALL_BELOW triangles have (a barrier among four waves, four columns per digit in the scan)
template <int W>
__global__ void __launch_bounds__(64 * W) depth_bucket_sort_kernel(int P, GeometryStateView g, DepthSplit ds, int cap)
{
    constexpr int DB_WAVES = W, DB_CAP = 64 * W * DB_KB;
    __shared__ __attribute__((aligned(16))) uint32_t stage_k[DB_CAP], stage_v[DB_CAP];
    __shared__ uint32_t wcnt[DB_WAVES][NB];
    __shared__ uint32_t wtot[4], rmin[DB_WAVES], rmax[DB_WAVES], dstart[NB];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int bucket = blockIdx.x;
    const int s0 = (int)ds.bucket_start[bucket], e0 = bucket + 1 < NB ? (int)ds.bucket_start[bucket + 1] : P;
    const int n = e0 - s0;
    if (n <= 0) return;
    const bool fits = n <= cap;
    // the whole bucket in registers when it fits (wave w: `per` consecutive positions, 64 per step); the key range either way
    const int per = ((n + 64 * DB_WAVES - 1) / (64 * DB_WAVES)) * 64;
    const int base = wave * per;
    const int mine = !fits ? 0 : (n - base < per ? (n - base > 0 ? n - base : 0) : per);
    uint32_t key[DB_KB], val[DB_KB], rk[DB_KB];
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u; // kmin: over the VISIBLE keys (depth_key_adjust)
    if (fits)
    {
        // branch-free loads (a lane past the end reads the bucket's first pair): all of a wave's steps are in flight together.  (With the loads under
        // `in ? load : constant` and the minimum taken in the same loop, every step waited for its predecessor: ten round trips in a row.)
#pragma unroll
        for (int b = 0; b < DB_KB; b++)
        {
            if (64 * b >= per) { key[b] = 0xFFFFFFFFu; val[b] = 0u; continue; } // wave-uniform
            const int i = 64 * b + lane;
            const int src = s0 + (i < mine ? base + i : 0);
            key[b] = g.sk[0][src];
            val[b] = g.sv[0][src];
        }
#pragma unroll
        for (int b = 0; b < DB_KB; b++)
        {
            const bool in = 64 * b + lane < mine;
            kmin = min(kmin, in && key[b] ? key[b] : 0xFFFFFFFFu);
            kmax = max(kmax, in ? key[b] : 0u);
        }
    }
    else
        for (int i = t; i < n; i += 64 * DB_WAVES)
        {
            const uint32_t k = g.sk[0][s0 + i];
            kmin = min(kmin, k ? k : 0xFFFFFFFFu);
            kmax = max(kmax, k);
        }
    wave_min_max(kmin, kmax);
    if (lane == 0) { rmin[wave] = kmin; rmax[wave] = kmax; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < DB_WAVES; w++) { kmin = min(kmin, rmin[w]); kmax = max(kmax, rmax[w]); }
    // sorted on the adjusted keys (culled 0, visible key - kmin + 1): `range` = the largest of them
    const uint32_t range = kmax ? kmax - kmin + 1u : 0u;
    const int kbits = range == 0u ? 0 : 32 - __clz((int)range), passes = (kbits + 7) / 8; // the bits that vary inside the bucket
    if (fits)
    {
#pragma unroll
        for (int b = 0; b < DB_KB; b++) key[b] = 64 * b + lane < mine ? depth_key_adjust(key[b], kmin) : 0xFFFFFFFFu;
    }
    if (fits)
    {
        // after every pass the pairs change owners through LDS
#pragma nounroll
        for (int pass = 0; pass < passes; pass++)
        {
            uint32_t unused;
            lsd_rank_pass<DB_KB, W>(key, rk, 8 * pass, per, mine, wcnt, wtot, unused);
#pragma unroll
            for (int b = 0; b < DB_KB; b++)
                if (64 * b + lane < mine) { stage_k[rk[b]] = key[b]; stage_v[rk[b]] = val[b]; }
            __syncthreads();
#pragma unroll
            for (int b = 0; b < DB_KB; b++)
                if (64 * b < per) { key[b] = stage_k[base + 64 * b + lane]; val[b] = stage_v[base + 64 * b + lane]; }
            __syncthreads();
        }
        // the tile counts of all steps are requested before anything else happens: one gather latency per wave, not one per step
#pragma unroll
        for (int b = 0; b < DB_KB; b++)
            rk[b] = 64 * b >= per ? 0u : g.tiles_touched[64 * b + lane < mine ? val[b] : 0u];
#pragma unroll
        for (int b = 0; b < DB_KB; b++)
        {
            if (64 * b >= per) continue;
            const int pos = s0 + base + 64 * b + lane;
            if (64 * b + lane < mine) { g.sk[1][pos] = depth_key_restore(key[b], kmin); g.sv[1][pos] = val[b]; }
        }
        // (a bucket of n <= DB_CAP pairs meets at most DB_CAP / SB + 2 scan blocks; a block's sum stays below N < 2^31)
        constexpr int LB = DB_CAP / SB + 2;
        uint32_t *lsum = dstart; // free on this path (NB >= LB words)
        static_assert(LB <= NB, "the scan-block sums borrow dstart");
        if (t < LB) lsum[t] = 0u;
        __syncthreads();
        const int lblk0 = s0 / SB;
#pragma unroll
        for (int b = 0; b < DB_KB; b++)
        {
            if (64 * b >= per) continue;
            bucket_emit_tiles(g, s0 + base + 64 * b, s0 + base + 64 * b + lane, 64 * b + lane < mine, 64 * b + lane < mine ? rk[b] : 0u, lane, lsum, lblk0);
        }
        __syncthreads();
        if (t < LB && lsum[t])
            __hip_atomic_fetch_add((unsigned long long *)g.blocksum + lblk0 + t, (unsigned long long)lsum[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    else
    {
        // larger than the registers: the same passes through global memory, tile after tile, between (sk[0], sv[0]) and (sk[1], sv[1]) of this
        // bucket's range (nobody else touches it); an odd number of passes ends in [1], an even one -- and a bucket of equal keys -- is copied
        const int tile = (cap & ~(64 * DB_WAVES - 1)) ? (cap & ~(64 * DB_WAVES - 1)) : 64 * DB_WAVES; // pairs per tile: whole 64-pair steps per wave
        int src = 0;
        for (int pass = 0; pass < passes; pass++, src ^= 1)
        {
            const uint32_t *kin = g.sk[src] + s0, *vin = g.sv[src] + s0;
            uint32_t *kout = g.sk[src ^ 1] + s0, *vout = g.sv[src ^ 1] + s0;
            if (t < NB) dstart[t] = 0u;
            __syncthreads();
            for (int i = t; i < n; i += 64 * DB_WAVES) atomicAdd(&dstart[(depth_key_adjust(peer_load(kin + i), kmin) >> (8 * pass)) & 0xFFu], 1u);
            __syncthreads();
            {
                const uint32_t start = digit_exclusive_prefix<W>(t < NB ? dstart[t] : 0u, wtot, wave, lane);
                if (t < NB) dstart[t] = start; // where digit t begins in the bucket
                __syncthreads();
            }
            for (int t0 = 0; t0 < n; t0 += tile)
            {
                const int nt = n - t0 < tile ? n - t0 : tile;
                const int tper = ((nt + 64 * DB_WAVES - 1) / (64 * DB_WAVES)) * 64;
                const int tbase = wave * tper;
                const int tmine = nt - tbase < tper ? (nt - tbase > 0 ? nt - tbase : 0) : tper;
#pragma unroll
                for (int b = 0; b < DB_KB; b++)
                {
                    const int i = 64 * b + lane;
                    const bool in = i < tmine;
                    key[b] = in ? depth_key_adjust(peer_load(kin + t0 + tbase + i), kmin) : 0xFFFFFFFFu; // past this compute unit's L1: an earlier pass of this workgroup wrote them
                    val[b] = in ? peer_load(vin + t0 + tbase + i) : 0u;
                }
                uint32_t tile_cnt;
                lsd_rank_pass<DB_KB, W>(key, rk, 8 * pass, tper, tmine, wcnt, wtot, tile_cnt);
                // rk = position inside the tile's (digit, order) arrangement; the digit's pairs of this tile go behind the earlier tiles' ones:
                // global position = dstart[d] + (rk - start of d inside the tile) = dstart[d] + rk - wcnt[0][d]
#pragma unroll
                for (int b = 0; b < DB_KB; b++)
                    if (64 * b + lane < tmine)
                    {
                        const uint32_t d = (key[b] >> (8 * pass)) & 0xFFu;
                        const uint32_t p = dstart[d] + rk[b] - wcnt[0][d];
                        peer_store(kout + p, depth_key_restore(key[b], kmin));
                        peer_store(vout + p, val[b]);
                    }
                __syncthreads();
                if (t < NB) dstart[t] += tile_cnt;
                __syncthreads();
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the next pass of this workgroup reads what other waves of it wrote to global memory
            __syncthreads();
        }
        if (src == 0)
            for (int i = t; i < n; i += 64 * DB_WAVES) { peer_store(g.sk[1] + s0 + i, peer_load(g.sk[0] + s0 + i)); peer_store(g.sv[1] + s0 + i, peer_load(g.sv[0] + s0 + i)); }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int i0 = 64 * wave; i0 < n; i0 += 64 * DB_WAVES)
        {
            const bool in = i0 + lane < n;
            bucket_emit_tiles(g, s0 + i0, s0 + i0 + lane, in, in ? g.tiles_touched[peer_load(g.sv[1] + s0 + i0 + lane)] : 0u, lane);
        }
    }
}
} // namespace

// Step 1: (depth bits, id) -> sorted ids.  Depth keys are view-space z of visible triangles (> 0, so the unsigned bit
// pattern is monotone) and 0 for culled ones, which emit nothing wherever they land.  `begin` = the launches that produce N (to `host_out`
// as well when given) and the key-bit census: the first histogram, and on the ticket-free path the first scatter too; `finish` = the other
// launches (the 4th pass returns at once when the census found the top byte constant: then sk[0] / sv[0] hold the order).
// The one-launch form (depth_order_small_kernel) -- never under the lab library's switches, which exist to run the multi-launch forms on small scenes.
#ifndef TS_DEPTH_SMALL_USE_VALUE // up to how many triangles the one-launch form is USED (<= its capacity TS_DEPTH_SMALL_MAX)
#define TS_DEPTH_SMALL_USE_VALUE 9216 // measured against the split form (variant builds, 256 x 256, graph replay): 3 k 17 vs 30 us, 5 k 22 vs 30, 10 k 32 vs 30 (step 0.133 -> 0.128 ms)
#endif
constexpr int TS_DEPTH_SMALL_USE = TS_DEPTH_SMALL_USE_VALUE;
static_assert(TS_DEPTH_SMALL_USE <= TS_DEPTH_SMALL_MAX && TS_DEPTH_SMALL_USE >= 2048, "the split form's scratch needs 1024 + 2 chunks words of `offsets`");
// Which form orders a scene of P triangles: the one-launch form up to TS_DEPTH_SMALL_USE, the sampled-splitter form from there to TS_DEPTH_SPLIT_MAX when
// the scratch takes the ticket-free passes, the LSD passes (ticket-free or, for the largest sorts, with tickets) beyond.  The lab library's switches
// that ask for the LSD forms (forced tickets, forced fourth pass, split mode 1) get them at every size.
enum class DepthForm { OneLaunch, Split, LsdDirect, LsdTickets };
static DepthForm depth_form(int32_t P, const RadixScratchView &r)
{
    const bool lsd_forced = ts_radix_tickets_forced() || g_force_pass4;
    if (P <= TS_DEPTH_SMALL_USE && !lsd_forced) return DepthForm::OneLaunch;
    if (!ts_radix_direct_ok(r)) return DepthForm::LsdTickets;
    const bool split = P > TS_DEPTH_SMALL_USE && P <= (g_depth_split_mode == 2 ? TS_DEPTH_SPLIT_HARD_MAX : TS_DEPTH_SPLIT_MAX) && g_depth_split_mode != 1;
    return split && !lsd_forced ? DepthForm::Split : DepthForm::LsdDirect;
}
void ts_sort_by_depth_begin(const GeometryStateView &g, int32_t P, unsigned long long *host_out, hipStream_t s)
{
    if (P <= 0) return;
    const DepthForm form = depth_form(P, g.rs);
    if (form == DepthForm::OneLaunch)
    {
        hipLaunchKernelGGL(depth_order_small_kernel, dim3(1), dim3(64 * DS_WAVES), 0, s, P, g, host_out);
        return;
    }
    if (form == DepthForm::Split)
    {
        const DepthSplit ds = depth_split_of(g);
        const dim3 grid((unsigned)g.rs.chunks);
        if (P < DSPL_SMALL_BELOW) hipLaunchKernelGGL(depth_split_sample_kernel<DSPL_SAMPLES_SMALL>, dim3(NB - 1), dim3(256), 0, s, P, g, ds);
        else hipLaunchKernelGGL(depth_split_sample_kernel<DSPL_SAMPLES>, dim3(NB - 1), dim3(256), 0, s, P, g, ds);
        TS_WITH_CHUNK(g.rs.chunk,
                      hipLaunchKernelGGL((depth_split_hist_kernel<CH>), grid, dim3(256), 0, s, (int64_t)P, g, g.rs, g.rs.slabacc[0], ds);
                      hipLaunchKernelGGL((depth_split_scatter_kernel<CH>), grid, dim3(256), 0, s, (int64_t)P, g, g.rs, (const uint32_t *)g.rs.slabacc[0], ds, host_out))
        return; // N is out; the buckets' sorts belong to `finish`
    }
    DepthCensus c;
    c.tiles_touched = g.tiles_touched;
    c.chunk_sum = (unsigned long long *)g.blocksum; // scratch: rewritten by gather_blocksum_kernel (chunks <= ceil(P / 1024))
    c.chunk_or = g.tiles_sorted;                    // scratch: rewritten by gather_blocksum_kernel / scan_emit_kernel
    c.chunk_and = g.offsets;
    c.n_out = (unsigned long long *)g.blocksum + (P + SB - 1) / SB;
    c.host_out = host_out;
    c.top_const = g.top_const;
    c.force_varying = g_force_pass4 ? 0xFF000000u : 0u;
    const dim3 grid((unsigned)g.rs.chunks);
    const uint32_t *keys = (const uint32_t *)g.depth;
    const unsigned long long *no_count = nullptr;
    const uint32_t *no_vals = nullptr, *no_skip = nullptr;
    if (form == DepthForm::LsdTickets) // the hierarchical histogram with the census riding along; its scatter belongs to `finish`
    {
        TS_WITH_CHUNK(g.rs.chunk, hipLaunchKernelGGL((rs_hist_kernel<true, CH>), grid, dim3(256), 0, s, keys, (int64_t)P, no_count, 0, 0xFFu, g.rs, c, no_skip))
        return;
    }
    // ticket-free: the histogram (with the census) adds into slabacc[0], which the step's first launch cleared (clear_tickets); the first
    // scatter belongs to `begin` because its block 0 publishes the census
    TS_WITH_CHUNK(g.rs.chunk,
                  hipLaunchKernelGGL((rs_hist_census_direct_kernel<CH>), grid, dim3(256), 0, s, keys, (int64_t)P, 0xFFu, g.rs, g.rs.slabacc[0], c);
                  hipLaunchKernelGGL((rs_scatter_kernel<true, CH, true, true>), grid, dim3(256), 0, s, keys, no_vals, g.sk[0], g.sv[0], (int64_t)P, no_count, 0, 8,
                                     g.rs, no_skip, (const uint32_t *)g.rs.slabacc[0], g.rs.slabacc[1], c))
}
void ts_sort_by_depth_finish(const GeometryStateView &g, int32_t P, hipStream_t s)
{
    if (P <= 0) return;
    switch (depth_form(P, g.rs))
    {
    case DepthForm::OneLaunch: return;
    case DepthForm::Split:
        if (P < DB_SMALL_BELOW)
            hipLaunchKernelGGL(depth_bucket_sort_kernel<DB_SMALL_WAVES>, dim3(NB), dim3(64 * DB_SMALL_WAVES), 0, s, P, g, depth_split_of(g),
                               min(g_depth_bucket_cap, 64 * DB_SMALL_WAVES * DB_KB));
        else hipLaunchKernelGGL(depth_bucket_sort_kernel<DB_WAVES>, dim3(NB), dim3(64 * DB_WAVES), 0, s, P, g, depth_split_of(g), g_depth_bucket_cap);
        return;
    case DepthForm::LsdTickets:
        ts_radix_scatter((const uint32_t *)g.depth, nullptr, g.sk[0], g.sv[0], P, nullptr, 0, 8, g.rs, s);
        ts_radix_pass(g.sk[0], g.sv[0], g.sk[1], g.sv[1], P, nullptr, 8, 8, g.rs, s);
        ts_radix_pass(g.sk[1], g.sv[1], g.sk[0], g.sv[0], P, nullptr, 16, 8, g.rs, s);
        ts_radix_pass(g.sk[0], g.sv[0], g.sk[1], g.sv[1], P, nullptr, 24, 8, g.rs, s, g.top_const);
        return;
    case DepthForm::LsdDirect:
        ts_radix_pass_direct(g.sk[0], g.sv[0], g.sk[1], g.sv[1], P, nullptr, 8, 8, g.rs, 1, s);
        ts_radix_pass_direct(g.sk[1], g.sv[1], g.sk[0], g.sv[0], P, nullptr, 16, 8, g.rs, 0, s);
        ts_radix_pass_direct(g.sk[0], g.sv[0], g.sk[1], g.sv[1], P, nullptr, 24, 8, g.rs, 1, s, g.top_const);
        return;
    }
}

// Step 2: tiles_sorted = tiles_touched[perm], raw block sums (+ their groups' sums above 2048 blocks, or always under the lab library's
// ts2d_lab_force_ticket_passes, so that the suite runs the two-level form on small scenes); blocksum[nblocks] = N comes from the census.
bool ts_scan_two_level(int32_t P) { return ts_radix_tickets_forced() || (P + SB - 1) / SB > 2048; }
void ts_scan_offsets(const GeometryStateView &g, int32_t P, hipStream_t s)
{
    if (P <= 0) return;
    switch (depth_form(P, g.rs))
    {
    case DepthForm::OneLaunch:
    case DepthForm::Split: return; // depth_order_small_kernel / depth_bucket_sort_kernel left tiles_sorted and the block sums behind
    case DepthForm::LsdDirect:
    case DepthForm::LsdTickets: break;
    }
    hipLaunchKernelGGL(gather_blocksum_kernel, dim3((unsigned)((P + SB - 1) / SB)), dim3(256), 0, s, P, g, ts_scan_two_level(P));
}

void ts_force_depth_pass4(bool on) { g_force_pass4 = on; }
void ts_lab_depth_split(int mode, int bucket_cap)
{
    g_depth_split_mode = mode;
    g_depth_bucket_cap = bucket_cap > 0 && bucket_cap < DB_CAP ? bucket_cap : DB_CAP;
}
