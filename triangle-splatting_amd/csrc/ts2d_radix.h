// ts2d_radix.h -- what the three binning units share: depth_order.hip (steps 1-2 below), emit.hip (steps 3 and 5), radix_sort.hip (step 4 and
// the same sort for other callers).  Depth ordering, instance emission, tile grouping and tile ranges, all hand-written for gfx950.
//
// Result contract (integer-exact, what the blend kernels and the parity tests rely on): the instance list is ordered
// by (tile id, depth bit pattern, triangle id) -- exactly what the reference obtains with cub::DeviceScan::InclusiveSum
// + duplicateWithKeys + one stable cub::DeviceRadixSort::SortPairs over N 64-bit (tile << 32 | depth) keys +
// identifyTileRanges (R2D/src/rasterizer.cu:186, 37-75, 210-218, 79-99).
//
// How it is obtained here (same order, ~4.5x less sort traffic; N ~ 4.6 x P for the headline scene):
//   1. stable radix sort of the P triangles by their 32-bit depth key (values = ascending ids): 3-4 passes x P pairs; the first histogram
//      also produces N = sum(tiles_touched) (the one value the host reads back) and finds out whether the fourth pass can be skipped;
//   2. tiles_touched gathered in that order + block sums;
//   3. per block: wave64 prefix scan (DPP) of the tile counts on top of the block sums in front -> instance slots, and (tile, id)
//      instances emitted in depth order through LDS; the same kernel clears the tile ranges and the contribution statistics;
//   4. stable radix sort of the N instances by TILE ID ONLY (13 bits at 1080p -> 2 passes x N x 8 B instead of
//      6 passes x N x 12 B); stability keeps the depth order (and the id order among equal depths) inside a tile;
//   5. tile ranges from the sorted tile ids.
//
// One radix pass (digit of up to 8 bits) = two kernels, no look-back spinning.  Two flavours of the first one:
//   rs_hist_direct  (sorts of up to 48 slabs = 12.6 M pairs: everything the headline runs) one workgroup per chunk of 2048 / 4096 pairs
//               counts its digits in a 1 KB LDS table (ds_add_u32), stores the 256 counts as a raw table row and adds them to its slab's
//               totals with fire-and-forget atomics.  Nobody waits for anybody: the scatter kernel works out its prefixes itself
//               (<= 63 rows of its slab + the slabs' totals, requested while its keys are on their way);
//   rs_hist     (larger sorts) the workgroup that arrives LAST in its slab of 64 chunks (one atomic ticket; the counts travel as
//               write-through stores and L1-bypassing loads, so no L2 write-back fence is needed) turns the slab's rows into
//               exclusive column prefixes, and the last slab to finish does the same over the slab totals and over the 256 digit totals.
//               Its cost does not grow with the slab count, but the elected block walks seven dependent memory round trips alone:
//               18 us at 1 M keys, which is why the small sorts left it;
//   rs_scatter  the workgroup re-reads its chunk (each wave a contiguous quarter, 64 pairs per step): the lanes holding equal
//               digits find each other with one ballot per digit bit (wave64 match), rank = v_mbcnt of the match mask on top of the
//               digit's running count; the pairs are parked in LDS in chunk-local sorted order and leave as coalesced runs.  Ranks
//               follow lane order, steps follow list order, waves follow chunk order: stable by construction.
// The same rule removed the elected blocks from the scan (raw block sums, added up by the emission blocks) and from the census (published
// by block 0 of the first scatter).  The round-1 rocPRIM calls (radix_sort_pairs, inclusive_scan) survive only as the comparators of
// tests/test_binning_gpu.py.
// Every form of step 1 (depth_order.hip) ranks with the same pieces, each defined once here: wave_match_rank (the 64-pair step),
// digit_exclusive_prefix / digit_run_starts (counts -> run starts), lsd_rank_pass (a pass of a workgroup that holds its pairs in registers),
// DirectPrefix (the ticket-free prefixes), KeyCensus / publish_instance_count (N and the fourth-pass verdict).
// Everything device-side sits in an unnamed namespace: a kernel is instantiated by the one unit that launches it, and what crosses a unit
// boundary is a host function declared at the end of this file or in ts2d_common.h.
#pragma once
#include "ts2d_common.h"
#include "ts2d_wave.h"

namespace
{
constexpr int NB = TS_RS_BINS;
constexpr int SB = 1024; // triangles per scan block (256 threads x 4): steps 2 and 3

__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, int lane) // DPP row shifts + two row broadcasts
{
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true); // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true); // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true); // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true); // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, true); // row_bcast:15 -> rows 1 and 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, true); // row_bcast:31 -> rows 2 and 3
    return (uint32_t)x;
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) // on every lane
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ void wave_min_max(uint32_t &lo, uint32_t &hi) // on every lane
{
    for (int o = 32; o > 0; o >>= 1)
    {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, o));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, o));
    }
}

// ---- the pieces every form of the stable radix ranking is made of ----------------------------------------------------------------------------------
// Stable ranks of one step of 64 pairs: returns how many pairs with this lane's digit `d` (< 256; the caller decides which bits of its key that is)
// the wave has ranked before -- in earlier steps (`cnt`, the wave's 256 LDS counters, advanced here) and in lower lanes of this one.  The lanes
// holding equal digits find each other with one ballot per digit bit (wave64 match); ranks follow lane order, steps follow list order.
__device__ __forceinline__ uint32_t wave_match_rank(uint32_t d, bool valid, uint32_t *cnt)
{
    // lanes whose digit differs from mine in some bit: (ballot of bit i) xor (my bit i, sign-extended), or-ed over the bits, in two 32-bit
    // halves -- three instructions per bit and half (round 5; the select form `m &= one ? bb : ~bb` compiled to ~100 instructions per step,
    // and a launch of a few resident workgroups per SIMD -- or ONE workgroup on one compute unit -- spends a good part of its time issuing exactly these)
    const unsigned long long vm = ballot64(valid);
    uint32_t mis_lo = ~(uint32_t)vm, mis_hi = ~(uint32_t)(vm >> 32);
    // all eight bits, unrolled, however many the digit has (the bits above them are zero in every lane and cost a ballot that changes nothing): with
    // the bit index a compile-time constant a bit is four instructions (v_bfe_i32, the compare behind the ballot, two fused xor-or); as a loop
    // over a run-time bit count it was twelve (shift by an SGPR, select, loop control, two s_nop) -- 96 of the ~135 instructions of a 64-pair
    // step, in kernels whose time IS this ranking (round 6: profiles/r06_rank_unroll.txt)
#pragma unroll
    for (int bit = 0; bit < 8; bit++)
    {
        const unsigned long long bb = ballot64((d >> bit) & 1u);
        const uint32_t e = (uint32_t)__builtin_amdgcn_sbfe((int)d, bit, 1); // all ones when my bit is set
        mis_lo |= (uint32_t)bb ^ e;
        mis_hi |= (uint32_t)(bb >> 32) ^ e;
    }
    const uint32_t m_lo = ~mis_lo, m_hi = ~mis_hi; // the valid lanes that hold my digit
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi(m_hi, __builtin_amdgcn_mbcnt_lo(m_lo, 0u));
    const uint32_t c = (uint32_t)(__popc(m_lo) + __popc(m_hi));
    uint32_t seen = 0;
    if (valid) seen = cnt[d];
    wave_lds_order(); // every lane has read its digit's count before the group leaders advance it
    if (valid && rank == c - 1u) cnt[d] = seen + c;
    wave_lds_order();
    return seen + rank;
}

// Exclusive prefix over the 256 digits of `total` in a workgroup of W waves (thread d < 256: digit d; the threads of waves 4 and up come along for
// the barrier): wave64 DPP scan + the preceding waves' totals, which meet in wtot[4].
template <int W>
__device__ __forceinline__ uint32_t digit_exclusive_prefix(uint32_t total, uint32_t *wtot, int wave, int lane)
{
    const bool digit = W <= 4 || wave < NB / 64;
    uint32_t inc = 0u;
    if (digit)
    {
        inc = wave_inclusive_scan(total, lane);
        if (lane == 63) wtot[wave] = inc;
    }
    __syncthreads();
    uint32_t excl = inc - total;
    if (digit)
        for (int w = 0; w < wave; w++) excl += wtot[w];
    return excl;
}
// The W waves' counts of digit t (wcnt[w][t], complete: barrier before) -> where the run of every (wave, digit) starts in (digit, wave) order, left in
// wcnt (barrier after).  Returns the start of digit t's first run; `total` = the digit's count over the waves.
template <int W>
__device__ __forceinline__ uint32_t digit_run_starts(uint32_t (*wcnt)[NB], uint32_t *wtot, int wave, int lane, uint32_t &total)
{
    const int t = 64 * wave + lane;
    const bool digit = W <= 4 || wave < NB / 64;
    uint32_t c[W], tot = 0u;
    if (digit)
    {
#pragma unroll
        for (int w = 0; w < W; w++) { c[w] = wcnt[w][t]; tot += c[w]; }
    }
    const uint32_t start = digit_exclusive_prefix<W>(tot, wtot, wave, lane);
    if (digit)
    {
        uint32_t run = start;
#pragma unroll
        for (int w = 0; w < W; w++) { wcnt[w][t] = run; run += c[w]; }
    }
    total = tot;
    return start;
}

// One stable LSD pass, on digit (key >> shift) & 255, of a workgroup of W waves over the pairs it holds in registers (wave w: `mine` of the `per`
// positions [w per, (w + 1) per) of the list, 64 consecutive ones per step).  Leaves in rk[] every pair's position in the list's (digit, wave,
// step, lane) order -- the caller exchanges the pairs through LDS on it -- and in `digit_count` (thread d < 256) how many pairs hold digit d.
template <int KBX, int W>
__device__ __forceinline__ void lsd_rank_pass(const uint32_t (&key)[KBX], uint32_t (&rk)[KBX], int shift, int per, int mine, uint32_t (*wcnt)[NB],
                                              uint32_t *wtot, uint32_t &digit_count)
{
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    uint32_t *cnt = wcnt[wave];
#pragma unroll
    for (int k = 0; k < NB / 64; k++) cnt[lane + 64 * k] = 0u;
    wave_lds_order();
#pragma unroll
    for (int b = 0; b < KBX; b++)
    {
        if (64 * b >= per) continue; // wave-uniform
        rk[b] = wave_match_rank((key[b] >> shift) & 0xFFu, 64 * b + lane < mine, cnt);
    }
    __syncthreads();
    digit_run_starts<W>(wcnt, wtot, wave, lane, digit_count);
    __syncthreads();
#pragma unroll
    for (int b = 0; b < KBX; b++)
        if (64 * b + lane < mine) rk[b] += cnt[(key[b] >> shift) & 0xFFu];
}

// The ticket-free ("DIRECT") prefixes of a scatter block: how many pairs of each digit sit in earlier chunks of its slab (`within`, from the raw table
// rows), in earlier slabs (`before`) and in all slabs (`total`, both from the slabs' totals `acc`).
constexpr int TS_DIRECT_MAX_SLABS = 48; // every scatter block reads the totals of all slabs: beyond this the hierarchical pass is cheaper
struct DirectPrefix
{
    uint4 within = make_uint4(0u, 0u, 0u, 0u), before = make_uint4(0u, 0u, 0u, 0u), total = make_uint4(0u, 0u, 0u, 0u);
    // Wave w takes every fourth row, lane l the digits 4l .. 4l + 3 (one dwordx4 per row: at most 16 + 12 loads per lane, all requested here -- the
    // caller puts this behind its key loads and its ranking in front of park())
    __device__ __forceinline__ void load(const RadixScratchView &r, const uint32_t *__restrict__ acc, int chunk, int wave, int lane)
    {
        const int slab = chunk >> 6, c0 = slab * 64;
        const uint4 *tab4 = (const uint4 *)r.table + (size_t)c0 * (NB / 4) + lane;
        const uint4 *acc4 = (const uint4 *)acc + lane;
#pragma unroll 4
        for (int k = 0; k < 16; k++)
        {
            const int c = wave + 4 * k;
            if (c0 + c < chunk)
            {
                const uint4 v = tab4[(size_t)c * (NB / 4)];
                within.x += v.x; within.y += v.y; within.z += v.z; within.w += v.w;
            }
        }
#pragma unroll 4
        for (int k = 0; k < TS_DIRECT_MAX_SLABS / 4; k++)
        {
            const int sl = wave + 4 * k;
            if (sl < r.slabs)
            {
                const uint4 v = acc4[(size_t)sl * (NB / 4)];
                total.x += v.x; total.y += v.y; total.z += v.z; total.w += v.w;
                if (sl < slab) { before.x += v.x; before.y += v.y; before.z += v.z; before.w += v.w; }
            }
        }
    }
    // the four waves' partial sums meet in LDS: 8 x 256 words at `x` (within, before) and 4 x 256 at `xtotal`; barrier, then fold()
    __device__ __forceinline__ void park(uint32_t *x, uint32_t *xtotal, int wave, int lane) const
    {
        *(uint4 *)(x + wave * NB + 4 * lane) = within;
        *(uint4 *)(x + (4 + wave) * NB + 4 * lane) = before;
        *(uint4 *)(xtotal + wave * NB + 4 * lane) = total;
    }
    // digit t: pairs in earlier chunks of the grid (within + before) and in the whole array
    static __device__ __forceinline__ void fold(const uint32_t *x, const uint32_t *xtotal, int t, uint32_t &d_earlier, uint32_t &d_total)
    {
        uint32_t d_within = 0u, d_before = 0u;
        d_total = 0u;
#pragma unroll
        for (int w = 0; w < 4; w++)
        {
            d_within += x[w * NB + t];
            d_before += x[(4 + w) * NB + t];
            d_total += xtotal[w * NB + t];
        }
        d_earlier = d_before + d_within;
    }
};

// Elects the block that arrives last at `ticket` among `count` arrivals; the elected block resets the ticket for the next
// launch and returns true on all of its threads.  Data handed to the elected block travels as write-through (sc0 sc1) stores and
// L1-bypassing (sc1) loads on both sides (peer_store / peer_load): with every store drained (s_waitcnt vmcnt(0)) before the ticket
// is taken, no L2 write-back fence is needed (MI355X_MICROARCH.md, "valid forms": a release fence per block costs 2-6 us).
// This is a HARDWARE contract of gfx950 (write-through sc0 sc1 stores + drain on the producer, sc1 loads on the consumer, both relaxed in
// the language's memory model), not something the HIP memory model promises: hence the target check below, and
// tests/test_binning_gpu.py::test_last_arrival_handoffs_under_uneven_load hammers every hand-off next to a noisy neighbour stream.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "last_arrival() relies on gfx950's write-through store / L1-bypassing load behaviour; re-validate before building for another target"
#endif
__device__ __forceinline__ bool last_arrival(uint32_t *ticket, uint32_t count)
{
    __shared__ bool elected;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0)
    {
        const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        elected = (t == count - 1u);
        if (elected) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return elected;
}
template <typename T>
__device__ __forceinline__ T peer_load(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ void peer_store(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// triangle ids in (depth, id) order: the 4th pass's output, or the 3rd's when the 4th was skipped (written by an earlier launch)
__device__ __forceinline__ const uint32_t *sorted_ids(const GeometryStateView &g) { return *g.top_const ? g.sv[0] : g.sv[1]; }

// Sync-free forward (ts2d_forward): the pair count lives on the device.  `n_dev` (null on the synchronous path) points at the
// 64-bit instance count the scan left behind; a count above `n` (the capacity the buffers were carved for) renders nothing and is
// reported through the state's status word.  The launch covers the capacity; blocks past the actual count return at once.
template <int CH>
__device__ __forceinline__ bool resolve_count(const unsigned long long *n_dev, int64_t &n, RadixScratchView &r)
{
    if (n_dev)
    {
        const unsigned long long live = *n_dev;
        n = (live <= (unsigned long long)n) ? (int64_t)live : 0;
        r.chunks = (int)((n + CH - 1) / CH);
        r.slabs = (r.chunks + 63) / 64;
    }
    return (int)blockIdx.x < 8 * ((r.chunks + 7) / 8);
}
// Which chunk a workgroup of a radix pass works on.  Workgroups go to the 8 XCDs round-robin (block b -> XCD b % 8); XCD x takes the chunks
// [x n / 8, (x + 1) n / 8): consecutive chunks write adjacent pieces of every digit's run (32 - 64 elements = one or two cache lines each),
// and with ONE XCD behind both halves of a shared line the two partial writes meet in one L2 instead of two (round 4: tile sort 73 -> 69 us,
// depth sort 48 -> 45 us against chunk = blockIdx, measured and dropped: profiles/r04_notes.md).  The partition follows the LIVE chunk count, so a launch that
// covers a larger capacity (speculative / sync-free forward) stays balanced over the XCDs.
__device__ __forceinline__ int rs_chunk_of_block(int nchunks)
{
    const int q = nchunks >> 3, r = nchunks & 7, x = blockIdx.x & 7, i = blockIdx.x >> 3;
    return i < q + (x < r ? 1 : 0) ? x * q + min(x, r) + i : -1;
}

// Digit counts of every chunk, and -- by the blocks that arrive last -- their prefixes: the last block of a slab (64 chunks)
// turns the slab's rows into exclusive column prefixes and its totals; the last slab to finish turns the slab totals into
// their prefix over the slabs and forms the exclusive prefix of the 256 digit totals.  One launch, no spinning.
//
// The FIRST pass of the depth sort (CENSUS) also takes stock of what it reads anyway (round 3: two launches and one pass fewer per step):
//   * N = sum(tiles_touched), the instance count the host is waiting for (the reference hands num_rendered to the host,
//     rasterizer.cu:189-191); it does not depend on the depth order, so it leaves as soon as this kernel is done -- through a pinned host
//     word -- while the rest of the sort runs (round 2 spent a kernel of its own on it);
//   * which key bits differ between VISIBLE triangles (culled ones carry key 0 and emit nothing wherever they land): depths are positive
//     floats, and when they all share their top byte -- sign + seven exponent bits: every scene whose depths span less than a factor
//     of four -- the fourth pass has nothing to order.  The verdict goes to `census->top_const`; the last pass's kernels return at once
//     when it is set and the consumers of the order take the third pass's output (sorted_ids()).
struct DepthCensus
{
    const uint32_t *tiles_touched; // per key
    unsigned long long *chunk_sum; // per chunk (scratch)
    uint32_t *chunk_or, *chunk_and; // per chunk (scratch)
    unsigned long long *n_out;     // device: where the scan will leave N as well
    unsigned long long *host_out;  // pinned host word or null
    uint32_t *top_const;           // device flag
    uint32_t force_varying;        // lab library only (ts2d_lab_force_depth_pass4): key bits reported as varying whatever the scene holds
};
__device__ __forceinline__ bool pass_skipped(const uint32_t *skip_flag) { return skip_flag && peer_load(skip_flag) != 0u; }
// What the depth sort's first pass takes stock of (see above): the sum of the tile counts and which key bits differ between VISIBLE keys.
struct KeyCensus
{
    unsigned long long tiles = 0ull;
    uint32_t kor = 0u, kand = 0xFFFFFFFFu;
    __device__ __forceinline__ void add(uint32_t key, uint32_t tiles_touched)
    {
        tiles += tiles_touched;
        if (key != 0u) { kor |= key; kand &= key; } // culled triangles (key 0) emit nothing wherever they land: they do not count
    }
    __device__ __forceinline__ void combine(unsigned long long s, uint32_t o, uint32_t a) { tiles += s; kor |= o; kand &= a; }
    __device__ __forceinline__ void wave_fold() // on every lane
    {
        for (int d = 32; d > 0; d >>= 1) combine(__shfl_xor(tiles, d), __shfl_xor(kor, d), __shfl_xor(kand, d));
    }
    // The waves' folded censuses meet in three LDS arrays of the caller: park (barrier) gather
    __device__ __forceinline__ void park(unsigned long long *s, uint32_t *o, uint32_t *a) const
    {
        if ((threadIdx.x & 63) == 0) { s[threadIdx.x >> 6] = tiles; o[threadIdx.x >> 6] = kor; a[threadIdx.x >> 6] = kand; }
    }
    template <int W>
    static __device__ __forceinline__ KeyCensus gather(const unsigned long long *s, const uint32_t *o, const uint32_t *a)
    {
        KeyCensus c;
#pragma unroll
        for (int w = 0; w < W; w++) c.combine(s[w], o[w], a[w]);
        return c;
    }
    // Depths are positive floats: when all visible keys share their top byte the fourth pass has nothing to order.  No visible triangle at all:
    // or = 0, and = ~0 -> every bit varies -> false.  `force_varying`: DepthCensus
    __device__ __forceinline__ bool top_byte_constant(uint32_t force_varying = 0u) const { return (((kor ^ kand) | force_varying) >> 24) == 0u; }
};
// N and the verdict on the fourth pass leave as soon as they are known.  `host_out`: a pinned, device-visible host word or null; the host reads it
// after the event recorded behind the kernel (no copy kernel in between).  PEER: the ticket path's write-through store of the verdict.
template <bool PEER = false>
__device__ __forceinline__ void publish_instance_count(unsigned long long N, unsigned long long *n_out, uint32_t *top_const, bool verdict,
                                                       unsigned long long *host_out)
{
    *n_out = N;
    if (PEER) peer_store(top_const, verdict ? 1u : 0u);
    else *top_const = verdict ? 1u : 0u;
    if (host_out) __hip_atomic_store(host_out, N, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <bool CENSUS, int CH>
__global__ void __launch_bounds__(256) rs_hist_kernel(const uint32_t *__restrict__ keys, int64_t n, const unsigned long long *n_dev, int shift,
                                                       uint32_t mask, RadixScratchView r, DepthCensus census, const uint32_t *skip_flag)
{
    __shared__ uint32_t bins[NB];
    __shared__ unsigned long long csum[4];
    __shared__ uint32_t cor[4], cand[4];
    if (!resolve_count<CH>(n_dev, n, r)) return;
    if (!CENSUS && pass_skipped(skip_flag)) return;
    const int t = threadIdx.x, chunk = rs_chunk_of_block(r.chunks);
    if (chunk < 0) return;
    bins[t] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)chunk * CH;
    KeyCensus mine;
#pragma unroll 4
    for (int b = 0; b < CH / 256; b++)
    {
        const int64_t i = base + 256 * b + t;
        if (i < n)
        {
            const uint32_t k = keys[i];
            atomicAdd(&bins[(k >> shift) & mask], 1u);
            if (CENSUS) mine.add(k, census.tiles_touched[i]);
        }
    }
    if (CENSUS)
    {
        mine.wave_fold();
        mine.park(csum, cor, cand);
    }
    __syncthreads();
    peer_store(r.table + (size_t)chunk * NB + t, bins[t]);
    if (CENSUS && t == 0)
    {
        const KeyCensus c = KeyCensus::gather<4>(csum, cor, cand);
        peer_store(census.chunk_sum + chunk, c.tiles);
        peer_store(census.chunk_or + chunk, c.kor);
        peer_store(census.chunk_and + chunk, c.kand);
    }

    const int slab = chunk >> 6, c0 = slab * 64, c1 = min(r.chunks, c0 + 64);
    if (!last_arrival(r.tickets + 2 + slab, (uint32_t)(c1 - c0))) return;
    uint32_t run = 0;
    {
        // the elected block is alone on the launch's critical path: all 64 rows of the slab are requested before the first one is used
        // (one memory round trip instead of four)
        uint32_t v[64];
#pragma unroll
        for (int k = 0; k < 64; k++) v[k] = (c0 + k < c1) ? peer_load(r.table + (size_t)(c0 + k) * NB + t) : 0u;
#pragma unroll
        for (int k = 0; k < 64; k++)
        {
            if (c0 + k < c1) r.table[(size_t)(c0 + k) * NB + t] = run;
            run += v[k];
        }
    }
    peer_store(r.slabtot + (size_t)slab * NB + t, run);

    if (!last_arrival(r.tickets, (uint32_t)r.slabs)) return;
    uint32_t total = 0;
    for (int s = 0; s < r.slabs; s += 32)
    {
        uint32_t v[32];
#pragma unroll
        for (int k = 0; k < 32; k++) v[k] = (s + k < r.slabs) ? peer_load(r.slabtot + (size_t)(s + k) * NB + t) : 0u;
#pragma unroll
        for (int k = 0; k < 32; k++)
        {
            if (s + k < r.slabs) r.slabtot[(size_t)(s + k) * NB + t] = total;
            total += v[k];
        }
    }
    __shared__ uint32_t wtot[4];
    r.binbase[t] = digit_exclusive_prefix<4>(total, wtot, t >> 6, t & 63);
    if (CENSUS)
    {
        // this block arrived last of all: every chunk's census is visible (same hand-off as the digit counts)
        KeyCensus all;
        for (int c = t; c < r.chunks; c += 256) all.combine(peer_load(census.chunk_sum + c), peer_load(census.chunk_or + c), peer_load(census.chunk_and + c));
        all.wave_fold();
        __syncthreads();
        all.park(csum, cor, cand);
        __syncthreads();
        if (t == 0)
        {
            all = KeyCensus::gather<4>(csum, cor, cand);
            publish_instance_count<true>(all.tiles, census.n_out, census.top_const, all.top_byte_constant(census.force_varying), census.host_out);
        }
    }
}

// Ticket-free histogram (round 3): a pass of the hierarchical version above is a chain of seven dependent memory round trips (keys ->
// counts -> ticket -> slab rows -> ticket -> slab totals -> prefixes) that one elected block walks alone while the chip idles; at 1 M keys
// that chain IS the kernel (18 us for 4 MB of keys).  Here a block leaves its 256 counts as a table row and adds them to its slab's totals
// with fire-and-forget atomics, and that is all; the scatter kernel that follows works out the three prefixes it needs from the rows
// (<= 63 rows of its slab + the slabs' totals, loaded while its keys are on their way).
template <int CH>
__global__ void __launch_bounds__(256) rs_hist_direct_kernel(const uint32_t *__restrict__ keys, int64_t n, const unsigned long long *n_dev, int shift,
                                                              uint32_t mask, RadixScratchView r, uint32_t *__restrict__ acc, const uint32_t *skip_flag)
{
    __shared__ uint32_t bins[NB];
    if (!resolve_count<CH>(n_dev, n, r)) return;
    if (pass_skipped(skip_flag)) return;
    const int t = threadIdx.x, chunk = rs_chunk_of_block(r.chunks);
    if (chunk < 0) return;
    bins[t] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)chunk * CH;
#pragma unroll
    for (int b = 0; b < CH / 1024; b++) // one dwordx4 per thread and round (the counts do not care about the order inside the chunk)
    {
        const int64_t i = base + 1024 * b + 4 * t;
        if (i + 3 < n)
        {
            const uint4 q = *(const uint4 *)(keys + i);
            atomicAdd(&bins[(q.x >> shift) & mask], 1u);
            atomicAdd(&bins[(q.y >> shift) & mask], 1u);
            atomicAdd(&bins[(q.z >> shift) & mask], 1u);
            atomicAdd(&bins[(q.w >> shift) & mask], 1u);
        }
        else
            for (int k = 0; k < 4; k++)
                if (i + k < n) atomicAdd(&bins[(keys[i + k] >> shift) & mask], 1u);
    }
    __syncthreads();
    const uint32_t c = bins[t];
    r.table[(size_t)chunk * NB + t] = c;
    if (c) __hip_atomic_fetch_add(acc + (size_t)(chunk >> 6) * NB + t, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Block 0 of the depth order's first ticket-free scatter (depth_order.hip: rs_hist_census_direct_kernel left the words): the chunks' census words -> N, top_const, the pinned host word (see above).
__device__ __forceinline__ void publish_census(const DepthCensus &census, int chunks, int t)
{
    __shared__ unsigned long long psum[4];
    __shared__ uint32_t por[4], pand[4];
    KeyCensus all;
    for (int c = t; c < chunks; c += 256) all.combine(census.chunk_sum[c], census.chunk_or[c], census.chunk_and[c]);
    all.wave_fold();
    all.park(psum, por, pand);
    __syncthreads();
    if (t == 0)
    {
        all = KeyCensus::gather<4>(psum, por, pand);
        publish_instance_count(all.tiles, census.n_out, census.top_const, all.top_byte_constant(census.force_varying), census.host_out);
    }
}

// One workgroup = one chunk of CH pairs; wave w owns the w-th quarter (KB steps of 64 consecutive pairs, held in registers).
//   1. wave-local stable ranks, step by step (wave_match_rank);
//   2. thread d turns the four waves' counts of digit d into the chunk-local start of every (wave, digit) run (digit_run_starts) and the
//      distance from the chunk-local order to the digit's global run;
//   3. every pair is parked in LDS at its chunk-local sorted position, and the chunk leaves in that order: consecutive threads
//      write consecutive addresses inside each digit's run (scattering straight from registers costs a 32-64 B fabric write
//      per 4-byte store on this chip: measured 2x slower than rocPRIM; staged, the stores are coalesced runs).
// DIRECT: the pass's histogram was rs_hist_direct_kernel; `acc` holds the slabs' digit totals and the table rows are raw counts.
// `acc_clear` (either flavour): the other totals buffer, cleared here for the next pass's histogram (nobody reads it any more).
// TWO_PHASE (the 4096-pair chunks of the instance sort): keys and values pass through ONE staging array one after the other, and the values
// are only loaded once the keys have been ranked.  Half the LDS and 16 registers less at the peak put seven workgroups on a CU instead of
// four: the 1126 chunks of the headline's instance list are then resident in one round (4 x 256 slots had left 102 of them for a second).
template <bool IDENTITY_VALUES, int CH, bool DIRECT, bool CENSUS, bool TWO_PHASE>
__device__ __forceinline__ void rs_scatter_body(const uint32_t *__restrict__ kin, const uint32_t *__restrict__ vin, uint32_t *__restrict__ kout,
                                                uint32_t *__restrict__ vout, int64_t n, const unsigned long long *n_dev, int shift, int nbits,
                                                RadixScratchView r, const uint32_t *skip_flag, const uint32_t *__restrict__ acc,
                                                uint32_t *__restrict__ acc_clear, const DepthCensus &census)
{
    constexpr int KB = CH / 256; // steps per wave
    if (!resolve_count<CH>(n_dev, n, r)) return;
    if (pass_skipped(skip_flag)) return;
    if (acc_clear && (int)blockIdx.x < r.slabs) acc_clear[(size_t)blockIdx.x * NB + threadIdx.x] = 0u;
    constexpr int SK = (!TWO_PHASE && CH < 8 * NB) ? 8 * NB : CH; // the DIRECT prefix exchange borrows 8 (TWO_PHASE: 12) x 256 words of stage_k
    constexpr int SV = TWO_PHASE ? 4 : (CH < 4 * NB ? 4 * NB : CH); // ... and 4 x 256 words of stage_v (TWO_PHASE: all 12 x 256 of stage_k)
    __shared__ __attribute__((aligned(16))) uint32_t stage_k[SK], stage_v[SV];
    static_assert(!TWO_PHASE || CH >= 12 * NB, "TWO_PHASE borrows 12 x 256 words of stage_k");
    static_assert(!TWO_PHASE || (!IDENTITY_VALUES && !CENSUS), "TWO_PHASE is the instance sort's flavour");
    uint32_t *const xtotal = TWO_PHASE ? stage_k + 8 * NB : stage_v; // where the four waves' partial digit totals meet
    __shared__ uint32_t wcnt[4][NB]; // per-wave digit counts, then the chunk-local start of the (wave, digit) run
    __shared__ int32_t gdelta[NB];   // global run start of the digit minus its chunk-local start
    __shared__ uint32_t wtot[4], gtot[4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int chunk = rs_chunk_of_block(r.chunks);
    if (chunk < 0) return;
    const uint32_t mask = (1u << nbits) - 1u;
    const int64_t base = (int64_t)chunk * CH + (int64_t)wave * (CH / 4);
    const int64_t here = n - base;                                        // pairs from this wave's first one to the end of the array
    const int mine = here >= CH / 4 ? CH / 4 : (here > 0 ? (int)here : 0); // ... of which this wave holds the first `mine`
    const uint32_t *kin_w = kin + base, *vin_w = IDENTITY_VALUES ? nullptr : vin + base;
    uint32_t key[KB], val[KB], rk[KB];
#pragma unroll
    for (int b = 0; b < KB; b++)
    {
        const int i = 64 * b + lane;
        key[b] = 0xFFFFFFFFu;
        val[b] = 0u;
        if (i < mine)
        {
            key[b] = kin_w[i];
            if (!TWO_PHASE) val[b] = IDENTITY_VALUES ? (uint32_t)(base + i) : vin_w[i];
        }
    }
    // DIRECT: the loads of the prefixes are requested here, behind the keys; the four waves' partial sums meet in LDS after the ranking (the
    // staging arrays are still free then)
    DirectPrefix prefix;
    if (DIRECT) prefix.load(r, acc, chunk, wave, lane);
#pragma unroll
    for (int k = 0; k < NB / 64; k++) wcnt[wave][lane + 64 * k] = 0u;
    wave_lds_order();
    uint32_t *cnt = wcnt[wave];
#pragma unroll
    for (int b = 0; b < KB; b++) rk[b] = wave_match_rank((key[b] >> shift) & mask, 64 * b + lane < mine, cnt);
    if (DIRECT) prefix.park(stage_k, xtotal, wave, lane);
    __syncthreads();
    {
        // thread t = digit t
        uint32_t d_earlier = 0u, d_total = 0u, tot;
        if (DIRECT) DirectPrefix::fold(stage_k, xtotal, t, d_earlier, d_total);
        const uint32_t dbase = digit_run_starts<4>(wcnt, wtot, wave, lane, tot);
        // global run start of the digit: the exclusive prefix of the digit totals over the digits + what earlier chunks hold of it
        const uint32_t g = DIRECT ? digit_exclusive_prefix<4>(d_total, gtot, wave, lane) + d_earlier
                                  : r.binbase[t] + r.slabtot[(size_t)(chunk >> 6) * NB + t] + r.table[(size_t)chunk * NB + t];
        gdelta[t] = (int32_t)(g - dbase);
    }
    __syncthreads();
    const int64_t left = n - (int64_t)chunk * CH;
    const int count = left < CH ? (int)left : CH;
    if (TWO_PHASE)
    {
#pragma unroll
        for (int b = 0; b < KB; b++)
            if (64 * b + lane < mine)
            {
                rk[b] += wcnt[wave][(key[b] >> shift) & mask]; // chunk-local sorted position, kept for the values
                stage_k[rk[b]] = key[b];
            }
#pragma unroll
        for (int b = 0; b < KB; b++) // the keys' registers are free now; the values arrive while the keys leave
        {
            const int i = 64 * b + lane;
            if (i < mine) val[b] = vin_w[i];
        }
        __syncthreads();
        uint32_t dpack[KB / 4 > 0 ? KB / 4 : 1]; // the digits of the KB positions this thread writes out, for the values' turn
#pragma unroll
        for (int j = 0; j < KB; j++)
        {
            const int p = t + 256 * j;
            if ((j & 3) == 0) dpack[j >> 2] = 0u;
            if (p < count)
            {
                const uint32_t k = stage_k[p], d = (k >> shift) & mask;
                dpack[j >> 2] |= d << (8 * (j & 3));
                kout[(int64_t)gdelta[d] + p] = k;
            }
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < KB; b++)
            if (64 * b + lane < mine) stage_k[rk[b]] = val[b];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KB; j++)
        {
            const int p = t + 256 * j;
            if (p < count) vout[(int64_t)gdelta[(dpack[j >> 2] >> (8 * (j & 3))) & 0xFFu] + p] = stage_k[p];
        }
        return;
    }
#pragma unroll
    for (int b = 0; b < KB; b++)
        if (64 * b + lane < mine)
        {
            const uint32_t p = wcnt[wave][(key[b] >> shift) & mask] + rk[b];
            stage_k[p] = key[b];
            stage_v[p] = val[b];
        }
    __syncthreads();
    for (int p = t; p < count; p += 256)
    {
        const uint32_t k = stage_k[p];
        const int64_t dst = (int64_t)gdelta[(k >> shift) & mask] + p;
        kout[dst] = k;
        vout[dst] = stage_v[p];
    }
    if (CENSUS && chunk == 0) publish_census(census, r.chunks, t);
}
template <bool IDENTITY_VALUES, int CH, bool DIRECT, bool CENSUS = false>
__global__ void __launch_bounds__(256) rs_scatter_kernel(const uint32_t *__restrict__ kin, const uint32_t *__restrict__ vin,
                                                          uint32_t *__restrict__ kout, uint32_t *__restrict__ vout, int64_t n,
                                                          const unsigned long long *n_dev, int shift, int nbits, RadixScratchView r, const uint32_t *skip_flag,
                                                          const uint32_t *__restrict__ acc, uint32_t *__restrict__ acc_clear, DepthCensus census = DepthCensus{})
{
    rs_scatter_body<IDENTITY_VALUES, CH, DIRECT, CENSUS, false>(kin, vin, kout, vout, n, n_dev, shift, nbits, r, skip_flag, acc, acc_clear, census);
}

// The chunk length is a run-time property of the sort's scratch (ts2d_common.h: 1024 / 2048 / 4096 pairs); every launcher instantiates its kernel
// for the three of them.  Inside the braces CH is the compile-time length.
#define TS_WITH_CHUNK(chunk, ...)                                    \
    switch (chunk)                                                   \
    {                                                                \
    case TS_RS_CHUNK_SMALL: { constexpr int CH = TS_RS_CHUNK_SMALL; __VA_ARGS__; } break; \
    case TS_RS_CHUNK_MID: { constexpr int CH = TS_RS_CHUNK_MID; __VA_ARGS__; } break;     \
    default: { constexpr int CH = TS_RS_CHUNK; __VA_ARGS__; } break; \
    }
} // namespace

// ---- radix_sort.hip: the host passes, for depth_order.hip ------------------------------------------------------------------------------------------
// One pass = histogram + scatter (ts_radix_pass: the hierarchical flavour, ts_radix_pass_direct: the ticket-free one, adding into r.slabacc[which]).
// The census flavours of the depth order's first pass are launched by depth_order.hip itself.
void ts_radix_hist(const uint32_t *kin, int64_t n, const unsigned long long *n_dev, int shift, int nbits, const RadixScratchView &r, hipStream_t s,
                   const uint32_t *skip_flag = nullptr);
void ts_radix_scatter(const uint32_t *kin, const uint32_t *vin, uint32_t *kout, uint32_t *vout, int64_t n, const unsigned long long *n_dev, int shift,
                      int nbits, const RadixScratchView &r, hipStream_t s, const uint32_t *skip_flag = nullptr, const uint32_t *acc = nullptr,
                      uint32_t *acc_clear = nullptr);
void ts_radix_pass(const uint32_t *kin, const uint32_t *vin, uint32_t *kout, uint32_t *vout, int64_t n, const unsigned long long *n_dev, int shift,
                   int nbits, const RadixScratchView &r, hipStream_t s, const uint32_t *skip_flag = nullptr);
void ts_radix_pass_direct(const uint32_t *kin, const uint32_t *vin, uint32_t *kout, uint32_t *vout, int64_t n, const unsigned long long *n_dev, int shift,
                          int nbits, const RadixScratchView &r, int which, hipStream_t s, const uint32_t *skip_flag = nullptr);
bool ts_radix_direct_ok(const RadixScratchView &r); // the sort takes the ticket-free passes: at most TS_DIRECT_MAX_SLABS slabs and no forced tickets
bool ts_radix_tickets_forced();                     // lab library only: ts2d_lab_force_ticket_passes is on
// ---- depth_order.hip, for emit.hip -------------------------------------------------------------------------------------------------------------------
bool ts_scan_two_level(int32_t P); // step 2 left the sums of every 64 block sums in g.supersum as well
