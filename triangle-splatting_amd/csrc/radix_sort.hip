// radix_sort.hip -- the stable LSD radix sort of (key, value) pairs: the host side of its passes (the kernels and the overview are in
// ts2d_radix.h), the instance sort by tile id (step 4 there) and the same sort for other callers (knn.hip, regularizers.hip, mesh_weld.hip,
// mesh_distance.hip).  The only binning unit libts_geom.so links.
#include "ts2d_radix.h"

namespace
{
// the TWO_PHASE flavour with the register budget of five workgroups per CU (1280 resident chunks = 5.2 M pairs)
template <int CH>
__global__ void __launch_bounds__(256, 5) rs_scatter_two_phase_kernel(const uint32_t *__restrict__ kin, const uint32_t *__restrict__ vin,
                                                                       uint32_t *__restrict__ kout, uint32_t *__restrict__ vout, int64_t n,
                                                                       const unsigned long long *n_dev, int shift, int nbits, RadixScratchView r,
                                                                       const uint32_t *skip_flag, const uint32_t *__restrict__ acc, uint32_t *__restrict__ acc_clear)
{
    rs_scatter_body<false, CH, true, false, true>(kin, vin, kout, vout, n, n_dev, shift, nbits, r, skip_flag, acc, acc_clear, DepthCensus{});
}

template <int CH>
void radix_scatter_ch(const uint32_t *kin, const uint32_t *vin, uint32_t *kout, uint32_t *vout, int64_t n, const unsigned long long *n_dev, int shift,
                      int nbits, const RadixScratchView &r, hipStream_t s, const uint32_t *skip_flag, const uint32_t *acc, uint32_t *acc_clear)
{
    const dim3 grid((unsigned)r.chunks);
#define TS_SCATTER(ID, D) hipLaunchKernelGGL((rs_scatter_kernel<ID, CH, D>), grid, dim3(256), 0, s, kin, vin, kout, vout, n, n_dev, shift, nbits, r, skip_flag, acc, acc_clear)
    if (acc && vin)
    {
        if constexpr (CH == TS_RS_CHUNK) // the instance sort of large scenes: keys and values through one staging array (rs_scatter_body)
            hipLaunchKernelGGL((rs_scatter_two_phase_kernel<CH>), grid, dim3(256), 0, s, kin, vin, kout, vout, n, n_dev, shift, nbits, r, skip_flag, acc, acc_clear);
        else TS_SCATTER(false, true);
    }
    else if (acc) TS_SCATTER(true, true);
    else if (vin) TS_SCATTER(false, false);
    else TS_SCATTER(true, false);
#undef TS_SCATTER
}
// g_force_tickets: a lab-library switch (csrc/ts2d_lab.h, ts2d_lab_force_ticket_passes; the symbol is not exported and nothing in the product
// library sets it): every sort takes the hierarchical passes that otherwise only sorts of more than 48 slabs reach (> 6.3 M triangles, > 12.6 M
// instances), so that the suite executes them -- including the ticket-path census that produces num_rendered there.
bool g_force_tickets = false;
__global__ void zero_words_kernel(uint32_t *p, size_t n) // 64-bit count and index: 16 P words at P near 2^28 pass 2^31
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0u;
}
__global__ void __launch_bounds__(256) zero_words4_kernel(uint4 *p, size_t n4)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) p[i] = make_uint4(0u, 0u, 0u, 0u);
}
} // namespace

void ts_radix_hist(const uint32_t *kin, int64_t n, const unsigned long long *n_dev, int shift, int nbits, const RadixScratchView &r, hipStream_t s,
                   const uint32_t *skip_flag)
{
    const dim3 grid((unsigned)r.chunks);
    const uint32_t mask = (1u << nbits) - 1u;
    TS_WITH_CHUNK(r.chunk, hipLaunchKernelGGL((rs_hist_kernel<false, CH>), grid, dim3(256), 0, s, kin, n, n_dev, shift, mask, r, DepthCensus{}, skip_flag))
}
void ts_radix_scatter(const uint32_t *kin, const uint32_t *vin, uint32_t *kout, uint32_t *vout, int64_t n, const unsigned long long *n_dev, int shift,
                      int nbits, const RadixScratchView &r, hipStream_t s, const uint32_t *skip_flag, const uint32_t *acc, uint32_t *acc_clear)
{
    TS_WITH_CHUNK(r.chunk, radix_scatter_ch<CH>(kin, vin, kout, vout, n, n_dev, shift, nbits, r, s, skip_flag, acc, acc_clear))
}
void ts_radix_pass(const uint32_t *kin, const uint32_t *vin, uint32_t *kout, uint32_t *vout, int64_t n, const unsigned long long *n_dev, int shift,
                   int nbits, const RadixScratchView &r, hipStream_t s, const uint32_t *skip_flag)
{
    ts_radix_hist(kin, n, n_dev, shift, nbits, r, s, skip_flag);
    ts_radix_scatter(kin, vin, kout, vout, n, n_dev, shift, nbits, r, s, skip_flag);
}
bool ts_radix_tickets_forced() { return g_force_tickets; }
bool ts_radix_direct_ok(const RadixScratchView &r) { return !g_force_tickets && r.slabs <= TS_DIRECT_MAX_SLABS; }
// The ticket-free pass: the histogram adds into slabacc[which] (cleared by whoever ran before), the scatter reads it and clears the other
// buffer for the pass after this one.  Every block reads the totals of all slabs, so sorts of more than TS_DIRECT_MAX_SLABS slabs (12.6 M
// pairs at 4096 per chunk) keep the hierarchical pass, whose cost does not grow with the slab count.
void ts_radix_pass_direct(const uint32_t *kin, const uint32_t *vin, uint32_t *kout, uint32_t *vout, int64_t n, const unsigned long long *n_dev, int shift,
                          int nbits, const RadixScratchView &r, int which, hipStream_t s, const uint32_t *skip_flag)
{
    const dim3 grid((unsigned)r.chunks);
    const uint32_t mask = (1u << nbits) - 1u;
    TS_WITH_CHUNK(r.chunk, hipLaunchKernelGGL((rs_hist_direct_kernel<CH>), grid, dim3(256), 0, s, kin, n, n_dev, shift, mask, r, r.slabacc[which], skip_flag))
    ts_radix_scatter(kin, vin, kout, vout, n, n_dev, shift, nbits, r, s, skip_flag, r.slabacc[which], r.slabacc[which ^ 1]);
}

// Step 4: stable sort of the instances by tile id: ceil(bits / 8) passes, ping-pong from (k[0], v[0]).
void ts_sort_pairs(const BinningStateView &b, int64_t N, const unsigned long long *n_dev, int ntiles, hipStream_t s)
{
    if (N <= 0) return;
    const int bits = ts_tile_bits(ntiles);
    // the key bits are shared out evenly over the passes (1080p: 13 bits = 7 + 6, not 8 + 5): fewer digits in the first pass mean longer
    // runs per digit in a chunk (32 pairs instead of 16), i.e. better coalesced stores, and one ballot less per ranking step
    const int per = (bits + b.passes - 1) / b.passes;
    int src = 0;
    for (int p = 0; p < b.passes; p++)
    {
        const int shift = per * p, nbits = min(per, bits - shift);
        // ticket-free passes when the sort is small enough; scan_emit_kernel cleared slabacc[0] for the first one
        if (ts_radix_direct_ok(b.rs)) ts_radix_pass_direct(b.k[src], b.v[src], b.k[src ^ 1], b.v[src ^ 1], N, n_dev, shift, nbits, b.rs, p & 1, s);
        else ts_radix_pass(b.k[src], b.v[src], b.k[src ^ 1], b.v[src ^ 1], N, n_dev, shift, nbits, b.rs, s);
        src ^= 1;
    }
}

// ---- the same sort for other callers (knn.hip: 30-bit Morton codes) --------------------------------------------------------
static int generic_chunk(size_t n) { return ts_instance_chunk(n); } // few keys: more, shorter workgroups
size_t ts_radix_scratch_bytes(size_t n)
{
    RadixScratchView r{};
    char *p = nullptr;
    ts_carve_radix(p, n, r, generic_chunk(n));
    return (size_t)p + TS_ALIGN;
}
// Stable LSD sort of (key, value) pairs by key bits [0, end_bit).  k[0] / v[0] hold the input, k[1] / v[1] are the ping-pong partners;
// returns which pair holds the result (passes & 1).
int ts_radix_sort_pairs(uint32_t *const k[2], uint32_t *const v[2], size_t n, int end_bit, void *scratch, hipStream_t s, bool force_tickets)
{
    if (n == 0) return 0;
    RadixScratchView r{};
    char *p = (char *)ts_align_up((size_t)scratch);
    ts_carve_radix(p, n, r, generic_chunk(n));
    hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)((r.slabs + TS_RS_TICKET_EXTRA + 255) / 256)), dim3(256), 0, s, r.tickets, (size_t)(r.slabs + TS_RS_TICKET_EXTRA));
    const bool direct = !force_tickets && ts_radix_direct_ok(r);
    if (direct) hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)r.slabs), dim3(256), 0, s, r.slabacc[0], (size_t)(r.slabs * NB));
    const int passes = (end_bit + 7) / 8;
    int src = 0;
    for (int ps = 0; ps < passes; ps++)
    {
        if (direct) ts_radix_pass_direct(k[src], v[src], k[src ^ 1], v[src ^ 1], (int64_t)n, nullptr, 8 * ps, min(8, end_bit - 8 * ps), r, ps & 1, s);
        else ts_radix_pass(k[src], v[src], k[src ^ 1], v[src ^ 1], (int64_t)n, nullptr, 8 * ps, min(8, end_bit - 8 * ps), r, s);
        src ^= 1;
    }
    return src;
}

void ts_force_ticket_passes(bool on) { g_force_tickets = on; }
void ts_launch_zero_words(uint32_t *p, size_t n, hipStream_t s) // n 32-bit words; 16-byte stores where the range allows
{
    if (n == 0) return;
    if (n % 4 == 0 && ((size_t)p & 15) == 0) hipLaunchKernelGGL(zero_words4_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, (uint4 *)p, n / 4);
    else hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, n);
}
