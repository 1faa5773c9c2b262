// ts2d_group.h -- everything the lane-group blend kernels of the two variants share (render_group.hip: 2D, render3d_group.hip: 3D): wave64
// ballots / ranks, dense batches, the 16-lane DPP-row transpose-reduce networks, the tile's contribution statistics, and the lane-group
// SKELETON of the four kernels (second half of the file).  A variant's file holds its table row layout, its cull, its per-pixel geometry and
// hit test, its gradient terms and its flush; nothing here asks which variant is running -- where the two differ, the difference is an
// argument (the row stride, where the sums or the list position sit inside a row, TCAP, the gather's filler record).
//
// Why this structure (measured on MI355X, profiles/r02_notes.md):
//   * a blended (triangle, 8x8 quadrant) pair touches 18 of the 64 pixels on average, so one triangle per wave
//     iteration leaves 72 % of the lanes idle, and gfx950 does not skip an all-idle 32-lane pass;
//   * on gfx950 only fma/add/mul (f32) and add/and (u32) issue at the full 32-lanes-per-clock rate; v_cmp, v_cndmask,
//     v_min/max, every DPP form and the integer shift/mad forms are half rate, transcendentals and v_permlane*_swap
//     quarter rate -- the blend loops are bound by exactly those, not by FMAs.
// So: one wave64 still owns one 8x8 pixel quadrant of a 16x16 tile, but its lanes form FOUR 16-lane groups, one per 4x4
// pixel block, and every group walks ITS OWN culled list of the batch's triangles: four different triangles are blended
// per wave step (lane occupancy 28 % -> ~45 %), the per-step body is branch-free, and all cross-lane reductions stay
// inside a 16-lane DPP row (no v_permlane*_swap).
//
//   batch   = up to 64 list entries, one per lane: the lane gathers the 64-byte render record, computes the conservative
//             support of the triangle (the variant's cull, used for CULLING only) against the four 4x4 blocks, and the wave
//             ballots one 64-bit mask per block;
//   lists   = each block's surviving entries, compacted in visiting order into a 64-byte LDS list (v_mbcnt rank);
//   step    = every lane reads ITS group's next entry, then that entry's constants from the wave-private LDS
//             table (4 distinct rows per ds_read_b128 cost the same as one broadcast row, tools/valu_bench2.hip); a group
//             whose list is exhausted reads the dummy row -1, which no pixel can hit.
#pragma once
#include "ts2d_common.h"
#include "ts2d_wave.h"

namespace
{
constexpr int NR = 32;  // table rows per pass: the entries of a 64-entry batch that have work, compacted (more than NR: two passes)
typedef unsigned short __attribute__((may_alias)) u16a;
constexpr int ROW = 20; // floats per entry row of the wave-private constants table (row -1 = a dummy no pixel can hit)

__device__ __forceinline__ unsigned long long ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ int lane_rank(unsigned long long m) // set bits of m below this lane
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// 0 <= ecc <= 10 (forward.cu:307) as ONE unsigned compare: negative floats and NaN have larger bit patterns than 10.0f
__device__ __forceinline__ bool ecc_in_range(float ecc) { return __float_as_uint(ecc) <= 0x41200000u; }

// ---- dense batches -------------------------------------------------------------------------------------------------------
// The emission kernel marks in the top four bits of an instance's value which quadrants of the tile the triangle can reach (ts2d_support.h).
// A quadrant wave reads the tile's list 64 candidates at a time and keeps the entries whose bit is set, COMPACTED: lanes [0, n) of (id, pos)
// hold the next n entries in processing order (pos = the entry's position in the tile's list).  One refill = one ballot, one cross-lane
// permutation (ds_permute: taken lanes go to slots n, n + 1, ..., the others fill the rest of the permutation) and no LDS memory; a window
// that does not fit is consumed only up to the last entry that does (the cursor moves by that many candidates).
// DESC = false: candidates cursor, cursor + 1, ... (< end), cursor moves up.  DESC = true: cursor - 1, cursor - 2, ... (>= 0), cursor moves down
// (the backward walks the list back to front; lane 0 is then the entry farthest back).
// CAP = entries per batch (64; 32 = every batch is ONE pass of the 32-row table and no record is gathered twice -- measured in round 5,
// profiles/r05_notes.md: the extra block culls cost what the re-gathers save).
// NIB (the 2D kernels' default front end): the candidate's sorted tile KEY is loaded beside its value; bits [qbit, qbit + 4) of it are the block
// mask of this quadrant (ts2d_support.h: qbit = 16 + 4 * quadrant).  An entry is kept when the nibble is not zero, and the nibble travels with
// the id through the one permutation, in the four bits above it: id = triangle | nibble << TS_ID_BITS.
template <bool DESC, int CAP = 64, bool NIB = false>
__device__ __forceinline__ void stream_refill(uint32_t &id, int &pos, int &n, const uint32_t *__restrict__ list, int &cursor, int end, int qbit, int lane,
                                              const uint32_t *__restrict__ keys = nullptr)
{
    while (n < CAP && (DESC ? cursor > 0 : cursor < end))
    {
        const int k = DESC ? cursor - 1 - lane : cursor + lane;
        const bool valid = DESC ? k >= 0 : k < end;
        uint32_t v = 0u, key = 0u;
        if (valid) // one branch: the two loads are in flight together
        {
            v = list[k];
            if (NIB) key = keys[k];
        }
        const uint32_t nib = NIB ? (key << (TS_ID_BITS - qbit)) & ~TS_ID_MASK : 0u; // already where it travels
        const bool want = NIB ? nib != 0u : valid && ((v >> qbit) & 1u);
        unsigned long long mt = ballot(want);
        int adv = 64;
        const int room = CAP - n;
        bool taken = want;
        if (__popcll(mt) > room) // keep the first `room` of them; the next refill starts behind the last one kept
        {
            taken = want && lane_rank(mt) < room;
            mt = ballot(taken);
            adv = 64 - __builtin_clzll(mt);
        }
        cursor += DESC ? -adv : adv;
        if (mt == 0) continue;
        const int cnt = __popcll(mt), rk = lane_rank(mt);
        const int dest = (taken ? n + rk : n + cnt + (lane - rk)) & 63; // a permutation of the 64 lanes
        const uint32_t pid = (uint32_t)__builtin_amdgcn_ds_permute(dest << 2, (int)((v & TS_ID_MASK) | nib));
        const int ppos = __builtin_amdgcn_ds_permute(dest << 2, k);
        const bool fresh = lane >= n && lane < n + cnt;
        id = fresh ? pid : id;
        pos = fresh ? ppos : pos;
        n += cnt;
    }
}

// ---- 16-lane (DPP row) transpose-reduce: N values per lane -> each lane keeps the row-wide reduction of ONE value ----
// Sum AND maximum of 8 values over the 16 lanes of each DPP row in one pass (the forward's contribution statistics): an 8-value
// transpose-reduce (level 1 pairs lanes l, l ^ 8 via row_ror:8, level 2 lanes inside a group of 8 via row_half_mirror, level 3 l, l ^ 2, then
// l, l ^ 1) with the write masks of row_reduce16 -- levels 1 and 2 pair lanes of different DPP banks, so "which half keeps which value" is the
// instruction's own bank mask (two v_add/v_max_f32_dpp per pair instead of two v_cndmask + one; every one of them half rate on gfx950): 32
// instructions for both results against 44 with v_cndmask selects.  The two chains are interleaved so that no DPP operand is read within two wait states of its
// write; level 1 writes fresh registers (the inputs stay intact for the caller).  Lanes l and l ^ 1 end up with step (b3 + 2 b2 + 4 b1).
__device__ __forceinline__ void row_reduce8_sum_max(const float (&c)[8], unsigned long long mask_b1, float &sum, float &mx)
{
    float s0, s1, s2, s3, m0, m1, m2, m3;
#define TSG8_L1(OP, T, X, Y)                                                              \
    OP " " T ", " Y ", " Y " row_ror:8 row_mask:0xf bank_mask:0xc\n"                      \
    OP " " T ", " X ", " X " row_ror:8 row_mask:0xf bank_mask:0x3\n"
#define TSG8_L2(OP, X, Y)                                                                 \
    OP " " Y ", " Y ", " Y " row_half_mirror row_mask:0xf bank_mask:0xa\n"                \
    OP " " Y ", " X ", " X " row_half_mirror row_mask:0xf bank_mask:0x5\n"
#define TSG8_QP(OP, X, QP) OP " " X ", " X ", " X " quad_perm:" QP " row_mask:0xf bank_mask:0xf\n"
    asm volatile("s_nop 1\n"
                 TSG8_L1("v_add_f32_dpp", "%0", "%8", "%9") TSG8_L1("v_add_f32_dpp", "%1", "%10", "%11")
                 TSG8_L1("v_add_f32_dpp", "%2", "%12", "%13") TSG8_L1("v_add_f32_dpp", "%3", "%14", "%15")
                 TSG8_L1("v_max_f32_dpp", "%4", "%8", "%9") TSG8_L1("v_max_f32_dpp", "%5", "%10", "%11")
                 TSG8_L1("v_max_f32_dpp", "%6", "%12", "%13") TSG8_L1("v_max_f32_dpp", "%7", "%14", "%15")
                 TSG8_L2("v_add_f32_dpp", "%0", "%1") TSG8_L2("v_max_f32_dpp", "%4", "%5")
                 TSG8_L2("v_add_f32_dpp", "%2", "%3") TSG8_L2("v_max_f32_dpp", "%6", "%7")
                 TSG8_QP("v_add_f32_dpp", "%1", "[2,3,0,1]") TSG8_QP("v_max_f32_dpp", "%5", "[2,3,0,1]")
                 TSG8_QP("v_add_f32_dpp", "%3", "[2,3,0,1]") TSG8_QP("v_max_f32_dpp", "%7", "[2,3,0,1]")
                 "v_cndmask_b32_e64 %3, %1, %3, %16\n"
                 "v_cndmask_b32_e64 %7, %5, %7, %16\n"
                 "s_nop 0\n"
                 TSG8_QP("v_add_f32_dpp", "%3", "[1,0,3,2]") TSG8_QP("v_max_f32_dpp", "%7", "[1,0,3,2]")
                 "s_nop 1\n"
                 : "=&v"(s0), "=&v"(s1), "=&v"(s2), "=&v"(s3), "=&v"(m0), "=&v"(m1), "=&v"(m2), "=&v"(m3)
                 : "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]), "v"(c[6]), "v"(c[7]), "s"(mask_b1));
#undef TSG8_L1
#undef TSG8_L2
#undef TSG8_QP
    sum = s3;
    mx = m3;
}

// 16 values: the row-wide sum of the value fed at position (b3 + 2 b2 + 4 b1 + 8 b0) lands in the lane -- callers feed
// gradient-record column c at position bitrev4(c), so that lane (l & 15) of a group ends up with column (l & 15).
// Levels 1 and 2 pair lanes of different DPP banks (l ^ 8 via row_ror:8, then the two banks of each 8 via row_half_mirror), so
// the "which half keeps which value" select is the instruction's own bank write mask: two v_add_f32_dpp per pair instead of
// two v_cndmask + one (all half rate on gfx950).  Levels 3 and 4 pair lanes inside a quad and need one v_cndmask each.
// Written as ONE asm statement because hipcc's DPP combiner does not form partially masked adds; wait states (a VALU
// result needs 2 states before a DPP op reads it) are satisfied by the instruction order plus the three s_nop.
__device__ __forceinline__ float row_reduce16(float (&v)[16], unsigned long long mask_b1, unsigned long long mask_b0)
{
#define TSG_L1(X, Y)                                                                    \
    "v_add_f32_dpp " Y ", " Y ", " Y " row_ror:8 row_mask:0xf bank_mask:0xc\n"         \
    "v_add_f32_dpp " Y ", " X ", " X " row_ror:8 row_mask:0xf bank_mask:0x3\n"
#define TSG_L2(X, Y)                                                                    \
    "v_add_f32_dpp " Y ", " Y ", " Y " row_half_mirror row_mask:0xf bank_mask:0xa\n"   \
    "v_add_f32_dpp " Y ", " X ", " X " row_half_mirror row_mask:0xf bank_mask:0x5\n"
#define TSG_L3(X, Y, QP, M)                                                             \
    "v_add_f32_dpp " X ", " X ", " X " quad_perm:" QP " row_mask:0xf bank_mask:0xf\n"  \
    "v_add_f32_dpp " Y ", " Y ", " Y " quad_perm:" QP " row_mask:0xf bank_mask:0xf\n"  \
    "v_cndmask_b32_e64 " Y ", " X ", " Y ", " M "\n"
    asm volatile("s_nop 1\n"
                 TSG_L1("%0", "%1") TSG_L1("%2", "%3") TSG_L1("%4", "%5") TSG_L1("%6", "%7")
                 TSG_L1("%8", "%9") TSG_L1("%10", "%11") TSG_L1("%12", "%13") TSG_L1("%14", "%15")
                 TSG_L2("%1", "%3") TSG_L2("%5", "%7") TSG_L2("%9", "%11") TSG_L2("%13", "%15")
                 TSG_L3("%3", "%7", "[2,3,0,1]", "%16") TSG_L3("%11", "%15", "[2,3,0,1]", "%16")
                 "v_add_f32_dpp %7, %7, %7 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
                 "s_nop 0\n"
                 "v_add_f32_dpp %15, %15, %15 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
                 "v_cndmask_b32_e64 %15, %7, %15, %17\n"
                 "s_nop 1\n"
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]),
                   "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15])
                 : "s"(mask_b1), "s"(mask_b0));
#undef TSG_L1
#undef TSG_L2
#undef TSG_L3
    return v[15];
}
// The same network when six of the sixteen columns are products  k_c(pixel) * x(pixel, entry)  of a per-pixel constant and ONE common
// per-step factor (the backward's dL/drgb and dL/dnormal: k = dL_dpixel, x = contrib).  A pair (X, Y) of such columns needs one level-1
// instruction instead of two if the two registers are filled "pre-swapped": v[X] = kA x with kA = column X's constant on lanes 0-7 of
// the row and column Y's on lanes 8-15, v[Y] = kB x with the two exchanged -- then  Y = ror8(v[Y]) + v[X]  is already the level-1 result.
// A quad of such columns (two pairs meeting at level 2) continues the idea with constants that depend on the lane's quarter and saves
// the level-2 instruction too.  Registers 0-3 = the quad, 4-5 = the pair, 6-15 as in row_reduce16: 26 DPP adds
// instead of 30.  Which lane ends up with which register is unchanged: reg(l) = 8 (l & 1) + 4 ((l >> 1) & 1) + {0, 2, 1, 3}[l >> 2].
__device__ __forceinline__ float row_reduce16c(float (&v)[16], unsigned long long mask_b1, unsigned long long mask_b0)
{
#define TSG_L1(X, Y)                                                                    \
    "v_add_f32_dpp " Y ", " Y ", " Y " row_ror:8 row_mask:0xf bank_mask:0xc\n"         \
    "v_add_f32_dpp " Y ", " X ", " X " row_ror:8 row_mask:0xf bank_mask:0x3\n"
#define TSG_L1C(X, Y) "v_add_f32_dpp " Y ", " Y ", " X " row_ror:8 row_mask:0xf bank_mask:0xf\n"
#define TSG_L2(X, Y)                                                                    \
    "v_add_f32_dpp " Y ", " Y ", " Y " row_half_mirror row_mask:0xf bank_mask:0xa\n"   \
    "v_add_f32_dpp " Y ", " X ", " X " row_half_mirror row_mask:0xf bank_mask:0x5\n"
#define TSG_L3(X, Y, QP, M)                                                             \
    "v_add_f32_dpp " X ", " X ", " X " quad_perm:" QP " row_mask:0xf bank_mask:0xf\n"  \
    "v_add_f32_dpp " Y ", " Y ", " Y " quad_perm:" QP " row_mask:0xf bank_mask:0xf\n"  \
    "v_cndmask_b32_e64 " Y ", " X ", " Y ", " M "\n"
    asm volatile("s_nop 1\n"
                 TSG_L1C("%0", "%1") TSG_L1C("%2", "%3") TSG_L1C("%4", "%5") TSG_L1("%6", "%7")
                 TSG_L1("%8", "%9") TSG_L1("%10", "%11") TSG_L1("%12", "%13") TSG_L1("%14", "%15")
                 "v_add_f32_dpp %3, %3, %1 row_half_mirror row_mask:0xf bank_mask:0xf\n" // level 2 of the quad: one instruction
                 TSG_L2("%5", "%7") TSG_L2("%9", "%11") TSG_L2("%13", "%15")
                 TSG_L3("%3", "%7", "[2,3,0,1]", "%16") TSG_L3("%11", "%15", "[2,3,0,1]", "%16")
                 "v_add_f32_dpp %7, %7, %7 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
                 "s_nop 0\n"
                 "v_add_f32_dpp %15, %15, %15 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
                 "v_cndmask_b32_e64 %15, %7, %15, %17\n"
                 "s_nop 1\n"
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]),
                   "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15])
                 : "s"(mask_b1), "s"(mask_b0));
#undef TSG_L1
#undef TSG_L1C
#undef TSG_L2
#undef TSG_L3
    return v[15];
}
constexpr int bitrev4(int c) { return ((c & 1) << 3) | ((c & 2) << 1) | ((c & 4) >> 1) | ((c & 8) >> 3); }


// ---- contrib_sum / contrib_max of a tile (forward, rich_info) ---------------------------------------------------------------
// The four quadrant waves of a tile and the four lane groups of each wave meet in two LDS arrays indexed by list position.
// LDS atomics on gfx950 (tools/lds_atomic_bench2.hip): ds_add_f32 193 cycles per wave instruction, ds_add_u32 4.9, ds_add_u64 7.0,
// ds_max_i32 4.8 -- so the sums are kept in 16.48 FIXED POINT (a (group, entry) sum is <= 16, a tile's <= 256; the smallest
// possible contribution, 1/255 * 1e-4, still carries 27 significant bits: the fixed-point sum is closer to the exact one than any
// fp32 summation order) and the maxima as the bit patterns of non-negative floats (int order == float order).
__device__ __forceinline__ unsigned long long to_fixed48(float x) // x in [0, 2^15): floor(x * 2^48), exact for x >= 2^-25
{
    const float y = x * 0x1p48f;                          // exact
    const uint32_t hi = (uint32_t)(y * 0x1p-32f);         // truncates
    const float rem = fmaf(-(float)hi, 0x1p32f, y);       // exact: in [0, 2^32)
    return ((unsigned long long)hi << 32) | (unsigned long long)(uint32_t)rem;
}
// Scattered global atomics cost one L2 line operation each (~20 G/s chip-wide, tools/atomic_scope_bench.hip).  A running maximum
// only grows, so a (possibly stale, hence smaller) plain read that already exceeds the new value proves the atomic redundant.
__device__ __forceinline__ void global_stats_add(uint32_t tid, float sm, float mx, float *contrib_sum, float *contrib_max)
{
    unsafeAtomicAdd(contrib_sum + tid, sm);
    if (mx > contrib_max[tid]) atomicMax((int *)contrib_max + tid, __float_as_int(mx));
}
template <int TCAP>
__device__ __forceinline__ void tile_stats_add(unsigned long long *tsum, int *tmax, int k, float sm, float mx, const uint32_t *tile_list,
                                               float *contrib_sum, float *contrib_max)
{
    if (k < TCAP)
    {
        __hip_atomic_fetch_add(tsum + k, to_fixed48(sm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_max(tmax + k, __float_as_int(mx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    else global_stats_add(tile_list[k] & TS_ID_MASK, sm, mx, contrib_sum, contrib_max); // list positions beyond the LDS arrays (a very long tile list); id bits only
}
__device__ __forceinline__ void tile_stats_flush(unsigned long long fx48, int mxbits, uint32_t tid, float *contrib_sum, float *contrib_max)
{
    global_stats_add(tid, (float)((double)fx48 * 0x1p-48), __int_as_float(mxbits), contrib_sum, contrib_max);
}

// ==== the lane-group skeleton ===============================================================================================================
// ---- tile -> quadrant -> 16-lane group -> pixel ------------------------------------------------------------------------------------------
struct GroupPixel
{
    int lane, grp, sub;         // lane of the wave; its 16-lane group = the 4x4 block (by >> 2) * 2 + (bx >> 2) of the quadrant; lane inside the group
    int X0, Y0, lx, ly, px, py; // the quadrant's origin, the pixel inside the quadrant, the pixel
    bool inside;
};
__device__ __forceinline__ GroupPixel group_pixel(const RenderArgs &a, int tile, int quad)
{
    GroupPixel p;
    const int tx = tile % a.grid_x, ty = tile / a.grid_x;
    p.lane = threadIdx.x & 63;
    p.grp = p.lane >> 4; p.sub = p.lane & 15;
    p.X0 = tx * TS_TILE + (quad & 1) * 8; p.Y0 = ty * TS_TILE + (quad >> 1) * 8;
    p.lx = ((p.grp & 1) << 2) + (p.sub & 3); p.ly = ((p.grp >> 1) << 2) + (p.sub >> 2);
    p.px = p.X0 + p.lx; p.py = p.Y0 + p.ly;
    p.inside = p.px < a.W && p.py < a.H;
    return p;
}
// The forward runs the four quadrant waves of a tile as one workgroup (they merge the tile's contribution statistics).  In the backward they
// never talk to each other, so it launches them as single-wave workgroups: the dispatcher then fills a freed wave slot with the next quadrant
// instead of waiting for four slots of one CU, which shortens the tail of the launch (8160 tiles are only 5.3 rounds of 256-thread
// workgroups).  Four consecutive units of an XCD are the four quadrants of one tile: they stay neighbours in dispatch order and on one XCD
// (shared L2 for the tile's list and records).
static inline int ts_quadrant_units(int grid_x, int grid_y) { return 4 * ts_tile_units(grid_x, grid_y); } // padded: units past the image return at once
__device__ __forceinline__ int tile_of_quadrant_block(int b, int grid_x, int grid_y, int &quad)
{
    const int x = b & 7, j = b >> 3;
    quad = j & 3;
    return tile_of_block(((j >> 2) << 3) | x, grid_x, grid_y);
}

// ---- one batch: gather, block masks, compaction into table rows, the four lists ---------------------------------------------------------------
// A workgroup's table = (NR + 1) rows of `stride` floats per wave, the first of them the wave's dummy row.  A list entry is the LDS BYTE
// OFFSET of its row (u16): the step loops spend no instruction on unpacking or scaling an index (round 3: four half-rate instructions per
// step gone; gfx950 issues shifts, bit-field extracts and 24-bit multiply-adds at half rate, tools/valu_bench3.hip).
// Row r of `wave` is at table_row0(wave, stride) + r * (stride * 4), its dummy row one row before.
__device__ __forceinline__ uint32_t table_row0(int wave, int stride) { return (uint32_t)(wave * (NR + 1) + 1) * (stride * 4); }

// The lane's render record; a lane past the end of the batch keeps the caller's filler, a record the variant's cull can take.
template <bool R3>
__device__ __forceinline__ void gather_record(const float4 *__restrict__ rec, uint32_t id, bool valid, float4 &r0, float4 &r1, float4 &r2, float4 &r3)
{
    if (valid)
    {
        const float4 *rp = rec + 4 * (size_t)id;
        r0 = rp[0]; r1 = rp[1]; r2 = rp[2];
        if (R3) r3 = rp[3];
    }
}
// One entry mask per block, returns their union.  Forward: a block whose 16 pixels are all saturated takes no more entries.
__device__ __forceinline__ unsigned long long fwd_block_masks(unsigned long long (&M)[4], unsigned long long alive, bool valid, const bool (&ov)[4])
{
#pragma unroll
    for (int g = 0; g < 4; g++) M[g] = ((alive >> (16 * g)) & 0xFFFFull) ? ballot(valid && ov[g]) : 0ull;
    return M[0] | M[1] | M[2] | M[3];
}
// Backward: entries at or behind glast[g] are skipped by all of block g's pixels.
// (Plain pointers on purpose: with array references the compiler evaluates the three conditions without the short circuit, and the 3D
// backward measured 1 % slower, profiles/blend_skeleton_ab.txt.)
__device__ __forceinline__ unsigned long long bwd_block_masks(unsigned long long *M, bool valid, const bool *ov, int pos, const int *glast)
{
#pragma unroll
    for (int g = 0; g < 4; g++) M[g] = ballot(valid && ov[g] && pos < glast[g]);
    return M[0] | M[1] | M[2] | M[3];
}
// The entries with work are COMPACTED into at most NR table rows per pass (a batch with more survivors takes two passes: the lanes with
// rank < NR publish their rows first, the others in the second pass): half the LDS of a row per list entry, hence 7 instead of 5 resident
// waves per SIMD -- the blend kernels are latency bound (3 instead of 5 waves: +27 %, profiles/r02_notes.md).  The second pass gathers its
// records again: keeping the first gather's registers alive across the first pass would cost the occupancy the compaction buys (handing the
// surplus to the next batch instead was measured and dropped, a loss: profiles/r06_blend_ab.txt).
struct Compaction
{
    unsigned long long any;
    bool anybit;      // this lane's entry has work
    int rank, nact, r; // its rank among those, their number, its table row
};
__device__ __forceinline__ Compaction compact_rows(unsigned long long any, int lane)
{
    Compaction k;
    k.any = any;
    k.anybit = (any >> lane) & 1;
    k.rank = lane_rank(any); k.nact = __popcll(any);
    k.r = k.rank & (NR - 1);
    return k;
}
__device__ __forceinline__ bool in_pass(const Compaction &k, bool second) { return k.anybit && (second ? k.rank >= NR : k.rank < NR); }
__device__ __forceinline__ unsigned long long pass_mask(const Compaction &k, bool mine) { return k.nact <= NR ? k.any : ballot(mine); }
// The four per-group lists of this pass (mm = pass_mask), each in visiting order and padded with the dummy row; returns the number of steps.
// The form is pinned by the kernels' register budgets (profiles/blend_skeleton_resources.txt): the row offset is formed inside the lane's
// branch, and a block's entries are counted before it -- counted after it, the 2D backward spills two more registers.
__device__ __forceinline__ int build_lists(uint32_t *list, const unsigned long long (&M)[4], unsigned long long mm, uint32_t row0, int r, int stride,
                                           uint32_t dummy, int lane)
{
    list[lane] = dummy | (dummy << 16); // four lists x NR entries: the dummy row
    int steps = 0;
#pragma unroll
    for (int g = 0; g < 4; g++)
    {
        const unsigned long long Mh = M[g] & mm;
        const int n = __popcll(Mh);
        if ((Mh >> lane) & 1) ((u16a *)list)[g * NR + lane_rank(Mh)] = (unsigned short)(row0 + r * (stride * 4));
        steps = max(steps, n);
    }
    return steps;
}
// Steps at which two groups work on the SAME entry (the backward must then add their sums to its row one after the other): bit t = step t.
__device__ __forceinline__ unsigned long long list_conflicts(const uint32_t *list, uint32_t dummy, int lane)
{
    const u16a *l16 = (const u16a *)list + (lane & (NR - 1));
    const uint32_t l0 = l16[0], l1 = l16[NR], l2 = l16[2 * NR], l3 = l16[3 * NR];
    return ballot(lane < NR && ((l0 != dummy && (l0 == l1 || l0 == l2 || l0 == l3)) || (l1 != dummy && (l1 == l2 || l1 == l3)) || (l2 != dummy && l2 == l3)));
}

// ---- forward: the pixel's front-to-back state, the 8-step window, the epilogue -----------------------------------------------------------------
struct FwdPixel
{
    float T, ar, ag, ab, anx, any_, anz, ad;
    bool done;
    uint32_t last;
};
__device__ __forceinline__ FwdPixel fwd_pixel(bool inside, int len)
{
    return {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, !inside, (uint32_t)len}; // a pixel that never saturates examines the whole list (forward.cu:296-297)
}
// One step of one pixel (forward.cu:318-340), returns its contribution.  Branch-free: a lane that does not hit runs with alpha = 0
// (x + c*0 == x, T*1 == T bit for bit).  jpos = the entry's position in the tile's list.
template <bool RICH>
__device__ __forceinline__ float fwd_blend(FwdPixel &P, bool hit, float alpha, float r, float g, float b, float nx, float ny, float nz, float d, int jpos)
{
    const float al = hit ? alpha : 0.0f;
    const float contrib = al * P.T;
    P.ar = fmaf(r, contrib, P.ar);
    P.ag = fmaf(g, contrib, P.ag);
    P.ab = fmaf(b, contrib, P.ab);
    if (RICH)
    {
        P.anx = fmaf(nx, contrib, P.anx);
        P.any_ = fmaf(ny, contrib, P.any_);
        P.anz = fmaf(nz, contrib, P.anz);
        P.ad = fmaf(d, contrib, P.ad);
    }
    P.T *= (1.0f - al);
    const bool sat = hit && P.T <= 0.0001f; // forward.cu:333
    P.last = sat ? (uint32_t)(jpos + 1) : P.last;
    P.done = P.done || sat;
    return contrib;
}
// Step st of a window: the row of the group's entry, from the window's eight packed list entries (uint4 read at mylist + t0).
__device__ __forceinline__ const float *window_row(const char *lds0, const uint4 &packed, int st)
{
    const uint32_t word = st < 2 ? packed.x : (st < 4 ? packed.y : (st < 6 ? packed.z : packed.w));
    return (const float *)(lds0 + ((st & 1) ? (word >> 16) : (word & 0xFFFFu)));
}
// contrib_sum / contrib_max (forward.cu:323-324; the reference issues two global atomics per (pixel, triangle)): the window's 8 x 64
// contributions are reduced inside each 16-lane group, lane pairs (l, l ^ 1) end up with (sum, max) of step `b3 + 2 b2 + 4 b1` of their
// group, and the even lanes add them to the TILE's statistics in LDS with INTEGER atomics (ds_add_u64 / ds_max_i32 cost 5-7 cycles per
// wave instruction, ds_add_f32 193) -- no ordering between groups or waves is needed.  The list position of "its" step comes from float
// `slot` of the step's row (two LDS reads on the few lanes that have something to add) rather than carried through the window in eight
// registers and selected with seven v_cndmask.
template <int TCAP>
__device__ __forceinline__ void window_stats(const float (&c)[8], int lane, int stat_step, const char *lds0, const u16a *mylist, int t0, int slot,
                                             unsigned long long *tsum, int *tmax, const uint32_t *tile_list, float *contrib_sum, float *contrib_max)
{
    float sm, mx;
    row_reduce8_sum_max(c, 0xCCCCCCCCCCCCCCCCull, sm, mx);
    int k = 0;
    if ((lane & 1) == 0 && sm > 0.0f) k = __float_as_int(*(const float *)(lds0 + mylist[t0 + stat_step] + slot * 4));
    if ((lane & 1) == 0 && sm > 0.0f) tile_stats_add<TCAP>(tsum, tmax, k, sm, mx, tile_list, contrib_sum, contrib_max);
}
__device__ __forceinline__ int window_stat_step(int lane) // the step of a window whose statistics this lane ends up with
{
    return ((lane >> 3) & 1) | ((lane >> 1) & 2) | ((lane << 1) & 4);
}
// contrib_sum / contrib_max of the tile's first TCAP list entries are merged over the four quadrant waves in LDS before they leave as global
// atomics (one L2 line operation per (tile, triangle) instead of one per (quadrant, triangle)).
template <int TCAP>
__device__ __forceinline__ void tile_stats_clear(unsigned long long *tsum, int *tmax, int len)
{
    for (int k = threadIdx.x; k < min(len, TCAP); k += 256) { tsum[k] = 0ull; tmax[k] = 0; }
    __syncthreads();
}
// The wave's pixels leave first: their stores, and the ids the statistics' flush needs, are in flight while the wave waits for the others.
template <bool RICH>
__device__ __forceinline__ void fwd_store_pixel(const RenderArgs &a, const GroupPixel &p, const FwdPixel &P,
                                                float *__restrict__ final_T, uint32_t *__restrict__ n_contrib, float *__restrict__ out_feature,
                                                float *__restrict__ out_depth, float *__restrict__ out_normal)
{
    if (p.inside)
    {
        const size_t pix = (size_t)p.py * a.W + p.px, HW = (size_t)a.H * a.W;
        final_T[pix] = P.T;
        n_contrib[pix] = P.last;
        out_feature[pix] = P.ar + P.T * a.background[0]; // forward.cu:345
        if (a.C > 1) out_feature[HW + pix] = P.ag + P.T * a.background[1];
        if (a.C > 2) out_feature[2 * HW + pix] = P.ab + P.T * a.background[2];
        if (RICH)
        {
            out_depth[pix] = P.ad + P.T * (a.background_depth_dev ? *a.background_depth_dev : a.background_depth); // forward.cu:349
            out_normal[pix] = P.anx;
            out_normal[HW + pix] = P.any_;
            out_normal[2 * HW + pix] = P.anz;
        }
    }
}
template <int TCAP>
__device__ __forceinline__ void tile_stats_leave(const unsigned long long *tsum, const int *tmax, int len, const uint32_t *tile_list, float *contrib_sum,
                                                 float *contrib_max)
{
    constexpr int NF = (TCAP + 255) / 256;
    const int nflush = min(len, TCAP);
    uint32_t ids[NF];
#pragma unroll
    for (int j = 0; j < NF; j++)
    {
        const int k = (int)threadIdx.x + 256 * j;
        ids[j] = k < nflush ? tile_list[k] & TS_ID_MASK : 0u;
    }
    __syncthreads(); // the only rendezvous of the four quadrant waves: the tile's merged contribution statistics leave
#pragma unroll
    for (int j = 0; j < NF; j++)
    {
        const int k = (int)threadIdx.x + 256 * j;
        if (k < nflush)
        {
            const unsigned long long fx48 = tsum[k];
            if (fx48 != 0ull) tile_stats_flush(fx48, tmax[k], ids[j], contrib_sum, contrib_max);
        }
    }
}

// ---- backward: the pixel's state, the blocks' last entries, the conflict-aware add ----------------------------------------------------------------
// The reference keeps seven back-to-front composites per pixel (accum_feature[3], accum_normal, accum_depth: backward.cu:323-325) but uses
// them only through dL_dcontrib = sum_c dL_dpix_c * (value_c - accum_c).  With X = sum_c dL_dpix_c * value_c and B = sum_c dL_dpix_c * accum_c
// that is X - B, and the per-channel update accum_c <- alpha value_c + (1 - alpha) accum_c collapses to B <- alpha X + (1 - alpha) B: one
// scalar of sequential state instead of seven (same mathematics, different rounding order).
struct BwdPixel
{
    float T;  // backward.cu:318
    int last; // backward.cu:320
    float dpr, dpg, dpb, dnx, dny, dnz, dd, B;
};
template <bool RICH>
__device__ __forceinline__ BwdPixel bwd_pixel(const RenderArgs &a, const GroupPixel &p, const float *__restrict__ final_T, const uint32_t *__restrict__ n_contrib,
                                              const float *__restrict__ dL_dout_feature, const float *__restrict__ dL_dout_depth,
                                              const float *__restrict__ dL_dout_normal)
{
    const size_t pix = (size_t)p.py * a.W + p.px, HW = (size_t)a.H * a.W;
    BwdPixel P = {p.inside ? final_T[pix] : 0.0f, p.inside ? (int)n_contrib[pix] : 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (p.inside) // backward.cu:331-343
    {
        P.dpr = dL_dout_feature[pix];
        P.B = P.dpr * a.background[0];
        if (a.C > 1) { P.dpg = dL_dout_feature[HW + pix]; P.B = fmaf(P.dpg, a.background[1], P.B); }
        if (a.C > 2) { P.dpb = dL_dout_feature[2 * HW + pix]; P.B = fmaf(P.dpb, a.background[2], P.B); }
        if (RICH)
        {
            P.dnx = dL_dout_normal[pix]; P.dny = dL_dout_normal[HW + pix]; P.dnz = dL_dout_normal[2 * HW + pix];
            P.dd = dL_dout_depth[pix];
            P.B = fmaf(P.dd, a.background_depth_dev ? *a.background_depth_dev : a.background_depth, P.B); // accum_normal starts at 0, accum_depth at background_depth
        }
    }
    return P;
}
// glast[g] = the largest n_contrib of block g: entries at list positions >= it are skipped by all of its pixels (backward.cu:377-379).
// Returns the largest of the four.
__device__ __forceinline__ int block_lasts(int last, int (&glast)[4])
{
    float lm = (float)last;
    lm = fmaxf(lm, dpp<DPP_XOR1>(lm));
    lm = fmaxf(lm, dpp<DPP_XOR2>(lm));
    lm = fmaxf(lm, dpp<DPP_HALF_MIRROR>(lm));
    lm = fmaxf(lm, dpp<DPP_MIRROR>(lm));
#pragma unroll
    for (int g = 0; g < 4; g++) glast[g] = (int)__builtin_amdgcn_readlane((int)lm, 16 * g);
    return max(max(glast[0], glast[1]), max(glast[2], glast[3]));
}
__device__ __forceinline__ void zero_sums(float *sums)
{
    float4 *z = (float4 *)sums;
    z[0] = z[1] = z[2] = z[3] = make_float4(0, 0, 0, 0);
}
// Adds the group's reduced column to its sum in the entry's row.  acc0 = *acc fetched early, only used when no other group adds to this
// row now; shared_row (wave-uniform, a bit of list_conflicts) = one group after the other.
__device__ __forceinline__ void row_add(float *acc, float acc0, float red, bool shared_row, int grp)
{
    if (!shared_row) *acc = acc0 + red;
    else
    {
#pragma unroll
        for (int g = 0; g < 4; g++)
        {
            if (grp == g) *acc += red;
            wave_lds_order();
        }
    }
}
} // namespace

// Launches the <RICH, GAMMA1> instantiation of a blend kernel that the RenderArgs A select.
#define TS_LAUNCH_BLEND(KERNEL, A, GRID, BLOCK, STREAM, ...)                                                                      \
    do                                                                                                                            \
    {                                                                                                                             \
        const bool g1 = ((A).gamma == 1.0f);                                                                                      \
        if ((A).rich_info && g1) hipLaunchKernelGGL((KERNEL<true, true>), dim3(GRID), dim3(BLOCK), 0, STREAM, __VA_ARGS__);       \
        else if ((A).rich_info) hipLaunchKernelGGL((KERNEL<true, false>), dim3(GRID), dim3(BLOCK), 0, STREAM, __VA_ARGS__);       \
        else if (g1) hipLaunchKernelGGL((KERNEL<false, true>), dim3(GRID), dim3(BLOCK), 0, STREAM, __VA_ARGS__);                  \
        else hipLaunchKernelGGL((KERNEL<false, false>), dim3(GRID), dim3(BLOCK), 0, STREAM, __VA_ARGS__);                         \
    } while (0)
