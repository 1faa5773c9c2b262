// emit.hip -- steps 3 and 5 of the binning (overview: ts2d_radix.h): instance slots + emission in depth order, and the tile ranges of the list
// once radix_sort.hip has grouped it by tile.
#include "ts2d_radix.h"
#include "ts2d_support.h"

namespace
{
// ---- step 3: instance slots + emission ------------------------------------------------------------------------------------------
// One lane per depth-ordered triangle.  Triangles covering up to SMALL tiles are emitted by their own lane; larger ones
// (stress scenes where a triangle spans thousands of tiles) are emitted cooperatively by the whole wave so that a single
// lane never serialises a long loop.  Tiles of one triangle are emitted row-major like the reference's loop
// (rasterizer.cu:63-73); the later sort is by tile id, so only the order BETWEEN triangles matters.
constexpr uint32_t SMALL = 32;

// Round 5, measured on three scenes with the five combinations alternating on one box (profiles/r05_emission_variants.txt; tools/r05_call4.sh):
// a register budget for 6 waves per SIMD (80 registers, 3 spilled; the compiler's own choice is 94 = 5 waves) is worth 0-3 %, and requesting
// the rectangle / record gather EARLY, under the block sums and the scan, cost 10 % and was dropped (1 M triangles: 0.054 -> 0.064 ms; 5 M:
// 0.245 -> 0.277): the gather's 96-128 bytes per lane sit in registers across the scan and the loads queue in front of the block sums.
#ifndef TS_EMIT_WAVES // register budget for N waves per SIMD (0: the compiler's choice)
#define TS_EMIT_WAVES 6
#endif
// BM: the instances' block masks go into the keys' top halves (QuadMaskArgs::blocks) -- an instantiation of its own, so that neither form
// carries the other's registers.
template <bool BM>
#if TS_EMIT_WAVES > 0
__global__ void __launch_bounds__(256, TS_EMIT_WAVES) scan_emit_kernel(
#else
__global__ void __launch_bounds__(256) scan_emit_kernel(
#endif
int P, int grid_x, int ntiles, GeometryStateView g, BinningStateView b, uint2 *ranges,
                                                         float *contrib_sum, float *contrib_max, long long capacity, int32_t *status, bool two_level,
                                                         QuadMaskArgs qmask)
{
    __shared__ uint32_t wtot[4];
    __shared__ unsigned long long wpart[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = blockIdx.x * 256 + t;
    // output clears that used to be three memset launches: tile ranges (rasterizer.cu:223) and the contribution statistics
    for (int k = i; k < ntiles; k += gridDim.x * 256) ranges[k] = make_uint2(0u, 0u);
    if (b.rs.tickets)
    {
        for (int k = i; k < b.rs.slabs + TS_RS_TICKET_EXTRA; k += gridDim.x * 256) b.rs.tickets[k] = 0u; // the tile sort's tickets
        for (int k = i; k < b.rs.slabs * NB; k += gridDim.x * 256) b.rs.slabacc[0][k] = 0u; // ... and its first pass's slab totals
    }
    if (contrib_sum && i < P)
    {
        contrib_sum[i] = 0.0f;
        contrib_max[i] = 0.0f;
    }
    const bool valid = i < P;
    uint32_t tiles = valid ? g.tiles_sorted[i] : 0u;
    const uint32_t id_ahead = valid ? sorted_ids(g)[i] : 0u; // wanted after the scan: requested now, one round trip less behind it
    // Everything in front of this block, requested together and reduced once: the earlier quarters of this scan block (scan blocks are 1024
    // triangles = four of these 256-lane blocks), the raw sums of the scan blocks of its group of 64, the group sums in front of that.
    const int sblock = blockIdx.x >> 2, quarter = blockIdx.x & 3;
    unsigned long long part = 0;
    if (two_level)
    {
        for (int k = t; k < (sblock >> 6); k += 256) part += g.supersum[k];
        if (t < (sblock & 63)) part += g.blocksum[(sblock & ~63) + t];
    }
    else
        for (int k = t; k < sblock; k += 256) part += g.blocksum[k];
    for (int q = 0; q < quarter; q++)
    {
        const int j = (sblock * 4 + q) * 256 + t;
        part += (j < P) ? g.tiles_sorted[j] : 0u;
    }
    if (capacity >= 0) // sync-free forward: the instance count is only known here; over capacity nothing is emitted
    {
        const unsigned long long live = g.blocksum[(P + SB - 1) / SB];
        const bool over = live > (unsigned long long)capacity;
        if (i == 0 && status) *status = over ? 1 : 0;
        if (over) tiles = 0u;
    }
    else if (i == 0 && status) *status = 0; // the host knows the count (the reference's sequence, or the exact re-run after an overflow)
    // inclusive prefix inside the block (wave64 DPP scan + the three preceding waves' totals) on top of what lies in front of the block
    const uint32_t inc = wave_inclusive_scan(tiles, lane);
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 63) wtot[wave] = inc;
    if (lane == 0) wpart[wave] = part;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wave; w++) before += wtot[w];
    const unsigned long long qbase = wpart[0] + wpart[1] + wpart[2] + wpart[3];
    const uint32_t incl = (uint32_t)(qbase + before + inc); // N < 2^31 is checked on the host before anything is emitted
    if (valid) g.offsets[i] = incl;
    const uint32_t id = tiles > 0 ? id_ahead : 0u;
    const uint32_t off = incl - tiles; // exclusive prefix
    uint2 rect = {0u, 0u};
    float4 rec0 = make_float4(0, 0, 0, 0), rec1 = rec0, rec2 = rec0;
    if (tiles > 0)
    {
        rect = g.rect[id];
        const float4 *rp = g.rec + 4 * (size_t)id;
        rec0 = rp[0];
        rec1 = rp[1];
        if (qmask.variant == 3) rec2 = rp[2];
    }
    const uint32_t minx = rect.x & 0xffffu, miny = rect.x >> 16, maxx = rect.y & 0xffffu, maxy = rect.y >> 16;
    uint32_t *tile_out = b.k[0], *val_out = b.v[0];
    // the four spare bits of an instance's value say which 8x8 quadrants of its tile the triangle's support can reach (ts2d_support.h; both
    // variants since round 5, ts2d_common.h: QuadMaskArgs); the blend kernels' quadrant waves then skip the other entries unseen
    constexpr bool qm = true;
    // 2D variant on grids of at most 65 535 tiles: the instance's sixteen 4x4 BLOCK bits go into bits 16..31 of its tile key (the tile sort ranks
    // the low bits only and moves the word whole), the quadrant bits are the OR of their nibbles; the blend kernels then cull nothing themselves
    constexpr bool bm = BM;
    const float quad_g2 = qmask.g2;
    auto setup_from = [&](const float4 &r0, const float4 &r1, const float4 &r2, uint32_t tminx, uint32_t tminy, uint32_t tmaxx, uint32_t tmaxy) {
        if (qmask.variant == 0) return quad_setup_all(); // lab library only: every quadrant (ts2d_lab_force_all_quadrants)
        if (qmask.variant == 3) // the head of the triangle's record and its tile rectangle
        {
            const float E = quad_g2 == 2.0f ? support_scale<true>(1.0f, quad_g2) : support_scale<false>(1.0f, quad_g2);
            return quad_setup_3d(r0, r1, r2, E, qmask.tan_fovx, qmask.tan_fovy, qmask.W, qmask.H, qmask.inv_W, qmask.inv_H, (float)(tminx * TS_TILE) - 1.0f,
                                 (float)(tminy * TS_TILE) - 1.0f, (float)(tmaxx * TS_TILE), (float)(tmaxy * TS_TILE));
        }
        const float E = quad_g2 == 2.0f ? support_scale<true>(r1.z, quad_g2) : support_scale<false>(r1.z, quad_g2);
        return quad_setup<bm ? 3 : 7>(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, E); // block masks: the 4x4 sample box
    };
    auto setup_of = [&](uint32_t tri, uint32_t tminx, uint32_t tminy, uint32_t tmaxx, uint32_t tmaxy) { // another lane's triangle: gathered here
        const float4 *rp = g.rec + 4 * (size_t)tri;
        return setup_from(rp[0], rp[1], qmask.variant == 3 ? rp[2] : make_float4(0, 0, 0, 0), tminx, tminy, tmaxx, tmaxy);
    };
    QuadSetup qs{};
    // The block's instances are one contiguous run of the list.  A lane writing its triangle's few slots straight to memory issues 4-byte
    // stores a few slots apart from its neighbours' (a 32-64 byte fabric write each on this chip); runs of up to STAGE instances are put
    // together in LDS instead and leave as coalesced rows.
    constexpr uint32_t STAGE = 2048;
    // stage_t: a staged instance's tile; region B: its value (plain staging) or -- when the masks are formed -- the 256 triangles' affine mask
    // constants (ts2d_support.h: QuadAffine, 64 bytes each), in which case a staged instance is (dx | dy << 12 | triangle slot << 24)
    __shared__ uint32_t stage_t[STAGE];
    __shared__ __attribute__((aligned(16))) float4 region_b[256 * 4];
    uint32_t *const stage_v = (uint32_t *)region_b;
    const uint32_t run0 = (uint32_t)qbase, run = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    const bool staged = run <= STAGE;
    // Staged runs form their masks in the flush loop below, one lane per INSTANCE, evenly spread over the block (a lane that walks its triangle's
    // tiles makes the whole wave wait for the triangle with the most tiles).  Round 4 gathered the triangle's record and redid the whole setup
    // per instance (~130 VALU instructions + a 32-byte gather each: 0.052 ms against 0.029 without masks at 1 M triangles); round 5 does the
    // setup once per TRIANGLE, leaves its 16 affine constants in LDS, and an instance costs two FMAs per edge + the compares.  Runs too long
    // for the stage (big triangles) test per tile where they write.
    const bool qstage = qm && staged;
    const uint32_t rw = maxx - minx, rh = maxy - miny;
    if (qm && tiles > 0)
    {
        qs = setup_from(rec0, rec1, rec2, minx, miny, maxx, maxy);
        if (qstage)
        {
            const QuadAffine qa = quad_anchor(qs, id, minx, miny, rw, rh);
            region_b[4 * t] = qa.a; region_b[4 * t + 1] = qa.b; region_b[4 * t + 2] = qa.c; region_b[4 * t + 3] = qa.d;
        }
    }
    if (tiles > 0 && tiles <= SMALL)
    {
        uint32_t o = off;
        if (staged)
        {
            o -= run0;
            for (uint32_t y = miny; y < maxy; y++)
                for (uint32_t x = minx; x < maxx; x++)
                {
                    stage_t[o] = qstage ? ((x - minx) | ((y - miny) << 12) | ((uint32_t)t << 24)) : y * grid_x + x;
                    if (!qstage) stage_v[o] = id;
                    o++;
                }
        }
        else
            for (uint32_t y = miny; y < maxy; y++)
                for (uint32_t x = minx; x < maxx; x++)
                {
                    if (bm)
                    {
                        const uint32_t m16 = block_mask(qs, (float)(x * TS_TILE), (float)(y * TS_TILE));
                        tile_out[o] = (y * grid_x + x) | (m16 << 16);
                        val_out[o] = id | (quadrants_of_blocks(m16) << TS_ID_BITS);
                    }
                    else
                    {
                        tile_out[o] = y * grid_x + x;
                        val_out[o] = qm ? id | (quadrant_mask(qs, (float)(x * TS_TILE), (float)(y * TS_TILE)) << TS_ID_BITS) : id;
                    }
                    o++;
                }
    }
    unsigned long long big = ballot64(tiles > SMALL);
    while (big)
    {
        const int j = __builtin_ctzll(big);
        big &= big - 1;
        const uint32_t t_minx = __shfl(minx, j), t_miny = __shfl(miny, j), t_maxx = __shfl(maxx, j), t_maxy = __shfl(maxy, j);
        const uint32_t t_tiles = __shfl(tiles, j), t_off = __shfl(off, j), t_id = __shfl(id, j);
        const uint32_t w = t_maxx - t_minx;
        QuadSetup tq{};
        if (qm && !staged) tq = setup_of(t_id, t_minx, t_miny, t_maxx, t_maxy); // every lane of the wave for itself: the same record, no 20-value broadcast
        for (uint32_t k = lane; k < t_tiles; k += 64)
        {
            const uint32_t y = t_miny + k / w, x = t_minx + k % w;
            if (staged)
            {
                stage_t[t_off - run0 + k] = qstage ? ((k % w) | ((k / w) << 12) | ((uint32_t)(wave * 64 + j) << 24)) : y * grid_x + x;
                if (!qstage) stage_v[t_off - run0 + k] = t_id;
            }
            else
            {
                if (bm)
                {
                    const uint32_t m16 = block_mask(tq, (float)(x * TS_TILE), (float)(y * TS_TILE));
                    tile_out[t_off + k] = (y * grid_x + x) | (m16 << 16);
                    val_out[t_off + k] = t_id | (quadrants_of_blocks(m16) << TS_ID_BITS);
                }
                else
                {
                    tile_out[t_off + k] = y * grid_x + x;
                    val_out[t_off + k] = qm ? t_id | (quadrant_mask(tq, (float)(x * TS_TILE), (float)(y * TS_TILE)) << TS_ID_BITS) : t_id;
                }
            }
        }
    }
    if (staged)
    {
        __syncthreads();
        for (uint32_t k = t; k < run; k += 256)
        {
            uint32_t tl = stage_t[k], v;
            if (qstage)
            {
                const uint32_t dx = tl & 0xfffu, dy = (tl >> 12) & 0xfffu, slot = tl >> 24;
                QuadAffine qa;
                qa.a = region_b[4 * slot]; qa.b = region_b[4 * slot + 1]; qa.c = region_b[4 * slot + 2]; qa.d = region_b[4 * slot + 3];
                const uint32_t org = __float_as_uint(qa.d.z), x = (org & 0xffffu) + dx, y = (org >> 16) + dy;
                if (bm)
                {
                    const uint32_t m16 = block_mask_affine(qa, dx, dy, x, y);
                    v = __float_as_uint(qa.d.y) | (quadrants_of_blocks(m16) << TS_ID_BITS);
                    tl = (y * grid_x + x) | (m16 << 16);
                }
                else
                {
                    v = __float_as_uint(qa.d.y) | (quadrant_mask_affine(qa, dx, dy, x, y) << TS_ID_BITS);
                    tl = y * grid_x + x;
                }
            }
            else v = stage_v[k];
            tile_out[run0 + k] = tl;
            val_out[run0 + k] = v;
        }
    }
}

// Four consecutive instances per thread (one dwordx4 + the word in front): a quarter of the workgroups and of the loads of the one-key-per-thread
// form (10.4 -> 7.6 us at the headline, 38.9 -> 19.1 us at 5 M triangles: profiles/r05_notes.md section 12).  `tile` is 16-byte aligned (ts_carve); words past N are never looked at.
// keymask: the key's tile bits (ts_tile_keymask: above them a 2D instance carries its block mask).
__global__ void __launch_bounds__(256) tile_ranges_kernel(int64_t N, const unsigned long long *n_dev, const uint32_t *__restrict__ tile,
                                                           uint2 *__restrict__ ranges, uint32_t keymask)
{
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (n_dev)
    {
        const unsigned long long live = *n_dev;
        N = (live <= (unsigned long long)N) ? (int64_t)live : 0;
    }
    if (i0 >= N) return;
    uint32_t k[4];
    if (i0 + 3 < N)
    {
        const uint4 q = *(const uint4 *)(tile + i0);
        k[0] = q.x & keymask; k[1] = q.y & keymask; k[2] = q.z & keymask; k[3] = q.w & keymask;
    }
    else
        for (int j = 0; j < 4; j++) k[j] = i0 + j < N ? tile[i0 + j] & keymask : 0u;
    uint32_t prev = i0 > 0 ? tile[i0 - 1] & keymask : 0u;
#pragma unroll
    for (int j = 0; j < 4; j++)
    {
        const int64_t i = i0 + j;
        if (i >= N) break;
        const uint32_t cur = k[j];
        if (i == 0) ranges[cur].x = 0;
        else if (cur != prev)
        {
            ranges[prev].y = (uint32_t)i;
            ranges[cur].x = (uint32_t)i;
        }
        if (i == N - 1) ranges[cur].y = (uint32_t)N;
        prev = cur;
    }
}
} // namespace

void ts_launch_emit_keys(int P, int grid_x, int ntiles, const GeometryStateView &g, const BinningStateView &b, const ImageStateView &im,
                         float *contrib_sum, float *contrib_max, int64_t capacity, int32_t *status, const QuadMaskArgs &qmask, hipStream_t s)
{
    if (P <= 0) return;
    const dim3 grid((unsigned)(((P + SB - 1) / SB) * 4));
    if (qmask.blocks)
        hipLaunchKernelGGL(scan_emit_kernel<true>, grid, dim3(256), 0, s, P, grid_x, ntiles, g, b, im.ranges, contrib_sum, contrib_max, (long long)capacity,
                           status, ts_scan_two_level(P), qmask);
    else
        hipLaunchKernelGGL(scan_emit_kernel<false>, grid, dim3(256), 0, s, P, grid_x, ntiles, g, b, im.ranges, contrib_sum, contrib_max, (long long)capacity,
                           status, ts_scan_two_level(P), qmask);
}
const unsigned long long *ts_instance_count_dev(const GeometryStateView &g, int P) { return (const unsigned long long *)(g.blocksum + (P + SB - 1) / SB); }

void ts_launch_tile_ranges(int64_t N, const unsigned long long *n_dev, int ntiles, const BinningStateView &b, const ImageStateView &im, hipStream_t s)
{
    if (N <= 0) return;
    hipLaunchKernelGGL(tile_ranges_kernel, dim3((unsigned)((N + 1023) / 1024)), dim3(256), 0, s, N, n_dev, b.tile, im.ranges, ts_tile_keymask(ntiles));
}
