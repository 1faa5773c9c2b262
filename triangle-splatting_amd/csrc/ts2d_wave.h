// ts2d_wave.h -- wave64 building blocks of the 2D and 3D blend kernels (gfx950): the wave-order LDS fence (ts2d_radix.h uses it too), DPP lane
// moves, a fast power of non-negative floats, XCD-aware tile mapping.
// Costs measured on MI355X (profiles/r01_valu_microbench.txt): DPP add 4.5, plain VOP2 fp32 2.6, v_exp/v_rcp 8.3 cycles per wave instruction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace
{
// Orders this wave's LDS accesses ACROSS LANES at this point of the program: the per-thread language model lets the compiler
// merge or reorder the accesses of different lanes (it did: three lane groups' read-add-write sequences became three reads and
// one common write); a wavefront-scope fence + wave_barrier pins them.  No instruction is emitted: LDS executes a wave's
// accesses in order.
__device__ __forceinline__ void wave_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
constexpr int DPP_XOR1 = 0xB1;        // quad_perm:[1,0,3,2]
constexpr int DPP_XOR2 = 0x4E;        // quad_perm:[2,3,0,1]
constexpr int DPP_HALF_MIRROR = 0x141; // lane -> 7 - lane inside each group of 8
constexpr int DPP_MIRROR = 0x140;     // lane -> 15 - lane inside a row of 16

// x^y for x >= 0, y >= 0 via v_log_f32 / v_exp_f32 (x = 0 -> 0, y = 0 -> 1 like powf).
__device__ __forceinline__ float pow_nonneg(float x, float y)
{
    const float r = __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x));
    return y == 0.0f ? 1.0f : r;
}

// blockIdx -> tile.  Workgroups are handed to the 8 XCDs round-robin (block b runs on XCD b % 8) and an XCD never takes over another
// one's blocks, so the mapping decides two things: which tiles share an L2 (neighbouring tiles gather mostly the same triangle records),
// and how evenly the WORK is spread over the XCDs.  XCD x owns the tile ROWS x, x + 8, x + 16, ... of the first 8 floor(rows / 8) rows --
// every XCD samples the whole image height, horizontal neighbours still share an L2 (a row of 120 tiles at 1080p), vertical neighbours are
// fetched by two XCDs -- and an eighth of the tiles of the remaining rows (68 rows at 1080p: XCDs with nine rows against XCDs with eight
// would cost the uniform scene 6 %).  Rounds 1-3 gave each XCD one contiguous band of rows instead, measured and dropped in round 4: the
// same triangles concentrated about the optical axis 1.52 instead of 1.00 ms per step, the uniform headline scene within 1 % of it
// (profiles/r04_notes.md, profiles/r04_xcd_mapping.txt).
// Every XCD gets ceil(ntiles / 8) units; a unit past its share returns -1 (the grid is padded to 8 x that).
static inline int ts_tile_units(int grid_x, int grid_y) { return 8 * ((grid_x * grid_y + 7) / 8); }
__device__ __forceinline__ int tile_of_block(int b, int grid_x, int grid_y)
{
    const int x = b & 7, i = b >> 3;
    const int rows8 = grid_y >> 3, full = rows8 * grid_x; // units of an XCD that are whole rows
    if (i < full) return (x + 8 * (i / grid_x)) * grid_x + i % grid_x;
    const int rest = (grid_y & 7) * grid_x, q = rest >> 3, r = rest & 7, k = i - full; // the last grid_y % 8 rows, shared out tile by tile
    return k < q + (x < r ? 1 : 0) ? 8 * full + x * q + min(x, r) + k : -1;
}

} // namespace
