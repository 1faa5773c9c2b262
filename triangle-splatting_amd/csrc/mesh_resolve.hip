// mesh_resolve.hip -- the per-pixel depth test of the opaque mesh renderer (include/ts_mesh.h).
//
// One workgroup per 16 x 16 tile, one pixel per lane, wavefront w = pixel rows 4 w .. 4 w + 3.  The tile's face list (ascending
// nearest-vertex depth, then face index: mesh_preprocess.hip + the ordering chain) is streamed through LDS in batches of 256: lane t
// gathers face t's 64-byte record and leaves 16 words of per-(face, tile) constants -- three edge functions and the ray / plane
// denominator as affine functions of the pixel's offset inside the TILE (local origin: the constants carry no image-sized terms) --
// and every lane then walks the batch with two FMAs per edge.  Each pixel keeps (depth, face) in registers; no global atomics.
//
// Early stop, exact: a face whose key (nearest vertex depth) is greater than what a pixel holds cannot win that pixel -- its depth there
// is clamped to its own vertices' range, so it is >= the key -- and the keys only grow along the list.  A wavefront therefore leaves
// the walk at the first face with  key > kept depth  on ALL its pixels (one compare + ballot per face; `>` strictly, so a face that
// ties a kept depth with a smaller index is still visited), and the workgroup stops fetching batches once its four wavefronts have.
// Pixels outside the image hold depth 0 from the start: they never accept a face and never keep a wavefront going.
// Built with -ffp-contract=off: what is fused is written as fmaf.
#include "ts2d_common.h"
#include "ts2d_wave.h"

namespace
{
constexpr int MESH_BATCH = 256;

__global__ void __launch_bounds__(256) mesh_resolve_kernel(MeshArgs a, const float4 *__restrict__ rec, const uint32_t *__restrict__ vals,
                                                           const uint2 *__restrict__ ranges, const float *__restrict__ faces_color,
                                                           const float *__restrict__ background, float *__restrict__ render,
                                                           float *__restrict__ mask, float *__restrict__ depth, int32_t *__restrict__ face_idx,
                                                           unsigned long long *wave_visits)
{
    __shared__ float4 s_face[MESH_BATCH * 4 + 4]; // + one padding row for the walk's read-ahead
    __shared__ int s_done[4];
    const int tile = tile_of_block(blockIdx.x, a.grid_x, a.grid_y);
    if (tile < 0) return; // padding of the XCD-aware mapping (uniform for the workgroup)
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int tx = tile % a.grid_x, ty = tile / a.grid_x;
    const int px = tx * TS_TILE + (t & 15), py = ty * TS_TILE + (t >> 4);
    const bool in_image = px < a.W && py < a.H;
    const float fx = (float)(t & 15) + 0.5f, fy = (float)(t >> 4) + 0.5f; // the pixel centre, relative to the tile's corner
    const float ox = (float)(tx * TS_TILE), oy = (float)(ty * TS_TILE);
    // ray through pixel centre (X, Y): r = ((2 X / W - 1) tan_fovx, (2 Y / H - 1) tan_fovy, 1), affine in (fx, fy)
    const float rx_step = 2.0f / (float)a.W * a.tan_fovx, ry_step = 2.0f / (float)a.H * a.tan_fovy;
    const float rx0 = (2.0f * ox / (float)a.W - 1.0f) * a.tan_fovx, ry0 = (2.0f * oy / (float)a.H - 1.0f) * a.tan_fovy;

    const uint2 range = ranges[tile];
    float best = in_image ? __int_as_float(0x7f800000) : 0.0f;
    uint32_t best_id = 0xFFFFFFFFu;
    bool done = false; // wave-uniform
    uint32_t visits = 0;

    for (uint32_t base = range.x; base < range.y; base += MESH_BATCH)
    {
        if (lane == 0) s_done[wave] = done ? 1 : 0;
        __syncthreads(); // the previous batch has been walked by everyone; the four flags are in
        if (s_done[0] & s_done[1] & s_done[2] & s_done[3]) break; // uniform: every wavefront read the same four words
        const uint32_t n = min((uint32_t)MESH_BATCH, range.y - base);
        if ((uint32_t)t < n)
        {
            const uint32_t id = vals[base + t] & TS_ID_MASK;
            const float4 *rp = rec + 4 * (size_t)id;
            const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2];
            const float x1 = r0.x - ox, y1 = r0.y - oy, x2 = r0.z - ox, y2 = r0.w - oy, x3 = r1.x - ox, y3 = r1.y - oy; // tile-local
            const float e1x = x2 - x1, e1y = y2 - y1, e2x = x3 - x2, e2y = y3 - y2, e3x = x1 - x3, e3y = y1 - y3;
            const float sgn = (e1x * (y3 - y1) - e1y * (x3 - x1)) < 0.0f ? -1.0f : 1.0f;
            // edge i from vertex p with direction e: E(X, Y) = sgn (e.x (Y - p.y) - e.y (X - p.x)) >= 0 inside or on the triangle
            const float A1 = -sgn * e1y, B1 = sgn * e1x, C1 = sgn * (e1y * x1 - e1x * y1);
            const float A2 = -sgn * e2y, B2 = sgn * e2x, C2 = sgn * (e2y * x2 - e2x * y2);
            const float A3 = -sgn * e3y, B3 = sgn * e3x, C3 = sgn * (e3y * x3 - e3x * y3);
            const float nx = r1.z, ny = r1.w, nz = r2.x;
            const float Dx = nx * rx_step, Dy = ny * ry_step, D0 = fmaf(nx, rx0, fmaf(ny, ry0, nz)); // n . r = Dx fx + Dy fy + D0
            float4 *o = s_face + 4 * t;
            o[0] = make_float4(r2.z, A1, B1, C1); // .x = the key
            o[1] = make_float4(A2, B2, C2, A3);
            o[2] = make_float4(B3, C3, Dx, Dy);
            o[3] = make_float4(D0, r2.y, r2.w, __uint_as_float(id)); // n . v1, farthest vertex depth, face
        }
        __syncthreads();
        if (done) continue;
        // software-pipelined: face j + 1's constants are requested before face j is tested, so one LDS latency per face is exposed instead of
        // two dependent ones (the row behind the last face is padding: read, never used)
        float4 q0 = s_face[0], q1 = s_face[1], q2 = s_face[2];
        for (uint32_t j = 0; j < n; j++)
        {
            const float4 p0 = s_face[4 * j + 4], p1 = s_face[4 * j + 5], p2 = s_face[4 * j + 6];
            if (__ballot(q0.x <= best) == 0ull) { done = true; break; }
            visits++;
            const float E1 = fmaf(q0.y, fx, fmaf(q0.z, fy, q0.w));
            const float E2 = fmaf(q1.x, fx, fmaf(q1.y, fy, q1.z));
            const float E3 = fmaf(q1.w, fx, fmaf(q2.x, fy, q2.y));
            if (E1 >= 0.0f && E2 >= 0.0f && E3 >= 0.0f)
            {
                const float4 q3 = s_face[4 * j + 3];
                const float den = fmaf(q2.z, fx, fmaf(q2.w, fy, q3.x));
                // ray / plane depth, kept inside the face's own depth range (where the exact value lies; fmaxf / fminf also absorb a NaN)
                const float d = fminf(fmaxf(q3.y / den, q0.x), q3.z);
                const uint32_t id = __float_as_uint(q3.w);
                if (d < best || (d == best && id < best_id))
                {
                    best = d;
                    best_id = id;
                }
            }
            q0 = p0; q1 = p1; q2 = p2;
        }
    }
    if (wave_visits && lane == 0 && visits) atomicAdd(wave_visits, (unsigned long long)visits);
    if (!in_image) return;
    const bool covered = best_id != 0xFFFFFFFFu;
    const size_t pix = (size_t)py * a.W + px, plane = (size_t)a.W * a.H;
    const float *c = covered ? faces_color + 3 * (size_t)best_id : background;
    render[pix] = fminf(fmaxf(c[0], 0.0f), 1.0f);
    render[plane + pix] = fminf(fmaxf(c[1], 0.0f), 1.0f);
    render[2 * plane + pix] = fminf(fmaxf(c[2], 0.0f), 1.0f);
    mask[pix] = covered ? 1.0f : 0.0f;
    if (depth) depth[pix] = covered ? best : 0.0f;
    if (face_idx) face_idx[pix] = covered ? (int32_t)best_id : -1;
}
} // namespace

void ts_launch_mesh_resolve(const MeshArgs &a, const GeometryStateView &g, const BinningStateView &b, const ImageStateView &im,
                            const float *faces_color, const float *background, float *render, float *mask, float *depth, int32_t *face_idx,
                            unsigned long long *wave_visits, hipStream_t s)
{
    hipLaunchKernelGGL(mesh_resolve_kernel, dim3((unsigned)ts_tile_units(a.grid_x, a.grid_y)), dim3(256), 0, s, a, (const float4 *)g.rec,
                       (const uint32_t *)b.vals, (const uint2 *)im.ranges, faces_color, background, render, mask, depth, face_idx, wave_visits);
}
