// mesh_atlas.hip -- the texture atlas of an indexed mesh (include/ts_atlas.h): the texel of every pixel of a face_idx image, the per-face
// totals of the texel accumulator, the resolve of the accumulator into an image and the draw of that image over a view.
//
// Built with -ffp-contract=off: every float64 operation of the header rounds, so the indices, the barycentrics and the image are
// bit-identical to tests/ref_mesh_texture.py.  The barycentrics are csrc/ts_mesh_bary.h's, the one statement color_volume.hip
// (tsc_interpolate) is built from as well.
//
// Texel index, resolve and render: one item (pixel, atlas texel, pixel) per lane, consecutive lanes take consecutive items, so every image
// load and store is coalesced; the gathers (faces, vertices, accumulator rows) follow the face of the pixel, which neighbouring lanes share.
// Face totals: a segmented integer reduction without atomics.  The T rows of a face are 4 T consecutive 64-bit words; a group of G lanes
// (a power of two, 4 <= G <= 64, G >= min(4 T, 64)) walks them with stride G, so a lane always reads the same column of the rows (G is a
// multiple of 4) and a wave reads 512 consecutive bytes per step; the lanes of a column are then added by xor-shuffles over the offsets
// G / 2 .. 4.  At T == 1 that is 16 faces per wave and no shuffle, from T >= 16 on one wave per face.
// No kernel here indexes an array at run time, none uses scratch or LDS (profiles/mesh_atlas_resources.txt).
#include "ts_atlas_launch.h"
#include "ts_mesh_bary.h"

namespace
{
constexpr int TPB = 256;

__global__ void __launch_bounds__(TPB) texel_index_kernel(const float *__restrict__ view, float tan_fovx, float tan_fovy, int W, int H, int V,
                                                           const float *__restrict__ vertices, int F, const int32_t *__restrict__ faces,
                                                           const int32_t *__restrict__ face_idx, int R, int Cx, int32_t *__restrict__ texel_idx,
                                                           int32_t *__restrict__ atlas_idx, float *__restrict__ bary)
{
    const size_t plane = (size_t)W * (size_t)H, p = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= plane) return;
    const int f = face_idx[p];
    int ia, ib, ic;
    if (!drawn_face(f, F, V, faces, ia, ib, ic))
    {
        texel_idx[p] = -1;
        if (atlas_idx) atlas_idx[p] = -1;
        if (bary) bary[p] = bary[plane + p] = bary[2 * plane + p] = 0.0f;
        return;
    }
    double alpha, beta, gamma;
    pixel_barycentrics(view, tan_fovx, tan_fovy, W, H, (int)(p % (size_t)W), (int)(p / (size_t)W), vertices, ia, ib, ic, alpha, beta, gamma);
    int i = (int)floor(beta * (double)R); // beta and gamma lie in [0, 1] and R <= 64: the casts are exact
    i = i < R - 1 ? i : R - 1;
    int j = (int)floor(gamma * (double)R);
    j = j < R - 1 - i ? j : R - 1 - i;
    const int T = R * (R + 1) / 2;
    texel_idx[p] = f * T + j * R - j * (j - 1) / 2 + i; // F T <= 2^31 - 1 (api_atlas.hip)
    if (atlas_idx)
    {
        const int k = f >> 1, X0 = (k % Cx) * (R + 1), Y0 = (k / Cx) * R, Wa = Cx * (R + 1); // Wa Ha <= 2^31 - 1
        const int x = (f & 1) ? X0 + R - i : X0 + i, y = (f & 1) ? Y0 + R - 1 - j : Y0 + j;
        atlas_idx[p] = y * Wa + x;
    }
    if (bary)
    {
        bary[p] = (float)alpha;
        bary[plane + p] = (float)beta;
        bary[2 * plane + p] = (float)gamma;
    }
}

__global__ void __launch_bounds__(TPB) face_totals_kernel(int F, int T, int G, const unsigned long long *__restrict__ texels,
                                                           unsigned long long *__restrict__ face_totals)
{
    const size_t face = ((size_t)blockIdx.x * TPB + threadIdx.x) / (size_t)G; // G divides 64: a group never straddles a wave
    const int lane = (int)threadIdx.x & (G - 1);
    unsigned long long sum = 0;
    if (face < (size_t)F)
    {
        const unsigned long long *row = texels + 4 * face * (size_t)T;
        for (int w = lane, words = 4 * T; w < words; w += G) sum += row[w];
    }
    for (int off = G >> 1; off >= 4; off >>= 1) sum += __shfl_xor(sum, off); // every lane of the wave takes part: G is uniform
    if (face < (size_t)F && lane < 4) face_totals[4 * face + lane] = sum;
}

// (float)((double)sum / ((double)count 65536))
__device__ __forceinline__ float mean_q16(unsigned long long sum, unsigned long long count)
{
    return (float)((double)sum / ((double)count * 65536.0));
}

// (uint8) rint(min(max(c, 0), 1) 255) in double; a NaN gives 0
__device__ __forceinline__ uint8_t to_byte(float c)
{
    const double cd = (double)c, lo = cd > 0.0 ? cd : 0.0, hi = lo < 1.0 ? lo : 1.0;
    return (uint8_t)rint(hi * 255.0);
}

__global__ void __launch_bounds__(TPB) resolve_kernel(int F, int R, int Cx, size_t texels_total /* Wa Ha */,
                                                       const unsigned long long *__restrict__ texels,
                                                       const unsigned long long *__restrict__ face_totals, int min_count,
                                                       const float *__restrict__ face_fallback, float fill_r, float fill_g, float fill_b,
                                                       float *__restrict__ image, uint8_t *__restrict__ state, uint8_t *__restrict__ rgb8)
{
    const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= texels_total) return;
    const int Wa = Cx * (R + 1);
    const int x = (int)(t % (size_t)Wa), y = (int)(t / (size_t)Wa);
    const int lx = x % (R + 1), ly = y % R;
    const long long k = (long long)(y / R) * Cx + x / (R + 1);
    const bool lower = lx + ly <= R - 1;
    const long long f = lower ? 2 * k : 2 * k + 1;
    float r = fill_r, g = fill_g, b = fill_b;
    uint8_t st = 0;
    if (f < (long long)F)
    {
        const int i = lower ? lx : R - lx, j = lower ? ly : R - 1 - ly;
        const size_t n = (size_t)f * (size_t)(R * (R + 1) / 2) + (size_t)(j * R - j * (j - 1) / 2 + i);
        const unsigned long long count = texels[4 * n];
        if (count >= (unsigned long long)min_count)
        {
            r = mean_q16(texels[4 * n + 1], count);
            g = mean_q16(texels[4 * n + 2], count);
            b = mean_q16(texels[4 * n + 3], count);
            st = 3;
        }
        else
        {
            const unsigned long long total = face_totals[4 * (size_t)f];
            if (total >= 1)
            {
                r = mean_q16(face_totals[4 * (size_t)f + 1], total);
                g = mean_q16(face_totals[4 * (size_t)f + 2], total);
                b = mean_q16(face_totals[4 * (size_t)f + 3], total);
                st = 2;
            }
            else if (face_fallback)
            {
                r = face_fallback[3 * (size_t)f];
                g = face_fallback[3 * (size_t)f + 1];
                b = face_fallback[3 * (size_t)f + 2];
                st = 1;
            }
        }
    }
    image[t] = r;
    image[texels_total + t] = g;
    image[2 * texels_total + t] = b;
    state[t] = st;
    if (rgb8)
    {
        rgb8[3 * t] = to_byte(r);
        rgb8[3 * t + 1] = to_byte(g);
        rgb8[3 * t + 2] = to_byte(b);
    }
}

__global__ void __launch_bounds__(TPB) render_kernel(size_t plane /* W H */, int atlas_texels /* Wa Ha */, const int32_t *__restrict__ atlas_idx,
                                                      const float *__restrict__ image, const float *__restrict__ background,
                                                      float *__restrict__ out)
{
    const size_t p = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= plane) return;
    const int a = atlas_idx[p];
    const bool ok = a >= 0 && a < atlas_texels;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[(size_t)ch * plane + p] = ok ? image[(size_t)ch * (size_t)atlas_texels + (size_t)a] : background[ch];
}

inline unsigned blocks_of(size_t items) { return (unsigned)((items + TPB - 1) / TPB); }
} // namespace

hipError_t ts_atlas_texel_index(const float *view, float tan_fovx, float tan_fovy, int W, int H, int V, const float *vertices, int F,
                                const int32_t *faces, const int32_t *face_idx, int R, int Cx, int32_t *texel_idx, int32_t *atlas_idx, float *bary,
                                hipStream_t s)
{
    hipLaunchKernelGGL(texel_index_kernel, dim3(blocks_of((size_t)W * (size_t)H)), dim3(TPB), 0, s, view, tan_fovx, tan_fovy, W, H, V, vertices, F,
                       faces, face_idx, R, Cx, texel_idx, atlas_idx, bary);
    return hipGetLastError();
}

hipError_t ts_atlas_face_totals(int F, int R, const unsigned long long *texels, unsigned long long *face_totals, hipStream_t s)
{
    if (F == 0) return hipSuccess;
    const int T = R * (R + 1) / 2;
    int G = 4;
    while (G < 64 && G < 4 * T) G <<= 1;
    hipLaunchKernelGGL(face_totals_kernel, dim3(blocks_of((size_t)F * (size_t)G)), dim3(TPB), 0, s, F, T, G, texels, face_totals);
    return hipGetLastError();
}

hipError_t ts_atlas_resolve(int F, int R, int Cx, int Cy, const unsigned long long *texels, const unsigned long long *face_totals, int min_count,
                            const float *face_fallback, float fill_r, float fill_g, float fill_b, float *image, uint8_t *state, uint8_t *rgb8,
                            hipStream_t s)
{
    const size_t total = (size_t)Cx * (size_t)(R + 1) * (size_t)Cy * (size_t)R;
    hipLaunchKernelGGL(resolve_kernel, dim3(blocks_of(total)), dim3(TPB), 0, s, F, R, Cx, total, texels, face_totals, min_count, face_fallback,
                       fill_r, fill_g, fill_b, image, state, rgb8);
    return hipGetLastError();
}

hipError_t ts_atlas_render(int W, int H, int Wa, int Ha, const int32_t *atlas_idx, const float *image, const float *background, float *out,
                           hipStream_t s)
{
    const size_t plane = (size_t)W * (size_t)H;
    hipLaunchKernelGGL(render_kernel, dim3(blocks_of(plane)), dim3(TPB), 0, s, plane, Wa * Ha, atlas_idx, image, background, out);
    return hipGetLastError();
}
