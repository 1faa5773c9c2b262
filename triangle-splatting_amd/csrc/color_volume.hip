// color_volume.hip -- colour fused beside a TSDF volume in integers, the colour field, the trilinear sampler of a channel-planar grid and the
// per-pixel interpolation of vertex attributes (include/ts_color.h).
//
// Built with -ffp-contract=off: every float64 operation of the header rounds, so the state, the field, the samples and the interpolated
// images are bit-identical to tests/ref_color_volume.py.
//
// Integration: one thread per sample, consecutive lanes take consecutive x.  The projection of a sample into the view (steps 1-3 of the
// header) is restated here from volume.hip's integrate_kernel, not shared with it: libts_color.so links no object of libts_volume.so.  The
// three image loads are issued only for lanes inside the band, and a sample that is not coloured touches neither state array; a coloured one
// reads and writes its 28 bytes.
// Field, sampler and interpolation: one item (sample, point, pixel) per lane.  The sampler unrolls its eight corners at compile time and
// loops over the channels, so nothing is indexed at run time and no kernel here uses scratch.  The barycentrics of the interpolation are
// csrc/ts_mesh_bary.h's, which mesh_atlas.hip (libts_atlas.so) includes as well.
#include "ts_color_launch.h"
#include "ts_mesh_bary.h" // the barycentrics of a pixel, shared with mesh_atlas.hip

#include <float.h>

namespace
{
constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= FLT_MAX; }
__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= DBL_MAX; }
__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7FC00000u); }

// min(max(x, 0), 1) 65536, rounded to the nearest integer (ties to even); x is finite
__device__ __forceinline__ long long q16(float x)
{
    const double xd = (double)x, lo = xd > 0.0 ? xd : 0.0, c = lo < 1.0 ? lo : 1.0;
    return (long long)rint(c * 65536.0);
}

__global__ void __launch_bounds__(TPB) color_integrate_kernel(int nx, int ny, int n, float ox, float oy, float oz, float h, float trunc,
                                                               const float *__restrict__ view, float tan_fovx, float tan_fovy, int W, int H,
                                                               const float *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                               const float *__restrict__ image, long long *__restrict__ csum,
                                                               int32_t *__restrict__ cweight, unsigned long long *__restrict__ updated)
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
                    if (finite_f(d) && d > 0.0f)
                    {
                        const double sd = (double)d - z, tr = (double)trunc;
                        if (sd >= -tr && sd <= tr) // the band in which the distance is not clipped
                        {
                            const size_t plane = (size_t)W * (size_t)H;
                            const float x0 = image[pix], x1 = image[plane + pix], x2 = image[2 * plane + pix];
                            if (finite_f(x0) && finite_f(x1) && finite_f(x2))
                            {
                                const int32_t w = cweight[idx];
                                if (w != INT32_MAX)
                                {
                                    long long *c = csum + 3 * (size_t)idx;
                                    c[0] += q16(x0);
                                    c[1] += q16(x1);
                                    c[2] += q16(x2);
                                    cweight[idx] = w + 1;
                                    update = true;
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    if (updated) // one atomic per block that coloured anything
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

__global__ void __launch_bounds__(TPB) color_field_kernel(int n, const long long *__restrict__ csum, const int32_t *__restrict__ cweight,
                                                           int min_weight, float *__restrict__ field)
{
    const int idx = blockIdx.x * TPB + threadIdx.x;
    if (idx >= n) return;
    const int32_t w = cweight[idx];
    const bool ok = w >= min_weight;
    const double scale = (double)w * 65536.0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        field[(size_t)c * (size_t)n + idx] = ok ? (float)((double)csum[3 * (size_t)idx + c] / scale) : quiet_nan();
}

__global__ void __launch_bounds__(TPB) sample_kernel(int nx, int ny, int nz, float ox, float oy, float oz, float h, int C,
                                                      const float *__restrict__ grid, int N, const float *__restrict__ points,
                                                      float *__restrict__ out, uint8_t *__restrict__ valid)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= N) return;
    const double hd = (double)h;
    const double gx = ((double)points[3 * (size_t)i] - (double)ox) / hd;
    const double gy = ((double)points[3 * (size_t)i + 1] - (double)oy) / hd;
    const double gz = ((double)points[3 * (size_t)i + 2] - (double)oz) / hd;
    const bool inside = gx >= 0.0 && gx <= (double)(nx - 1) && gy >= 0.0 && gy <= (double)(ny - 1) && gz >= 0.0 && gz <= (double)(nz - 1); // a NaN fails
    float *o = out + (size_t)i * (size_t)C;
    if (!inside)
    {
        for (int c = 0; c < C; ++c) o[c] = quiet_nan();
        valid[i] = 0;
        return;
    }
    const int bx = nx >= 2 ? min((int)floor(gx), nx - 2) : 0;
    const int by = ny >= 2 ? min((int)floor(gy), ny - 2) : 0;
    const int bz = nz >= 2 ? min((int)floor(gz), nz - 2) : 0;
    const double tx = gx - (double)bx, ty = gy - (double)by, tz = gz - (double)bz;
    // an axis of one sample has no upper corner: its stride is 0 (every address stays inside the grid) and the corners with its bit set do not exist
    const size_t sx = nx >= 2 ? 1 : 0, sy = ny >= 2 ? (size_t)nx : 0, sz = nz >= 2 ? (size_t)nx * (size_t)ny : 0;
    const uint32_t exist = (nx >= 2 ? 0xFFu : 0x55u) & (ny >= 2 ? 0xFFu : 0x33u) & (nz >= 2 ? 0xFFu : 0x0Fu);
    const size_t n = (size_t)nx * (size_t)ny * (size_t)nz, base = ((size_t)bz * (size_t)ny + (size_t)by) * (size_t)nx + (size_t)bx;
    uint32_t data = exist;
    for (int c = 0; c < C; ++c)
    {
        const float *g = grid + (size_t)c * n + base;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (!finite_f(g[(k & 1) * sx + ((k >> 1) & 1) * sy + ((k >> 2) & 1) * sz])) data &= ~(1u << k);
    }
    double w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = (((k & 1) ? tx : 1.0 - tx) * (((k >> 1) & 1) ? ty : 1.0 - ty)) * (((k >> 2) & 1) ? tz : 1.0 - tz);
    double den = 0.0;
    bool first = true;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (data >> k & 1)
        {
            den = first ? w[k] : den + w[k];
            first = false;
        }
    const bool ok = den > 0.0;
    for (int c = 0; c < C; ++c)
    {
        const float *g = grid + (size_t)c * n + base;
        double num = 0.0;
        first = true;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (data >> k & 1)
            {
                const double term = w[k] * (double)g[(k & 1) * sx + ((k >> 1) & 1) * sy + ((k >> 2) & 1) * sz];
                num = first ? term : num + term;
                first = false;
            }
        o[c] = ok ? (float)(num / den) : quiet_nan();
    }
    valid[i] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(TPB) interpolate_kernel(const float *__restrict__ view, float tan_fovx, float tan_fovy, int W, int H, int V,
                                                           const float *__restrict__ vertices, int F, const int32_t *__restrict__ faces,
                                                           const int32_t *__restrict__ face_idx, int C, const float *__restrict__ attributes,
                                                           const float *__restrict__ background, float *__restrict__ out, float *__restrict__ bary)
{
    const size_t plane = (size_t)W * (size_t)H, p = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= plane) return;
    int ia, ib, ic;
    if (!drawn_face(face_idx[p], F, V, faces, ia, ib, ic)) // not drawn
    {
        for (int ch = 0; ch < C; ++ch) out[(size_t)ch * plane + p] = background[ch];
        if (bary) bary[p] = bary[plane + p] = bary[2 * plane + p] = 0.0f;
        return;
    }
    double alpha, beta, gamma;
    pixel_barycentrics(view, tan_fovx, tan_fovy, W, H, (int)(p % (size_t)W), (int)(p / (size_t)W), vertices, ia, ib, ic, alpha, beta, gamma);
    const float *A = attributes + (size_t)ia * (size_t)C, *B = attributes + (size_t)ib * (size_t)C, *G = attributes + (size_t)ic * (size_t)C;
    for (int ch = 0; ch < C; ++ch)
        out[(size_t)ch * plane + p] = (float)((alpha * (double)A[ch] + beta * (double)B[ch]) + gamma * (double)G[ch]);
    if (bary)
    {
        bary[p] = (float)alpha;
        bary[plane + p] = (float)beta;
        bary[2 * plane + p] = (float)gamma;
    }
}

inline unsigned blocks_of(size_t items) { return (unsigned)((items + TPB - 1) / TPB); }
} // namespace

hipError_t ts_color_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float h, float trunc, const float *view, float tan_fovx,
                              float tan_fovy, int W, int H, const float *depth, const uint8_t *mask, const float *image, long long *csum,
                              int32_t *cweight, unsigned long long *updated, hipStream_t s)
{
    const int n = nx * ny * nz;
    hipLaunchKernelGGL(color_integrate_kernel, dim3(blocks_of((size_t)n)), dim3(TPB), 0, s, nx, ny, n, ox, oy, oz, h, trunc, view, tan_fovx, tan_fovy,
                       W, H, depth, mask, image, csum, cweight, updated);
    return hipGetLastError();
}

hipError_t ts_color_field(int n, const long long *csum, const int32_t *cweight, int min_weight, float *field, hipStream_t s)
{
    hipLaunchKernelGGL(color_field_kernel, dim3(blocks_of((size_t)n)), dim3(TPB), 0, s, n, csum, cweight, min_weight, field);
    return hipGetLastError();
}

hipError_t ts_color_sample(int nx, int ny, int nz, float ox, float oy, float oz, float h, int C, const float *grid, int N, const float *points,
                           float *out, uint8_t *valid, hipStream_t s)
{
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(sample_kernel, dim3(blocks_of((size_t)N)), dim3(TPB), 0, s, nx, ny, nz, ox, oy, oz, h, C, grid, N, points, out, valid);
    return hipGetLastError();
}

hipError_t ts_color_interpolate(const float *view, float tan_fovx, float tan_fovy, int W, int H, int V, const float *vertices, int F,
                                const int32_t *faces, const int32_t *face_idx, int C, const float *attributes, const float *background, float *out,
                                float *bary, hipStream_t s)
{
    hipLaunchKernelGGL(interpolate_kernel, dim3(blocks_of((size_t)W * (size_t)H)), dim3(TPB), 0, s, view, tan_fovx, tan_fovy, W, H, V, vertices, F,
                       faces, face_idx, C, attributes, background, out, bary);
    return hipGetLastError();
}
