// regularizers.hip -- the regularisation half of the reference's training loss and its per-view colour affine (include/ts_loss.h).
//
//   scaling_reg = get_scaling.mean()                                   src/diff_recon/trainers/VanillaTS_trainer.py:87, VanillaTS_model.py:72-76
//   opacity_reg = (0.25 - (o - 0.5)^2).mean()  or  (1 - o).mean()      VanillaTS_trainer.py:89-97
//   vertex_reg  = nearest_dist2(vertex.view(-1, 3), nearest).mean()   VanillaTS_trainer.py:107-109, trainer_utils.py:339-346
//   image       = clamp(image.permute(1, 2, 0) @ W[uid] + b[uid], 0, 1)  VanillaTS_model.py:678-684
// Reference = eager torch: a chain of elementwise, norm, stack, mean and indexing kernels and their autograd counterparts, the neighbour term's
// backward an index-accumulate (float atomics).  Here: the three per-triangle terms in one pass + a one-wave finisher (deterministic two-stage sums
// in double over a fixed grid, as aux_losses.hip), their gradient in one gather-form pass -- the neighbour term reads an inverse of the nearest
// relation that tsl_reg_prepare builds with the library's stable radix sort each time the nearest indices are refreshed -- and the affine in one
// pass each way (+ a finisher for the 12 parameter gradients).  No float atomics, no host read: every call can be captured into a graph.  HBM-bound.
#include "../../include/ts_loss.h"
#include "ts2d_common.h"
#include "ts2d_tri.h"

namespace
{
constexpr int TPB = 256;
constexpr int SUM_BLOCKS = 2048;  // fixed grid of the two-stage sums (guide: cap ~2048 blocks and grid-stride the rest)
constexpr int AFF_PARTS = 12;     // dW (3 x 3, row k = input channel) + db (3)

// ---- per-triangle regularisers ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double s, double *red) // red: 4 doubles of LDS; the sum lands in thread 0
{
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const double t = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return t;
}

// partial[b], partial[SUM_BLOCKS + b], partial[2 SUM_BLOCKS + b]: block b's sums of s_i, of the opacity term and of |p_k - p_nearest[k]|^2.
// A term whose weight is 0 is neither read nor summed.  A nearest index outside [0, 3P) makes its term NaN (never an out-of-range read).
__global__ void __launch_bounds__(TPB) reg_sum_kernel(int P, const float *__restrict__ vertex, const float *__restrict__ opacity,
                                                      const uint32_t *__restrict__ nearest, int do_s, int omode, int do_v,
                                                      double *__restrict__ partial)
{
    __shared__ double red[4];
    double ss = 0.0, so = 0.0, sv = 0.0;
    const uint32_t n3 = 3u * (uint32_t)P;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < P; i += gridDim.x * TPB)
    {
        const float *v = vertex + 9 * (size_t)i;
        if (do_s)
        {
            float l1, l2, l3;
            ss += (double)mean_side(v, l1, l2, l3);
        }
        if (omode)
        {
            const double o = (double)opacity[i];
            so += omode == TSL_REG_OPACITY_QUAD ? 0.25 - (o - 0.5) * (o - 0.5) : 1.0 - o;
        }
        if (do_v)
#pragma unroll
            for (int c = 0; c < 3; c++)
            {
                const uint32_t n = nearest[3 * (size_t)i + c];
                if (n >= n3) { sv += __builtin_nan(""); continue; }
                const float *q = vertex + 3 * (size_t)n;
                const double x = (double)v[3 * c] - q[0], y = (double)v[3 * c + 1] - q[1], z = (double)v[3 * c + 2] - q[2];
                sv += (x * x + y * y) + z * z;
            }
    }
    ss = block_sum(ss, red);
    so = block_sum(so, red);
    sv = block_sum(sv, red);
    if (threadIdx.x == 0)
    {
        partial[blockIdx.x] = ss;
        partial[SUM_BLOCKS + blockIdx.x] = so;
        partial[2 * SUM_BLOCKS + blockIdx.x] = sv;
    }
}

// out[0] = w_s scaling_reg + w_o opacity_reg + w_v vertex_reg, out[1..3] = the three means (0 for a term that is off).  One wave: fixed
// order per lane, then a butterfly -- deterministic.
__global__ void __launch_bounds__(64) reg_finish_kernel(int nblocks, int P, float w_s, float w_o, float w_v, int do_s, int omode, int do_v,
                                                        const double *__restrict__ partial, float *__restrict__ out)
{
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nblocks; b += 64)
#pragma unroll
        for (int t = 0; t < 3; t++) s[t] += partial[t * SUM_BLOCKS + b];
#pragma unroll
    for (int t = 0; t < 3; t++)
        for (int o = 32; o > 0; o >>= 1) s[t] += __shfl_xor(s[t], o);
    if (threadIdx.x == 0)
    {
        const double ms = do_s ? s[0] / (double)P : 0.0, mo = omode ? s[1] / (double)P : 0.0, mv = do_v ? s[2] / (3.0 * (double)P) : 0.0;
        double total = 0.0;
        if (do_s) total += (double)w_s * ms;
        if (omode) total += (double)w_o * mo;
        if (do_v) total += (double)w_v * mv;
        out[0] = (float)total;
        out[1] = (float)ms;
        out[2] = (float)mo;
        out[3] = (float)mv;
    }
}

struct RegCoef
{
    float cs; // w_s / (3 P): d scaling_reg / d side length, times the weight
    float co; // w_o / P
    float cv; // 2 w_v / (3 P)
};

// One thread per triangle: dL/dvertex (9 floats) and dL/dopacity, fully written.
//   scaling: side e = a - b, length l: +cs g e / l on a, the negative on b; 0 for l == 0 (torch's norm backward masks norm == 0)
//   opacity: -2 (o - 0.5) co g (quad) or -co g (linear)
//   vertex j: cv g [(p_j - p_nearest[j]) - sum over k in inv(j) of (p_k - p_j)], the sources k in the ascending order tsl_reg_prepare left them in
__global__ void __launch_bounds__(TPB) reg_bwd_kernel(int P, const float *__restrict__ vertex, const float *__restrict__ opacity,
                                                      const uint32_t *__restrict__ nearest, const uint32_t *__restrict__ inv,
                                                      const uint32_t *__restrict__ off, RegCoef k, int do_s, int omode, int do_v,
                                                      const float *__restrict__ grad_out, float *__restrict__ dvertex, float *__restrict__ dopacity)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= P) return;
    const float g = grad_out ? *grad_out : 1.0f;
    const float *vp = vertex + 9 * (size_t)i;
    float v[9], d[9];
#pragma unroll
    for (int t = 0; t < 9; t++) { v[t] = vp[t]; d[t] = 0.0f; }
    if (do_s)
    {
        const float cs = k.cs * g;
        const int sa[3] = {2, 0, 1}, sb[3] = {1, 2, 0}; // sides (v3 - v2, v1 - v3, v2 - v1) of get_scaling
#pragma unroll
        for (int e = 0; e < 3; e++)
        {
            const float *a = v + 3 * sa[e], *b = v + 3 * sb[e];
            const float l = side_len(a, b);
            if (l > 0.0f)
            {
                const float t = cs / l;
#pragma unroll
                for (int c = 0; c < 3; c++)
                {
                    const float gc = t * (a[c] - b[c]);
                    d[3 * sa[e] + c] += gc;
                    d[3 * sb[e] + c] -= gc;
                }
            }
        }
    }
    if (do_v)
    {
        const uint32_t n3 = 3u * (uint32_t)P;
        const float cv = k.cv * g;
#pragma unroll
        for (int c = 0; c < 3; c++)
        {
            const uint32_t j = 3u * (uint32_t)i + c, n = nearest[j];
            const float *pj = v + 3 * c;
            double acc[3];
            if (n < n3)
            {
                const float *q = vertex + 3 * (size_t)n;
                for (int a = 0; a < 3; a++) acc[a] = (double)pj[a] - q[a];
            }
            else
                acc[0] = acc[1] = acc[2] = __builtin_nan("");
            const uint32_t e = min(off[j + 1], n3); // (bounded even for a buffer prepared for other indices: never an out-of-range read)
            for (uint32_t r = off[j]; r < e; r++)
            {
                const uint32_t src = inv[r];
                if (src >= n3) { acc[0] = acc[1] = acc[2] = __builtin_nan(""); break; }
                const float *q = vertex + 3 * (size_t)src;
                for (int a = 0; a < 3; a++) acc[a] -= (double)q[a] - pj[a];
            }
            for (int a = 0; a < 3; a++) d[3 * c + a] += cv * (float)acc[a];
        }
    }
    float *dp = dvertex + 9 * (size_t)i;
#pragma unroll
    for (int t = 0; t < 9; t++) dp[t] = d[t];
    float go = 0.0f;
    if (omode == TSL_REG_OPACITY_QUAD) go = -2.0f * (opacity[i] - 0.5f) * (k.co * g);
    else if (omode == TSL_REG_OPACITY_LINEAR) go = -(k.co * g);
    dopacity[i] = go;
}

// prepare, step 1: sort keys = nearest[k] clamped to n (an index outside [0, n) joins no vertex's list), values = k
__global__ void __launch_bounds__(TPB) inv_keys_kernel(uint32_t n, const uint32_t *__restrict__ nearest, uint32_t *__restrict__ key,
                                                       uint32_t *__restrict__ val)
{
    const uint32_t k = blockIdx.x * TPB + threadIdx.x;
    if (k >= n) return;
    const uint32_t t = nearest[k];
    key[k] = t < n ? t : n;
    val[k] = k;
}
// step 3: the sorted sources into inv, and run offsets: off[j] = first sorted position whose key is >= j, j = 0 .. n (every off[j] is written by
// exactly one thread: the one at the first position whose key reaches j, or the extra thread n for the keys beyond the last)
__global__ void __launch_bounds__(TPB) inv_offsets_kernel(uint32_t n, const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sval,
                                                          uint32_t *__restrict__ inv, uint32_t *__restrict__ off)
{
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i > n) return;
    if (i < n) inv[i] = sval[i];
    const uint32_t lo = i == 0 ? 0u : skey[i - 1] + 1u, hi = i < n ? skey[i] : n;
    for (uint32_t j = lo; j <= hi; j++) off[j] = i;
}

struct PrepCarve
{
    uint32_t *inv, *off, *k[2], *v[2];
    void *sort_scratch;
    size_t bytes;
};
PrepCarve prep_carve(void *ws, int P)
{
    PrepCarve c;
    const size_t n = 3 * (size_t)P;
    char *p = (char *)ws;
    ts_carve(p, c.inv, n);
    ts_carve(p, c.off, n + 1);
    for (int t = 0; t < 2; t++) { ts_carve(p, c.k[t], n); ts_carve(p, c.v[t], n); }
    p = (char *)ts_align_up((size_t)p);
    c.sort_scratch = p;
    p += ts_radix_scratch_bytes(n);
    c.bytes = (size_t)(p - (char *)ws) + TS_ALIGN;
    return c;
}

// ---- per-view colour affine ------------------------------------------------------------------------------------------------------
// y_c = x_0 W[0][c] + x_1 W[1][c] + x_2 W[2][c] + b_c (image.permute(1, 2, 0) @ W + b), without contraction
__device__ __forceinline__ void affine_pre(const float x[3], const float *W, const float *b, float y[3])
{
#pragma unroll
    for (int c = 0; c < 3; c++) y[c] = ((x[0] * W[c] + x[1] * W[3 + c]) + x[2] * W[6 + c]) + b[c];
}
__device__ __forceinline__ float clamp01(float y) { return y < 0.0f ? 0.0f : (y > 1.0f ? 1.0f : y); } // NaN stays NaN, as torch's clamp

__global__ void __launch_bounds__(TPB) affine_fwd_kernel(int HW, const float *__restrict__ x, const float *__restrict__ W, const float *__restrict__ b,
                                                         float *__restrict__ y)
{
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= HW) return;
    float w[9], bb[3], xi[3], yo[3];
#pragma unroll
    for (int t = 0; t < 9; t++) w[t] = W[t];
#pragma unroll
    for (int t = 0; t < 3; t++) { bb[t] = b[t]; xi[t] = x[(size_t)t * HW + p]; }
    affine_pre(xi, w, bb, yo);
#pragma unroll
    for (int c = 0; c < 3; c++) y[(size_t)c * HW + p] = clamp01(yo[c]);
}
// backward: the pre-clamp value is recomputed; the clamp passes the gradient where 0 <= y_pre <= 1 (torch's clamp backward, bounds included).
// dL/dx written in full; per block the 12 sums of x_k gy_c and gy_c in double
__global__ void __launch_bounds__(TPB) affine_bwd_kernel(int HW, const float *__restrict__ x, const float *__restrict__ W, const float *__restrict__ b,
                                                         const float *__restrict__ gy, float *__restrict__ gx, double *__restrict__ partial)
{
    __shared__ double red[4];
    float w[9], bb[3];
#pragma unroll
    for (int t = 0; t < 9; t++) w[t] = W[t];
#pragma unroll
    for (int t = 0; t < 3; t++) bb[t] = b[t];
    double acc[AFF_PARTS];
#pragma unroll
    for (int t = 0; t < AFF_PARTS; t++) acc[t] = 0.0;
    for (int p = blockIdx.x * TPB + threadIdx.x; p < HW; p += gridDim.x * TPB)
    {
        float xi[3], yp[3], g[3];
#pragma unroll
        for (int t = 0; t < 3; t++) xi[t] = x[(size_t)t * HW + p];
        affine_pre(xi, w, bb, yp);
#pragma unroll
        for (int c = 0; c < 3; c++)
        {
            const float go = gy[(size_t)c * HW + p];
            g[c] = (yp[c] >= 0.0f && yp[c] <= 1.0f) ? go : 0.0f;
        }
#pragma unroll
        for (int t = 0; t < 3; t++)
        {
            gx[(size_t)t * HW + p] = (g[0] * w[3 * t] + g[1] * w[3 * t + 1]) + g[2] * w[3 * t + 2];
#pragma unroll
            for (int c = 0; c < 3; c++) acc[3 * t + c] += (double)xi[t] * (double)g[c]; // exact products
        }
#pragma unroll
        for (int c = 0; c < 3; c++) acc[9 + c] += (double)g[c];
    }
#pragma unroll
    for (int t = 0; t < AFF_PARTS; t++)
    {
        const double s = block_sum(acc[t], red);
        if (threadIdx.x == 0) partial[t * SUM_BLOCKS + blockIdx.x] = s;
    }
}
__global__ void __launch_bounds__(64) affine_finish_kernel(int nblocks, const double *__restrict__ partial, float *__restrict__ dW, float *__restrict__ db)
{
    double s[AFF_PARTS];
#pragma unroll
    for (int t = 0; t < AFF_PARTS; t++) s[t] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 64)
#pragma unroll
        for (int t = 0; t < AFF_PARTS; t++) s[t] += partial[t * SUM_BLOCKS + b];
#pragma unroll
    for (int t = 0; t < AFF_PARTS; t++)
        for (int o = 32; o > 0; o >>= 1) s[t] += __shfl_xor(s[t], o);
    if (threadIdx.x == 0)
    {
        for (int t = 0; t < 9; t++) dW[t] = (float)s[t];
        for (int c = 0; c < 3; c++) db[c] = (float)s[9 + c];
    }
}
} // namespace

size_t ts_reg_workspace_bytes() { return ts_align_up((size_t)AFF_PARTS * SUM_BLOCKS * sizeof(double)) + TS_ALIGN; }
size_t ts_reg_prepared_bytes(int P) { return P > 0 ? prep_carve(nullptr, P).bytes : TS_ALIGN; }

hipError_t ts_reg_prepare(int P, const uint32_t *nearest, void *prepared, hipStream_t s)
{
    if (P <= 0) return hipSuccess;
    const PrepCarve c = prep_carve(prepared, P);
    const uint32_t n = 3u * (uint32_t)P;
    int end_bit = 1;
    while (end_bit < 32 && (n >> end_bit) != 0u) end_bit++; // keys lie in [0, n]
    hipLaunchKernelGGL(inv_keys_kernel, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, s, n, nearest, c.k[0], c.v[0]);
    const int at = ts_radix_sort_pairs(c.k, c.v, n, end_bit, c.sort_scratch, s); // stable: the sources of one target stay in ascending order
    hipLaunchKernelGGL(inv_offsets_kernel, dim3((n + 1 + TPB - 1) / TPB), dim3(TPB), 0, s, n, c.k[at], c.v[at], c.inv, c.off);
    return hipGetLastError();
}

hipError_t ts_reg_forward(int P, const float *vertex, const float *opacity, const uint32_t *nearest, float w_s, float w_o, int omode, float w_v,
                          void *workspace, float *out, hipStream_t s)
{
    double *partial = (double *)ts_align_up((size_t)workspace);
    const int do_s = w_s != 0.0f, om = w_o != 0.0f ? omode : TSL_REG_OPACITY_NONE, do_v = w_v != 0.0f;
    const int nb = P > 0 ? min(SUM_BLOCKS, (P + TPB - 1) / TPB) : 1;
    hipLaunchKernelGGL(reg_sum_kernel, dim3((unsigned)nb), dim3(TPB), 0, s, P, vertex, opacity, nearest, do_s, om, do_v, partial);
    hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(64), 0, s, nb, P, w_s, w_o, w_v, do_s, om, do_v, partial, out);
    return hipGetLastError();
}

hipError_t ts_reg_backward(int P, const float *vertex, const float *opacity, const uint32_t *nearest, const void *prepared, float w_s, float w_o,
                           int omode, float w_v, const float *grad_out, float *dvertex, float *dopacity, hipStream_t s)
{
    if (P <= 0) return hipSuccess;
    const int do_s = w_s != 0.0f, om = w_o != 0.0f ? omode : TSL_REG_OPACITY_NONE, do_v = w_v != 0.0f;
    const PrepCarve c = prep_carve(const_cast<void *>(prepared), do_v ? P : 0);
    RegCoef k;
    k.cs = (float)((double)w_s / (3.0 * P));
    k.co = (float)((double)w_o / P);
    k.cv = (float)(2.0 * (double)w_v / (3.0 * P));
    hipLaunchKernelGGL(reg_bwd_kernel, dim3((unsigned)((P + TPB - 1) / TPB)), dim3(TPB), 0, s, P, vertex, opacity, do_v ? nearest : nullptr,
                       do_v ? c.inv : nullptr, do_v ? c.off : nullptr, k, do_s, om, do_v, grad_out, dvertex, dopacity);
    return hipGetLastError();
}

hipError_t ts_color_affine_forward(const float *x, int H, int W, const float *Wm, const float *b, float *y, hipStream_t s)
{
    const int HW = H * W;
    hipLaunchKernelGGL(affine_fwd_kernel, dim3((unsigned)((HW + TPB - 1) / TPB)), dim3(TPB), 0, s, HW, x, Wm, b, y);
    return hipGetLastError();
}

hipError_t ts_color_affine_backward(const float *x, int H, int W, const float *Wm, const float *b, const float *gy, void *workspace, float *gx,
                                    float *dW, float *db, hipStream_t s)
{
    const int HW = H * W, nb = min(SUM_BLOCKS, (HW + TPB - 1) / TPB);
    double *partial = (double *)ts_align_up((size_t)workspace);
    hipLaunchKernelGGL(affine_bwd_kernel, dim3((unsigned)nb), dim3(TPB), 0, s, HW, x, Wm, b, gy, gx, partial);
    hipLaunchKernelGGL(affine_finish_kernel, dim3(1), dim3(64), 0, s, nb, partial, dW, db);
    return hipGetLastError();
}
