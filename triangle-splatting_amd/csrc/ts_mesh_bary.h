// ts_mesh_bary.h -- the perspective-correct barycentrics of a pixel-centre ray on a face of an indexed mesh, held inside the face
// (include/ts_color.h, "Interpolation of vertex attributes"): the ONE statement of them.  color_volume.hip (tsc_interpolate) and mesh_atlas.hip
// (tsa_texel_index) include it, so the texel of a pixel is by construction the texel of tsc_interpolate's `bary`.
//
// Both units are built with -ffp-contract=off: every float64 operation below rounds.  Everything is float64 on the fp32 inputs widened.
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// r dot (x cross y), r = (r0, r1, 1)
__device__ __forceinline__ double ray_dot_cross(double r0, double r1, const double x[3], const double y[3])
{
    const double n0 = x[1] * y[2] - x[2] * y[1], n1 = x[2] * y[0] - x[0] * y[2], n2 = x[0] * y[1] - x[1] * y[0];
    return (r0 * n0 + r1 * n1) + n2;
}

// v = [p, 1] @ view, row-vector convention
__device__ __forceinline__ void to_view(const float *__restrict__ view, const float *__restrict__ p, double v[3])
{
    const double p0 = (double)p[0], p1 = (double)p[1], p2 = (double)p[2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        v[k] = ((p0 * (double)view[k] + p1 * (double)view[4 + k]) + p2 * (double)view[8 + k]) + (double)view[12 + k];
}

// DRAWN: f lies in [0, F) and the three indices of its row of `faces` lie in [0, V).  Nothing is read out of bounds for any f or any row.
__device__ __forceinline__ bool drawn_face(int f, int F, int V, const int32_t *__restrict__ faces, int &ia, int &ib, int &ic)
{
    ia = ib = ic = -1;
    if (f >= 0 && f < F)
    {
        ia = faces[3 * (size_t)f];
        ib = faces[3 * (size_t)f + 1];
        ic = faces[3 * (size_t)f + 2];
    }
    return ia >= 0 && ia < V && ib >= 0 && ib < V && ic >= 0 && ic < V;
}

// (alpha, beta, gamma) of pixel (col, row) on the drawn face (ia, ib, ic): the view-space corners, the pixel-centre ray, the three weights,
// the sign flip, the clamp of negative or NaN weights, s' and the quotients, or 1.0 / 3.0 each where s' is not finite and > 0.
__device__ __forceinline__ void pixel_barycentrics(const float *__restrict__ view, float tan_fovx, float tan_fovy, int W, int H, int col, int row,
                                                   const float *__restrict__ vertices, int ia, int ib, int ic, double &alpha, double &beta,
                                                   double &gamma)
{
    double a[3], b[3], c[3];
    to_view(view, vertices + 3 * (size_t)ia, a);
    to_view(view, vertices + 3 * (size_t)ib, b);
    to_view(view, vertices + 3 * (size_t)ic, c);
    const double r0 = (((double)col + 0.5) / (0.5 * (double)W) - 1.0) * (double)tan_fovx;
    const double r1 = (((double)row + 0.5) / (0.5 * (double)H) - 1.0) * (double)tan_fovy;
    double wa = ray_dot_cross(r0, r1, b, c), wb = ray_dot_cross(r0, r1, c, a), wc = ray_dot_cross(r0, r1, a, b);
    if ((wa + wb) + wc < 0.0)
    {
        wa = -wa;
        wb = -wb;
        wc = -wc;
    }
    wa = wa >= 0.0 ? wa : 0.0; // negative or NaN
    wb = wb >= 0.0 ? wb : 0.0;
    wc = wc >= 0.0 ? wc : 0.0;
    const double s = (wa + wb) + wc;
    alpha = 1.0 / 3.0, beta = 1.0 / 3.0, gamma = 1.0 / 3.0;
    if (fabs(s) <= DBL_MAX && s > 0.0) // finite
    {
        alpha = wa / s;
        beta = wb / s;
        gamma = wc / s;
    }
}
