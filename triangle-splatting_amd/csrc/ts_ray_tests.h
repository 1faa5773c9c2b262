// ts_ray_tests.h -- the two tests of a ray that include/ts_ray.h defines, as device functions: the padded slab interval of a box and the
// watertight triangle test (Woop, Benthin and Wald), float64 on the fp32 coordinates.  Shared by mesh_ray.hip (the first hit) and
// mesh_inside.hip (all hits, include/ts_inside.h): one text, so that a face is hit in the one unit exactly when it is hit in the other.
// With them, for the same reason, the rule for which rays are cast at all (ray_direction_valid, ray_valid).
// Every translation unit that includes it gets its own internal copy and must be built with -ffp-contract=off: every operation below rounds.
#pragma once
#include "ts2d_common.h"

#include <cfloat>

namespace
{
// min and max of the header: of two equal values (+0 and -0) the first stays
__device__ __forceinline__ double min2(double x, double y) { return y < x ? y : x; }
__device__ __forceinline__ double max2(double x, double y) { return y > x ? y : x; }

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= FLT_MAX; }

// one axis of the slab interval: false when the direction is zero and the origin lies outside [lo, hi]
__device__ __forceinline__ bool slab_axis(double lo, double hi, double o, double d, double &tn, double &tf)
{
    if (d == 0.0) return lo <= o && o <= hi; // contributes (-inf, +inf)
    const double ta = (lo - o) / d, tb = (hi - o) / d;
    const double near = min2(ta, tb), far = max2(ta, tb);
    const double near_p = near - fabs(near) * 0x1p-40, far_p = far + fabs(far) * 0x1p-40;
    tn = max2(tn, near_p);
    tf = min2(tf, far_p);
    return true;
}

// the slab interval of the header: false when a zero-direction axis fails or tn > tf; tmin and the upper limit are the caller's
__device__ __forceinline__ bool slab(double ox, double oy, double oz, double dx, double dy, double dz, float mnx, float mny, float mnz, float mxx,
                                     float mxy, float mxz, double &tn, double &tf)
{
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    tn = -inf; tf = inf; // max2(-inf, x) = x and min2(+inf, x) = x, bit for bit: a zero axis, and this start, contribute nothing
    bool ok = slab_axis((double)mnx, (double)mxx, ox, dx, tn, tf);
    ok &= slab_axis((double)mny, (double)mxy, oy, dy, tn, tf);
    ok &= slab_axis((double)mnz, (double)mxz, oz, dz, tn, tf);
    return ok && tn <= tf;
}

// the slab interval of AABB(T), the per-axis minimum and maximum of the three fp32 vertices
__device__ __forceinline__ bool face_slab(double ox, double oy, double oz, double dx, double dy, double dz, float ax, float ay, float az, float bx,
                                          float by, float bz, float cx, float cy, float cz, double &tn, double &tf)
{
    return slab(ox, oy, oz, dx, dy, dz, fminf(fminf(ax, bx), cx), fminf(fminf(ay, by), cy), fminf(fminf(az, bz), cz), fmaxf(fmaxf(ax, bx), cx),
                fmaxf(fmaxf(ay, by), cy), fmaxf(fmaxf(az, bz), cz), tn, tf);
}

__device__ __forceinline__ double sel3(int k, double x, double y, double z) { return k == 0 ? x : (k == 1 ? y : z); }
__device__ __forceinline__ float sel3f(int k, float x, float y, float z) { return k == 0 ? x : (k == 1 ? y : z); }

// the dominant axis and the shear of the watertight test, once per ray, with the origin's components in that order
struct RayShear
{
    int kx, ky, kz;
    double Sx, Sy, Sz, okx, oky, okz;
};

__device__ __forceinline__ RayShear ray_shear(double ox, double oy, double oz, double dx, double dy, double dz)
{
    RayShear r;
    int kz = 0;
    if (fabs(dy) > fabs(dx)) kz = 1;
    if (fabs(dz) > fabs(kz ? dy : dx)) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const double dkz = sel3(kz, dx, dy, dz);
    if (dkz < 0.0)
    {
        const int s = kx; kx = ky; ky = s;
    }
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.Sx = sel3(kx, dx, dy, dz) / dkz; r.Sy = sel3(ky, dx, dy, dz) / dkz; r.Sz = 1.0 / dkz;
    r.okx = sel3(kx, ox, oy, oz); r.oky = sel3(ky, ox, oy, oz); r.okz = sel3(kz, ox, oy, oz);
    return r;
}

// the rays that are cast at all (include/ts_ray.h): a finite origin, a finite non-zero direction, a limit that is not NaN
__device__ __forceinline__ bool ray_direction_valid(float dx, float dy, float dz)
{
    return finite_f(dx) && finite_f(dy) && finite_f(dz) && !(dx == 0.0f && dy == 0.0f && dz == 0.0f);
}

__device__ __forceinline__ bool ray_valid(bool origin_finite, float dx, float dy, float dz, const float *__restrict__ t_limit, size_t i)
{
    return origin_finite && ray_direction_valid(dx, dy, dz) && !(t_limit && t_limit[i] != t_limit[i]);
}

// U, V, W, det of the face (a, b, c) and the three sheared depths' sources A[kz] - o[kz], ...: what face_t needs besides
struct FaceEdges
{
    double U, V, W, det, Akz, Bkz, Ckz;
};

__device__ __forceinline__ FaceEdges face_edges(const RayShear &r, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy,
                                                float cz)
{
    FaceEdges e;
    e.Akz = (double)sel3f(r.kz, ax, ay, az) - r.okz; e.Bkz = (double)sel3f(r.kz, bx, by, bz) - r.okz; e.Ckz = (double)sel3f(r.kz, cx, cy, cz) - r.okz;
    const double Ax = ((double)sel3f(r.kx, ax, ay, az) - r.okx) - r.Sx * e.Akz, Ay = ((double)sel3f(r.ky, ax, ay, az) - r.oky) - r.Sy * e.Akz;
    const double Bx = ((double)sel3f(r.kx, bx, by, bz) - r.okx) - r.Sx * e.Bkz, By = ((double)sel3f(r.ky, bx, by, bz) - r.oky) - r.Sy * e.Bkz;
    const double Cx = ((double)sel3f(r.kx, cx, cy, cz) - r.okx) - r.Sx * e.Ckz, Cy = ((double)sel3f(r.ky, cx, cy, cz) - r.oky) - r.Sy * e.Ckz;
    e.U = Cx * By - Cy * Bx; e.V = Ax * Cy - Ay * Cx; e.W = Bx * Ay - By * Ax;
    e.det = (e.U + e.V) + e.W;
    return e;
}

// a CANDIDATE without culling: det != 0 and U, V, W not of both signs
__device__ __forceinline__ bool face_candidate(const FaceEdges &e)
{
    const bool neg = e.U < 0.0 || e.V < 0.0 || e.W < 0.0, pos = e.U > 0.0 || e.V > 0.0 || e.W > 0.0;
    return !(e.det == 0.0 || (neg && pos));
}

// tt of a candidate
__device__ __forceinline__ double face_t(const RayShear &r, const FaceEdges &e)
{
    const double Az = r.Sz * e.Akz, Bz = r.Sz * e.Bkz, Cz = r.Sz * e.Ckz;
    return ((e.U * Az + e.V * Bz) + e.W * Cz) / e.det;
}
} // namespace
