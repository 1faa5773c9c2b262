// mesh_winding.hip -- the generalised winding number of a mesh at a point, summed on the index that mesh_bvh.hip's build wrote
// (csrc/ts_bvh_layout.h) with one far-field term per node, and the signed distance that follows (include/ts_winding.h).
//
// Built with -ffp-contract=off: the face term, the node term, the accept test and the moments round every operation (the header's text).
// Every term is quantised to an integer before it is summed, so a lane's sum is a pure function of WHICH terms it takes, and that is
// decided per lane by the accept test alone: neither the order of the walk nor the company in the wave changes a result.
//
// Moments.  One launch per level, bottom-up, writes [N, M, -, S] per node (a leaf from its slots, an inner node from its children, both in
// index order), then one launch over all nodes turns M into p = M / S and writes R2 from the node's box.  No atomics, no workspace.
//
// Query.  The points go through the front half of the box searches (ts_knn_front.h): the bounding box of the finite points, a Morton sort,
// a float4 gather that carries the original index; a non-finite point is stored as NaNs.  The walk is csrc/ts_bvh_walk.h, children in index
// order.  What is this kernel's own: every lane keeps an int64 sum and two int32 counters; at a popped node, whose moment record is a
// wave-uniform load, every lane that has not accepted an ancestor tests d2 > beta2 * R2 and either takes the node's term or asks for more;
// the node is entered when some lane asks.  A lane that accepted node (L, K) sits out of every popped (l, k) with l < L and
// k >> 3 (L - l) == K: the walk is depth first, so those are popped before anything else and one register pair is enough.  At a leaf every
// asking lane evaluates the face term.
#include "ts_bvh_layout.h"
#include "ts_bvh_walk.h"
#include "ts_ray_tests.h" // max2, finite_f
#include "ts_winding_launch.h"

namespace
{
constexpr double PI = 3.141592653589793;        // 0x400921FB54442D18
constexpr double UNITS_HALF = 137438953472.0;   // 2^37
constexpr double UNITS_TURN = 274877906944.0;   // 2^38
constexpr long long BAD_QUERY = (long long)0x8000000000000000ull; // INT64_MIN

struct Moment
{
    double nx, ny, nz, px, py, pz, r2, s; // px..pz hold M until finish_moments_kernel has run
};

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

// ---- moments -------------------------------------------------------------------------------------------------------------------------
// one lane per leaf: N, S and M over its slots in slot order, and the slots' face ids for whoever restates the tree
__global__ void __launch_bounds__(256) leaf_moments_kernel(int nleaves, const Leaf *__restrict__ leaves, Moment *__restrict__ mom,
                                                            int32_t *__restrict__ leaf_faces)
{
    const int leaf = blockIdx.x * 256 + threadIdx.x;
    if (leaf >= nleaves) return;
    const Leaf &lf = leaves[leaf];
    Moment m = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < LEAF; j++)
    {
        const int32_t id = lf.id[j];
        if (leaf_faces) leaf_faces[(size_t)leaf * LEAF + j] = id;
        if (id < 0) continue;
        const double ax = lf.v[j][0], ay = lf.v[j][1], az = lf.v[j][2], bx = lf.v[j][3], by = lf.v[j][4], bz = lf.v[j][5], cx = lf.v[j][6],
                     cy = lf.v[j][7], cz = lf.v[j][8];
        const double ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
        const double nx = 0.5 * (uy * vz - uz * vy), ny = 0.5 * (uz * vx - ux * vz), nz = 0.5 * (ux * vy - uy * vx);
        const double ar = sqrt(dot3(nx, ny, nz, nx, ny, nz));
        const double gx = ((ax + bx) + cx) / 3.0, gy = ((ay + by) + cy) / 3.0, gz = ((az + bz) + cz) / 3.0;
        m.nx += nx; m.ny += ny; m.nz += nz;
        m.s += ar;
        m.px += ar * gx; m.py += ar * gy; m.pz += ar * gz;
    }
    mom[leaf] = m;
}

// one lane per node of a level: the sums of its (up to FAN) children of the level below, in index order
__global__ void __launch_bounds__(256) inner_moments_kernel(int count, int count_below, const Moment *__restrict__ below, Moment *__restrict__ level)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    Moment m = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int c0 = k * FAN, c1 = min(count_below - c0, FAN); // k < count = ceil(count_below / FAN): c0 < count_below, no overflow
    for (int c = 0; c < c1; c++)
    {
        const Moment b = below[c0 + c];
        m.nx += b.nx; m.ny += b.ny; m.nz += b.nz;
        m.s += b.s;
        m.px += b.px; m.py += b.py; m.pz += b.pz;
    }
    level[k] = m;
}

// one lane per node of any level, after all sums: the centre p = M / S and the squared radius about it that holds the node's box
__global__ void __launch_bounds__(256) finish_moments_kernel(int total, const Box *__restrict__ nodes, Moment *__restrict__ mom)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    Moment m = mom[i];
    if (m.s > 0.0)
    {
        const Box b = nodes[i];
        m.px = m.px / m.s; m.py = m.py / m.s; m.pz = m.pz / m.s;
        const double ex = max2(m.px - (double)b.mnx, (double)b.mxx - m.px), ey = max2(m.py - (double)b.mny, (double)b.mxy - m.py),
                     ez = max2(m.pz - (double)b.mnz, (double)b.mxz - m.pz);
        m.r2 = dot3(ex, ey, ez, ex, ey, ez);
    }
    else
    {
        m.px = 0.0; m.py = 0.0; m.pz = 0.0;
        m.r2 = __longlong_as_double(0x7FF0000000000000ll);
    }
    mom[i] = m;
}

// ---- query ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long face_term(double qx, double qy, double qz, float Ax, float Ay, float Az, float Bx, float By, float Bz, float Cx,
                                               float Cy, float Cz)
{
    const double ax = (double)Ax - qx, ay = (double)Ay - qy, az = (double)Az - qz, bx = (double)Bx - qx, by = (double)By - qy, bz = (double)Bz - qz,
                 cx = (double)Cx - qx, cy = (double)Cy - qy, cz = (double)Cz - qz;
    const double la = sqrt(dot3(ax, ay, az, ax, ay, az)), lb = sqrt(dot3(bx, by, bz, bx, by, bz)), lc = sqrt(dot3(cx, cy, cz, cx, cy, cz));
    const double det = dot3(ax, ay, az, by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx);
    const double den = ((la * lb) * lc + dot3(ax, ay, az, bx, by, bz) * lc) + (dot3(bx, by, bz, cx, cy, cz) * la + dot3(cx, cy, cz, ax, ay, az) * lb);
    const double theta = det == 0.0 ? 0.0 : atan2(det, den);
    return llrint((theta / PI) * UNITS_HALF);
}

__global__ void __launch_bounds__(TPB) winding_kernel(int Q, int nleaves, int nlevels, const float4 *__restrict__ qsp, double beta2,
                                                       const Leaf *__restrict__ leaves, const Box *__restrict__ nodes,
                                                       const Moment *__restrict__ mom, long long *__restrict__ wq, int32_t *__restrict__ terms)
{
    __shared__ WalkShared ws;
    walk_levels(ws, nleaves);
    const WalkQuery q = walk_query(Q, qsp);
    // a lane that is not live walks along with a finite stand-in and never takes a term
    const double qx = q.live ? (double)q.p.x : 0.0, qy = q.live ? (double)q.p.y : 0.0, qz = q.live ? (double)q.p.z : 0.0;

    long long sum = 0;
    int nfaces = 0, nnodes = 0;
    int acc_level = 0;   // the node this lane accepted last: no popped node lies below level 0, so (0, 0) stands for none
    uint32_t acc_k = 0;
    bool ask = false;    // of the node at hand: this lane wants its children, or its faces

    if (__ballot(q.live) != 0ull) // wave-uniform
        bvh_walk<false>(
            ws, nlevels, nodes,
            [&](int level, uint32_t k, uint32_t at, const Box &) {
                const Moment m = mom[at];
                ask = q.live && !(level < acc_level && (k >> (FAN_SHIFT * (acc_level - level))) == acc_k);
                if (ask && m.s > 0.0)
                {
                    const double rx = m.px - qx, ry = m.py - qy, rz = m.pz - qz;
                    const double d2 = dot3(rx, ry, rz, rx, ry, rz);
                    if (d2 > beta2 * m.r2)
                    {
                        sum += llrint(((dot3(m.nx, m.ny, m.nz, rx, ry, rz) / (d2 * sqrt(d2))) / (4.0 * PI)) * UNITS_TURN);
                        nnodes++;
                        acc_level = level; acc_k = k;
                        ask = false;
                    }
                }
                return __ballot(ask) != 0ull;
            },
            [&](int leaf) {
                for_each_face(leaves[leaf], [&](int32_t, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
                    if (!ask) return;
                    sum += face_term(qx, qy, qz, ax, ay, az, bx, by, bz, cx, cy, cz);
                    nfaces++;
                });
            },
            NoChildKey());

    if (q.inside)
    {
        wq[q.pid] = q.live ? sum : BAD_QUERY;
        if (terms)
        {
            terms[2 * (size_t)q.pid] = q.live ? nfaces : -1;
            terms[2 * (size_t)q.pid + 1] = q.live ? nnodes : -1;
        }
    }
}

// F == 0: nothing winds around anything
__global__ void __launch_bounds__(256) no_faces_kernel(int Q, const float *__restrict__ points, long long *__restrict__ wq, int32_t *__restrict__ terms)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    const bool good = all_finite(points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]);
    wq[i] = good ? 0 : BAD_QUERY;
    if (terms)
    {
        terms[2 * (size_t)i] = good ? 0 : -1;
        terms[2 * (size_t)i + 1] = good ? 0 : -1;
    }
}

__global__ void __launch_bounds__(256) sign_distance_kernel(int Q, const double *__restrict__ dist2, const long long *__restrict__ wq,
                                                             long long threshold, float *__restrict__ out, uint8_t *__restrict__ decided)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    const double d2 = dist2[i];
    const long long w = wq[i];
    float o;
    uint8_t dec;
    if (d2 == 0.0)
    {
        o = 0.0f; dec = 1;
    }
    else if (!(d2 < __longlong_as_double(0x7FF0000000000000ll)) || w == BAD_QUERY) // NaN or +inf, or a bad point
    {
        o = __uint_as_float(0x7FC00000u); dec = 0;
    }
    else
    {
        const float r = (float)sqrt(d2);
        o = w >= threshold ? -r : r;
        dec = 1;
    }
    out[i] = o;
    decided[i] = dec;
}
} // namespace

size_t ts_winding_bvh_bytes(int F) { return bvh_view(nullptr, F).bytes; }

size_t ts_winding_moments_bytes(int F)
{
    const BvhView b = bvh_view(nullptr, F);
    return b.nlevels ? (b.offset[b.nlevels - 1] + (size_t)b.count[b.nlevels - 1]) * sizeof(Moment) : 0;
}

size_t ts_winding_leaf_faces_bytes(int F) { return (size_t)bvh_view(nullptr, F).nleaves * LEAF * sizeof(int32_t); }

size_t ts_winding_workspace_bytes(int Q) { return query_carve_bytes(Q) + TS_ALIGN; }

hipError_t ts_winding_moments(int F, const void *bvh, double *moments, int32_t *leaf_faces, hipStream_t s)
{
    if (F <= 0) return hipSuccess;
    const BvhView b = bvh_view(const_cast<void *>(bvh), F);
    Moment *mom = (Moment *)moments;
    hipLaunchKernelGGL(leaf_moments_kernel, dim3((unsigned)((b.nleaves + 255) / 256)), dim3(256), 0, s, b.nleaves, b.leaves, mom, leaf_faces);
    for (int l = 1; l < b.nlevels; l++)
        hipLaunchKernelGGL(inner_moments_kernel, dim3((unsigned)((b.count[l] + 255) / 256)), dim3(256), 0, s, b.count[l], b.count[l - 1],
                           mom + b.offset[l - 1], mom + b.offset[l]);
    const int total = (int)(b.offset[b.nlevels - 1] + (size_t)b.count[b.nlevels - 1]); // below 2^28 * 8 / 7
    hipLaunchKernelGGL(finish_moments_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, total, b.nodes, mom);
    return hipGetLastError();
}

hipError_t ts_winding_query(int Q, const float *points, double beta2, int F, const void *bvh, const double *moments, int64_t *wq, int32_t *terms,
                            void *ws, hipStream_t s)
{
    if (Q <= 0) return hipSuccess;
    if (F <= 0)
    {
        hipLaunchKernelGGL(no_faces_kernel, dim3((unsigned)(((size_t)Q + 255) / 256)), dim3(256), 0, s, Q, points, (long long *)wq, terms);
        return hipGetLastError();
    }
    const BvhView b = bvh_view(const_cast<void *>(bvh), F);
    const KnnCarve cq = knn_carve((void *)ts_align_up((size_t)ws), Q);
    const hipError_t e = knn_prepare<true>(Q, points, cq, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(winding_kernel, dim3((unsigned)(((size_t)Q + TPB - 1) / TPB)), dim3(TPB), 0, s, Q, b.nleaves, b.nlevels, cq.sp, beta2, b.leaves,
                       b.nodes, (const Moment *)moments, (long long *)wq, terms);
    return hipGetLastError();
}

hipError_t ts_winding_sign_distance(int Q, const double *dist2, const int64_t *wq, int64_t threshold, float *out, uint8_t *decided, hipStream_t s)
{
    if (Q <= 0) return hipSuccess;
    hipLaunchKernelGGL(sign_distance_kernel, dim3((unsigned)(((size_t)Q + 255) / 256)), dim3(256), 0, s, Q, dist2, (const long long *)wq,
                       (long long)threshold, out, decided);
    return hipGetLastError();
}
