// mesh_inside.hip -- all hits of a ray on the triangles of a mesh, counted in half crossings, and the signed distance that follows
// (include/ts_inside.h), on the index that mesh_bvh.hip's build wrote (csrc/ts_bvh_layout.h).
//
// Built with -ffp-contract=off: the slab interval and the watertight triangle test round every operation.  Both are csrc/ts_ray_tests.h, the
// text that mesh_ray.hip evaluates a ray with: a face is hit here exactly when it is hit there.
//
// The rays go through the front half of the box searches (ts_knn_front.h) like those of mesh_ray.hip, keyed on the ORIGINS; the direction
// and the per-ray limit are read through the original index; with SHARED the direction is three wave-uniform loads and the dominant axis
// and the shear live in scalar registers.
//
// The walk is csrc/ts_bvh_walk.h, children in index order.  What is this kernel's own: every lane keeps three int32 counters; a node is
// entered when some live lane crosses its box with tf >= tmin and tn <= hi.  There is no nearest hit: nothing to prune on, so no child
// ordering and no mean ray.  At a leaf every lane tests the face's own box first, then the triangle, and counts.  The sums are integers:
// the order of the walk does not matter.
#include "ts_bvh_layout.h"
#include "ts_bvh_walk.h"
#include "ts_inside_launch.h"
#include "ts_ray_tests.h"

namespace
{
template <bool SHARED>
__global__ void __launch_bounds__(TPB) crossings_kernel(int Q, int nleaves, int nlevels, const float4 *__restrict__ osp,
                                                         const float *__restrict__ directions, const float *__restrict__ t_limit, double tmin,
                                                         double tmax, const Leaf *__restrict__ leaves, const Box *__restrict__ nodes,
                                                         int32_t *__restrict__ hits_out, int32_t *__restrict__ winding2_out,
                                                         int32_t *__restrict__ touches_out, unsigned long long *leaf_visits)
{
    __shared__ WalkShared ws;
    walk_levels(ws, nleaves);
    const WalkQuery q = walk_query(Q, osp);
    float fdx, fdy, fdz;
    if (SHARED) // three scalar loads: a bad shared direction makes every ray bad
    {
        fdx = directions[0]; fdy = directions[1]; fdz = directions[2];
    }
    else
    {
        const size_t at = q.live ? 3 * (size_t)q.pid : 0; // Q >= 1: the first ray's direction is there to read
        fdx = directions[at]; fdy = directions[at + 1]; fdz = directions[at + 2];
    }
    const bool good_d = ray_direction_valid(fdx, fdy, fdz); // SHARED: wave-uniform
    bool live = q.live && good_d;
    double hi = tmax;
    if (live && t_limit)
    {
        const float tl = t_limit[q.pid];
        if (tl != tl) live = false;
        else hi = min2(tmax, (double)tl);
    }
    // a lane that is not live walks along with finite stand-ins and never counts; the direction's stand-in depends on the direction alone
    const double ox = live ? (double)q.p.x : 0.0, oy = live ? (double)q.p.y : 0.0, oz = live ? (double)q.p.z : 0.0;
    const double dx = good_d ? (double)fdx : 1.0, dy = good_d ? (double)fdy : 0.0, dz = good_d ? (double)fdz : 0.0;
    const RayShear sh = ray_shear(ox, oy, oz, dx, dy, dz); // with SHARED the axes and the shear are wave-uniform, the origin's part is not

    int hits = 0, winding2 = 0, touches = 0;
    unsigned visits = 0;

    if (__ballot(live) != 0ull) // wave-uniform
        bvh_walk<false>(
            ws, nlevels, nodes,
            [&](int, uint32_t, uint32_t, const Box &b) {
                double tn, tf;
                const bool crossed = slab(ox, oy, oz, dx, dy, dz, b.mnx, b.mny, b.mnz, b.mxx, b.mxy, b.mxz, tn, tf);
                return __ballot(live && crossed && tf >= tmin && !(tn > hi)) != 0ull;
            },
            [&](int leaf) {
                visits++;
                for_each_face(leaves[leaf], [&](int32_t, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
                    double tn, tf;
                    const bool crossed = face_slab(ox, oy, oz, dx, dy, dz, ax, ay, az, bx, by, bz, cx, cy, cz, tn, tf);
                    if (!live || !crossed || !(tf >= tmin) || tn > hi) return;
                    const FaceEdges e = face_edges(sh, ax, ay, az, bx, by, bz, cx, cy, cz);
                    if (!face_candidate(e)) return;
                    const double tp = max2(face_t(sh, e), tn);
                    if (!(tp >= tmin && tp <= hi)) return;
                    const int z = (e.U == 0.0) + (e.V == 0.0) + (e.W == 0.0); // at most 2: det != 0
                    const int s = e.det > 0.0 ? 1 : -1;
                    hits++;
                    winding2 += z == 0 ? 2 * s : (z == 1 ? s : 0);
                    touches += z >= 2;
                });
            },
            NoChildKey());

    if (q.inside)
    {
        hits_out[q.pid] = live ? hits : -1;
        winding2_out[q.pid] = winding2;
        touches_out[q.pid] = touches;
    }
    if (leaf_visits && (threadIdx.x & 63) == 0 && visits) atomicAdd(leaf_visits, (unsigned long long)visits);
}

// F == 0: nobody hits anything
__global__ void __launch_bounds__(256) no_faces_kernel(int Q, const float *__restrict__ origins, const float *__restrict__ directions, int dstride,
                                                        const float *__restrict__ t_limit, int32_t *__restrict__ hits, int32_t *__restrict__ winding2,
                                                        int32_t *__restrict__ touches)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    const size_t at = (size_t)dstride * (size_t)i;
    const float dx = directions[at], dy = directions[at + 1], dz = directions[at + 2];
    const bool good = ray_valid(all_finite(origins[3 * (size_t)i], origins[3 * (size_t)i + 1], origins[3 * (size_t)i + 2]), dx, dy, dz, t_limit, i);
    hits[i] = good ? 0 : -1;
    winding2[i] = 0;
    touches[i] = 0;
}

__global__ void __launch_bounds__(256) signed_distance_kernel(int Q, const double *__restrict__ dist2, const int32_t *__restrict__ winding2,
                                                               const int32_t *__restrict__ touches, const int32_t *__restrict__ hits, int rule,
                                                               int only_undecided, float *out, uint8_t *decided)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    if (only_undecided && decided[i] != 0) return;
    const double d2 = dist2[i];
    float o;
    uint8_t dec;
    if (d2 == 0.0)
    {
        o = 0.0f; dec = 1;
    }
    else if (!(d2 < __longlong_as_double(0x7FF0000000000000ll))) // NaN or +inf
    {
        o = __uint_as_float(0x7FC00000u); dec = 0;
    }
    else
    {
        const int w2 = winding2[i];
        const bool clean = hits[i] >= 0 && touches[i] == 0 && (w2 & 1) == 0;
        const int w = -(w2 / 2); // exact for an even w2
        const bool in = rule == 0 ? w != 0 : (rule == 1 ? (w & 1) != 0 : w > 0);
        const float r = (float)sqrt(d2);
        o = clean && in ? -r : r;
        dec = clean ? 1 : 0;
    }
    out[i] = o;
    decided[i] = dec;
}
} // namespace

size_t ts_inside_bvh_bytes(int F) { return bvh_view(nullptr, F).bytes; }

size_t ts_inside_crossings_workspace_bytes(int Q) { return query_carve_bytes(Q) + TS_ALIGN; }

hipError_t ts_inside_crossings(int Q, const float *origins, const float *directions, int shared_direction, const float *t_limit, double tmin,
                               double tmax, int F, const void *bvh, int32_t *hits, int32_t *winding2, int32_t *touches,
                               unsigned long long *leaf_visits, void *ws, hipStream_t s)
{
    if (Q <= 0) return hipSuccess;
    if (F <= 0)
    {
        hipLaunchKernelGGL(no_faces_kernel, dim3((unsigned)(((size_t)Q + 255) / 256)), dim3(256), 0, s, Q, origins, directions, shared_direction ? 0 : 3, t_limit, hits, winding2,
                           touches);
        return hipGetLastError();
    }
    const BvhView b = bvh_view(const_cast<void *>(bvh), F);
    const KnnCarve cq = knn_carve((void *)ts_align_up((size_t)ws), Q);
    const hipError_t e = knn_prepare<true>(Q, origins, cq, s);
    if (e != hipSuccess) return e;
    const unsigned qblocks = (unsigned)(((size_t)Q + TPB - 1) / TPB);
    if (shared_direction)
        hipLaunchKernelGGL(crossings_kernel<true>, dim3(qblocks), dim3(TPB), 0, s, Q, b.nleaves, b.nlevels, cq.sp, directions, t_limit, tmin, tmax,
                           b.leaves, b.nodes, hits, winding2, touches, leaf_visits);
    else
        hipLaunchKernelGGL(crossings_kernel<false>, dim3(qblocks), dim3(TPB), 0, s, Q, b.nleaves, b.nlevels, cq.sp, directions, t_limit, tmin, tmax,
                           b.leaves, b.nodes, hits, winding2, touches, leaf_visits);
    return hipGetLastError();
}

hipError_t ts_inside_signed_distance(int Q, const double *dist2, const int32_t *winding2, const int32_t *touches, const int32_t *hits, int rule,
                                     int only_undecided, float *out, uint8_t *decided, hipStream_t s)
{
    if (Q <= 0) return hipSuccess;
    hipLaunchKernelGGL(signed_distance_kernel, dim3((unsigned)(((size_t)Q + 255) / 256)), dim3(256), 0, s, Q, dist2, winding2, touches, hits, rule,
                       only_undecided, out, decided);
    return hipGetLastError();
}
