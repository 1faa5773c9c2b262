// mesh_inside.hip -- all hits of a ray on the triangles of a mesh, counted in half crossings, and the signed distance that follows
// (include/ts_inside.h), on the index that mesh_bvh.hip's build wrote (csrc/ts_bvh_layout.h).
//
// Built with -ffp-contract=off: the slab interval and the watertight triangle test round every operation.  Both are csrc/ts_ray_tests.h, the
// text that mesh_ray.hip evaluates a ray with: a face is hit here exactly when it is hit there.
//
// The rays go through the front half of the box searches (ts_knn_front.h) like those of mesh_ray.hip: the bounding box of the finite
// ORIGINS, a Morton sort, a float4 gather that carries the original index; a ray with a non-finite origin is stored as NaNs.  The direction
// and the per-ray limit are read through the original index; with SHARED the direction is three wave-uniform loads and the dominant axis
// and the shear live in scalar registers.
//
// One wave owns 64 consecutive sorted rays, one per lane; every lane keeps three int32 counters.  Control flow is wave-uniform: the wave pops
// a node from its stack in LDS, every lane evaluates the slab interval of the node's box, and the node is entered when __ballot says that some
// live lane crosses it with tf >= tmin and tn <= hi.  There is no nearest hit: nothing to prune on, so no child ordering and no mean ray; an
// inner node pushes its non-empty children in index order.  At a leaf the faces' words are wave-uniform loads; every lane tests the face's
// own box first, then the triangle, and counts.  The sums are integers: the order of the walk does not matter.
//
// Stack: STACK entries per wave in LDS, whatever the data (ts_bvh_layout.h).
#include "ts_bvh_layout.h"
#include "ts_inside_launch.h"
#include "ts_ray_tests.h"

#include <algorithm>

namespace
{
constexpr int WAVES = TPB / 64;

size_t inside_carve_bytes(int n)
{
    // the radix sort's tables shrink where its chunk length grows (TS_RS_SMALL_BELOW): never less than just below that size
    const size_t b = knn_carve(nullptr, n).bytes;
    return n > TS_RS_SMALL_BELOW ? std::max(b, knn_carve(nullptr, TS_RS_SMALL_BELOW).bytes) : b;
}

template <bool SHARED>
__global__ void __launch_bounds__(TPB) crossings_kernel(int Q, int nleaves, int nlevels, const float4 *__restrict__ osp,
                                                         const float *__restrict__ directions, const float *__restrict__ t_limit, double tmin,
                                                         double tmax, const Leaf *__restrict__ leaves, const Box *__restrict__ nodes,
                                                         int32_t *__restrict__ hits_out, int32_t *__restrict__ winding2_out,
                                                         int32_t *__restrict__ touches_out, unsigned long long *leaf_visits)
{
    __shared__ uint32_t lvl_off[MAX_LEVELS], lvl_cnt[MAX_LEVELS];
    __shared__ uint32_t stack[WAVES][STACK];
    const int tid = threadIdx.x, wave = tid >> 6;
    if (tid < MAX_LEVELS) // the level table follows from the leaf count alone (bvh_view)
    {
        uint32_t off = 0, cnt = (uint32_t)nleaves;
        for (int l = 0; l < tid; l++)
        {
            off += cnt;
            cnt = (cnt + FAN - 1) >> FAN_SHIFT;
        }
        lvl_off[tid] = off; lvl_cnt[tid] = cnt;
    }
    __syncthreads(); // the only one: from here on every wave is on its own

    const float nanf_ = __uint_as_float(0x7FC00000u);
    const size_t i = (size_t)blockIdx.x * TPB + tid;
    const bool inside = i < (size_t)Q;
    const float4 p = inside ? osp[i] : make_float4(nanf_, nanf_, nanf_, 0.0f);
    const uint32_t pid = __float_as_uint(p.w); // < Q for a lane inside: the sorted index of the front half
    bool live = inside && p.x == p.x; // a non-finite origin was stored as NaNs
    float fdx, fdy, fdz;
    if (SHARED) // three scalar loads: a bad shared direction makes every ray bad
    {
        fdx = directions[0]; fdy = directions[1]; fdz = directions[2];
    }
    else
    {
        const size_t at = live ? 3 * (size_t)pid : 0; // Q >= 1: the first ray's direction is there to read
        fdx = directions[at]; fdy = directions[at + 1]; fdz = directions[at + 2];
    }
    const bool good_d = finite_f(fdx) && finite_f(fdy) && finite_f(fdz) && !(fdx == 0.0f && fdy == 0.0f && fdz == 0.0f); // SHARED: wave-uniform
    live = live && good_d;
    double hi = tmax;
    if (live && t_limit)
    {
        const float tl = t_limit[pid];
        if (tl != tl) live = false;
        else hi = min2(tmax, (double)tl);
    }
    // a lane that is not live walks along with finite stand-ins and never counts; the direction's stand-in depends on the direction alone
    const double ox = live ? (double)p.x : 0.0, oy = live ? (double)p.y : 0.0, oz = live ? (double)p.z : 0.0;
    const double dx = good_d ? (double)fdx : 1.0, dy = good_d ? (double)fdy : 0.0, dz = good_d ? (double)fdz : 0.0;
    const RayShear sh = ray_shear(ox, oy, oz, dx, dy, dz); // with SHARED the axes and the shear are wave-uniform, the origin's part is not

    int hits = 0, winding2 = 0, touches = 0;
    unsigned visits = 0;

    if (__ballot(live) != 0ull) // wave-uniform
    {
        auto visit_leaf = [&](int leaf) {
            visits++;
            const Leaf &lf = leaves[leaf];
#pragma unroll 1
            for (int j = 0; j < LEAF; j++)
            {
                const int32_t id = lf.id[j];
                if (id < 0) continue; // wave-uniform: an ineligible or padding slot
                const float ax = lf.v[j][0], ay = lf.v[j][1], az = lf.v[j][2], bx = lf.v[j][3], by = lf.v[j][4], bz = lf.v[j][5], cx = lf.v[j][6],
                            cy = lf.v[j][7], cz = lf.v[j][8];
                double tn, tf;
                const bool crossed = face_slab(ox, oy, oz, dx, dy, dz, ax, ay, az, bx, by, bz, cx, cy, cz, tn, tf);
                if (!live || !crossed || !(tf >= tmin) || tn > hi) continue;
                const FaceEdges e = face_edges(sh, ax, ay, az, bx, by, bz, cx, cy, cz);
                if (!face_candidate(e)) continue;
                const double tp = max2(face_t(sh, e), tn);
                if (!(tp >= tmin && tp <= hi)) continue;
                const int z = (e.U == 0.0) + (e.V == 0.0) + (e.W == 0.0); // at most 2: det != 0
                const int s = e.det > 0.0 ? 1 : -1;
                hits++;
                winding2 += z == 0 ? 2 * s : (z == 1 ? s : 0);
                touches += z >= 2;
            }
        };

        uint32_t *st = stack[wave];
        int sp = 0;
        st[sp++] = (uint32_t)(nlevels - 1) << 28; // the root: node 0 of the top level
        while (sp > 0)
        {
            const uint32_t e = __builtin_amdgcn_readfirstlane(st[--sp]);
            const int level = (int)(e >> 28);
            const uint32_t k = e & 0x0FFFFFFFu; // k < lvl_cnt[level] by construction: the root is (top, 0), children are bounded below
            const Box b = nodes[__builtin_amdgcn_readfirstlane(lvl_off[level] + k)];
            if (b.mnx > b.mxx) continue; // no eligible face below
            double tn, tf;
            const bool crossed = slab(ox, oy, oz, dx, dy, dz, b.mnx, b.mny, b.mnz, b.mxx, b.mxy, b.mxz, tn, tf);
            if (__ballot(live && crossed && tf >= tmin && !(tn > hi)) == 0ull) continue;
            if (level == 0)
            {
                visit_leaf((int)k);
                continue;
            }
            const uint32_t c0 = k * FAN, below = __builtin_amdgcn_readfirstlane(lvl_cnt[level - 1]);
            const int nchild = (int)min(below - c0, (uint32_t)FAN); // c0 < below: k < ceil(below / FAN)
            for (int c = nchild - 1; c >= 0; c--) // the last first: pops come in index order, the order of the leaves in memory
                if (sp < STACK) st[sp++] = ((uint32_t)(level - 1) << 28) | (c0 + (uint32_t)c); // sp < STACK always (ts_bvh_layout.h); the test costs nothing
        }
    }

    if (inside)
    {
        hits_out[pid] = live ? hits : -1;
        winding2_out[pid] = winding2;
        touches_out[pid] = touches;
    }
    if (leaf_visits && (tid & 63) == 0 && visits) atomicAdd(leaf_visits, (unsigned long long)visits);
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
    bool good = all_finite(origins[3 * (size_t)i], origins[3 * (size_t)i + 1], origins[3 * (size_t)i + 2]) && all_finite(dx, dy, dz) &&
                !(dx == 0.0f && dy == 0.0f && dz == 0.0f);
    if (t_limit && t_limit[i] != t_limit[i]) good = false;
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

size_t ts_inside_crossings_workspace_bytes(int Q) { return inside_carve_bytes(Q) + TS_ALIGN; }

hipError_t ts_inside_crossings(int Q, const float *origins, const float *directions, int shared_direction, const float *t_limit, double tmin,
                               double tmax, int F, const void *bvh, int32_t *hits, int32_t *winding2, int32_t *touches,
                               unsigned long long *leaf_visits, void *ws, hipStream_t s)
{
    if (Q <= 0) return hipSuccess;
    const unsigned qblocks = (unsigned)(((size_t)Q + TPB - 1) / TPB);
    if (F <= 0)
    {
        hipLaunchKernelGGL(no_faces_kernel, dim3(qblocks), dim3(256), 0, s, Q, origins, directions, shared_direction ? 0 : 3, t_limit, hits, winding2,
                           touches);
        return hipGetLastError();
    }
    const BvhView b = bvh_view(const_cast<void *>(bvh), F);
    const KnnCarve cq = knn_carve((void *)ts_align_up((size_t)ws), Q);
    const hipError_t e = knn_prepare<true>(Q, origins, cq, s);
    if (e != hipSuccess) return e;
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
