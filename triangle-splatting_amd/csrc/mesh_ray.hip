// mesh_ray.hip -- the exact first hit of a ray on the triangles of a mesh (include/ts_ray.h), on the index that mesh_bvh.hip's build wrote
// (csrc/ts_bvh_layout.h).
//
// Built with -ffp-contract=off: the slab interval, the watertight triangle test and the reported t' round every operation (the header's text).
// The two tests are csrc/ts_ray_tests.h, shared with mesh_inside.hip (include/ts_inside.h), which counts all hits where this unit keeps the first.
//
// The rays go through the front half of the box searches (ts_knn_front.h): the bounding box of the finite ORIGINS, a Morton sort, a float4
// gather that carries the original index; a ray with a non-finite origin is stored as NaNs.  The key is the origin alone: the rays of one
// camera share it and the stable sort leaves them in pixel order, which is coherent already; the result does not depend on the key.  The
// direction and the per-ray limit are read through the original index.
//
// One wave owns 64 consecutive sorted rays, one per lane; every lane keeps (best t', face, bary, side) of its own and works out
// kz / kx / ky / Sx / Sy / Sz once, before the walk.  Control flow is wave-uniform: the wave pops a node from its stack in LDS, every lane
// evaluates the slab interval of the node's box, and the node is entered when __ballot says that some live lane crosses it with tn <= best --
// pruning on strict `>` only, which is what makes the result the brute-force first hit, ties included (see the header).  An inner node pushes
// its non-empty children, the one the wave's mean ray enters last first, so that the nearest is popped first.  At a leaf the faces' words
// are wave-uniform loads; every lane tests the face's own box first (not crossed, or tn > best: skip), then the triangle.  `best` starts at
// the ray's upper limit `hi` with no face: the acceptance t' <= hi and the pruning tn > best are the same comparison from the first node on.
//
// Stack: STACK entries per wave in LDS, whatever the data (the argument stands in ts_bvh_walk.h).
//
// The walk below is this kernel's own text, where the other three queries on the index use csrc/ts_bvh_walk.h: on the shared walk one of
// the five measured ray sets (one direction repeated per ray) ran 2 - 3.5 % slower at equal leaf visits, whichever way the set-up was
// worded (profiles/bvh_walk_ab.json).  A change to the fan-out, the stack or the node packing is made there and here.
#include "ts_bvh_layout.h"
#include "ts_bvh_walk.h" // WAVES, query_carve_bytes
#include "ts_ray_launch.h"
#include "ts_ray_tests.h"

namespace
{
__global__ void __launch_bounds__(TPB) cast_kernel(int Q, int nleaves, int nlevels, const float4 *__restrict__ osp, const float *__restrict__ directions,
                                                    const float *__restrict__ t_limit, double tmin, double tmax, int cull_back,
                                                    const Leaf *__restrict__ leaves, const Box *__restrict__ nodes, int32_t *__restrict__ face,
                                                    double *__restrict__ t_out, float *__restrict__ bary, int8_t *__restrict__ side,
                                                    unsigned long long *leaf_visits)
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
    const double inf = __longlong_as_double(0x7FF0000000000000ll), nan = __longlong_as_double(0x7FF8000000000000ll);
    const size_t i = (size_t)blockIdx.x * TPB + tid;
    const bool inside = i < (size_t)Q;
    const float4 p = inside ? osp[i] : make_float4(nanf_, nanf_, nanf_, 0.0f);
    const uint32_t pid = __float_as_uint(p.w); // < Q for a lane inside: the sorted index of the front half
    bool live = inside && p.x == p.x; // a non-finite origin was stored as NaNs
    float fdx = 0.0f, fdy = 0.0f, fdz = 0.0f;
    double hi = tmax;
    if (live)
    {
        fdx = directions[3 * (size_t)pid]; fdy = directions[3 * (size_t)pid + 1]; fdz = directions[3 * (size_t)pid + 2];
        live = ray_direction_valid(fdx, fdy, fdz);
        if (t_limit)
        {
            const float tl = t_limit[pid];
            if (tl != tl) live = false;
            else hi = min2(tmax, (double)tl);
        }
    }
    const double ox = live ? (double)p.x : 0.0, oy = live ? (double)p.y : 0.0, oz = live ? (double)p.z : 0.0;
    const double dx = live ? (double)fdx : 1.0, dy = live ? (double)fdy : 0.0, dz = live ? (double)fdz : 0.0;

    const RayShear sh = ray_shear(ox, oy, oz, dx, dy, dz); // the dominant axis and the shear of the watertight test, once per ray

    double best = hi;
    uint32_t bestid = 0xFFFFFFFFu;
    float b0 = nanf_, b1 = nanf_, b2 = nanf_;
    int bside = 0;
    unsigned visits = 0;

    const unsigned long long alive = __ballot(live);
    if (alive != 0ull) // wave-uniform
    {
        // the wave's mean ray orders the children; any value would do for the result
        double mox = live ? ox : 0.0, moy = live ? oy : 0.0, moz = live ? oz : 0.0;
        double mdx = live ? dx : 0.0, mdy = live ? dy : 0.0, mdz = live ? dz : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
        {
            mox += __shfl_xor(mox, o); moy += __shfl_xor(moy, o); moz += __shfl_xor(moz, o);
            mdx += __shfl_xor(mdx, o); mdy += __shfl_xor(mdy, o); mdz += __shfl_xor(mdz, o);
        }
        const double n_alive = (double)__popcll(alive);
        mox /= n_alive; moy /= n_alive; moz /= n_alive;
        mdx /= n_alive; mdy /= n_alive; mdz /= n_alive;

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
                if (!live || !crossed || !(tf >= tmin) || tn > best) continue; // t' >= tn(AABB(T)) > best: neither a gain nor a tie
                const FaceEdges e = face_edges(sh, ax, ay, az, bx, by, bz, cx, cy, cz);
                if (!face_candidate(e) || (cull_back && !(e.det > 0.0))) continue;
                const double tt = face_t(sh, e);
                const double tp = max2(tt, tn);
                if (!(tp >= tmin && tp <= hi)) continue;
                if (tp < best || (tp == best && (uint32_t)id < bestid))
                {
                    best = tp; bestid = (uint32_t)id;
                    b0 = (float)(e.U / e.det); b1 = (float)(e.V / e.det); b2 = (float)(e.W / e.det);
                    bside = e.det > 0.0 ? 1 : -1;
                }
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
            if (__ballot(live && crossed && tf >= tmin && !(tn > best)) == 0ull) continue; // strict: an equal bound may hide a smaller face index
            if (level == 0)
            {
                visit_leaf((int)k);
                continue;
            }
            const uint32_t c0 = k * FAN, below = __builtin_amdgcn_readfirstlane(lvl_cnt[level - 1]);
            const uint32_t base = __builtin_amdgcn_readfirstlane(lvl_off[level - 1]) + c0;
            const int nchild = (int)min(below - c0, (uint32_t)FAN); // c0 < below: k < ceil(below / FAN)
            float key[FAN];
            unsigned want = 0;
#pragma unroll
            for (int c = 0; c < FAN; c++)
            {
                key[c] = 0.0f;
                if (c < nchild)
                {
                    const Box cb = nodes[base + c];
                    if (!(cb.mnx > cb.mxx))
                    {
                        double ctn, ctf; // where the mean ray enters the child; a child it misses sorts behind the others
                        const bool hit = slab(mox, moy, moz, mdx, mdy, mdz, cb.mnx, cb.mny, cb.mnz, cb.mxx, cb.mxy, cb.mxz, ctn, ctf);
                        key[c] = hit ? fminf(fmaxf((float)ctn, -FLT_MAX), FLT_MAX) : FLT_MAX;
                        want |= 1u << c;
                    }
                }
            }
            while (want) // at most FAN pushes: the farthest first (ties: the highest index first), so that pops come nearest first
            {
                int far = -1;
                float far_key = 0.0f;
#pragma unroll
                for (int c = 0; c < FAN; c++)
                    if (((want >> c) & 1u) && (far < 0 || key[c] >= far_key)) { far = c; far_key = key[c]; }
                want &= ~(1u << far);
                if (sp < STACK) st[sp++] = ((uint32_t)(level - 1) << 28) | (c0 + (uint32_t)far); // sp < STACK always (ts_bvh_walk.h); the test costs nothing
            }
        }
    }

    if (inside)
    {
        const bool found = bestid != 0xFFFFFFFFu;
        face[pid] = found ? (int32_t)bestid : -1;
        t_out[pid] = live ? (found ? best : inf) : nan;
        if (bary)
        {
            bary[3 * (size_t)pid] = b0; bary[3 * (size_t)pid + 1] = b1; bary[3 * (size_t)pid + 2] = b2;
        }
        if (side) side[pid] = (int8_t)bside;
    }
    if (leaf_visits && (tid & 63) == 0 && visits) atomicAdd(leaf_visits, (unsigned long long)visits);
}

// F == 0: nobody hits anything
__global__ void __launch_bounds__(256) no_faces_kernel(int Q, const float *__restrict__ origins, const float *__restrict__ directions,
                                                        const float *__restrict__ t_limit, int32_t *__restrict__ face, double *__restrict__ t_out,
                                                        float *__restrict__ bary, int8_t *__restrict__ side)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    const float dx = directions[3 * (size_t)i], dy = directions[3 * (size_t)i + 1], dz = directions[3 * (size_t)i + 2];
    const bool good = ray_valid(all_finite(origins[3 * (size_t)i], origins[3 * (size_t)i + 1], origins[3 * (size_t)i + 2]), dx, dy, dz, t_limit, i);
    const float nan = __uint_as_float(0x7FC00000u);
    face[i] = -1;
    t_out[i] = __longlong_as_double(good ? 0x7FF0000000000000ll : 0x7FF8000000000000ll);
    if (bary)
    {
        bary[3 * (size_t)i] = nan; bary[3 * (size_t)i + 1] = nan; bary[3 * (size_t)i + 2] = nan;
    }
    if (side) side[i] = 0;
}
} // namespace

size_t ts_ray_bvh_bytes(int F) { return bvh_view(nullptr, F).bytes; }

size_t ts_ray_cast_workspace_bytes(int Q) { return query_carve_bytes(Q) + TS_ALIGN; }

hipError_t ts_ray_cast(int Q, const float *origins, const float *directions, const float *t_limit, double tmin, double tmax, int cull_back, int F,
                       const void *bvh, int32_t *face, double *t, float *bary, int8_t *side, unsigned long long *leaf_visits, void *ws, hipStream_t s)
{
    if (Q <= 0) return hipSuccess;
    if (F <= 0)
    {
        hipLaunchKernelGGL(no_faces_kernel, dim3((unsigned)(((size_t)Q + 255) / 256)), dim3(256), 0, s, Q, origins, directions, t_limit, face, t, bary, side);
        return hipGetLastError();
    }
    const BvhView b = bvh_view(const_cast<void *>(bvh), F);
    const KnnCarve cq = knn_carve((void *)ts_align_up((size_t)ws), Q);
    const hipError_t e = knn_prepare<true>(Q, origins, cq, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cast_kernel, dim3((unsigned)(((size_t)Q + TPB - 1) / TPB)), dim3(TPB), 0, s, Q, b.nleaves, b.nlevels, cq.sp, directions, t_limit, tmin, tmax, cull_back, b.leaves,
                       b.nodes, face, t, bary, side, leaf_visits);
    return hipGetLastError();
}
