// mesh_bvh.hip -- a bounding-volume hierarchy over the triangles of a mesh and the exact closest-point query on it (include/ts_bvh.h).
//
// Built with -ffp-contract=off: the float64 distance D', the box bound L and the fp32 points round every operation (the header's text).
//
// Index.  Per face: eligibility and the centroid (NaN for an ineligible face); the bounding box of the eligible centroids (ts_knn_front.h's
// FINITE_ONLY reductions); a 30-bit Morton code, bit 30 set for an ineligible face so that the stable radix sort of (code, face) puts those
// behind every eligible one; leaves of LEAF consecutive sorted faces with their nine fp32 coordinates gathered, so that a leaf reads as one
// stream (slot id -1: ineligible or padding, never evaluated); above them an IMPLICIT tree of fan-out FAN: node k of level l covers the
// leaves [k FAN^l, (k+1) FAN^l), level 0 being the leaves' own boxes.  Boxes are unioned bottom-up, one launch per level: no atomics, nobody
// waits for another workgroup.  A node without an eligible face has the empty box (+inf, -inf) and is never entered.  The layout is made of
// offsets from `bvh` alone, every word of it is written by the build, and a query takes every index it follows from F, never from memory.
//
// Query.  The queries go through the same front half (own bounding box, Morton sort, float4 gather with the original index; a non-finite
// query is stored as NaNs).  The walk is csrc/ts_bvh_walk.h, nearest child first.  What is this kernel's own: every lane keeps (best D',
// face, point); a node is entered when some lane has L(q, box) <= best -- pruning on strict `>` only, which is what makes the result the
// brute-force argmin, ties included (see the header).  The children are ordered by L of the wave's mean query.  At a leaf every lane
// evaluates D' of the leaf's faces for its own query.  `best` is seeded from the leaf that holds the Morton code of the wave's mean query
// (binary search among the sorted face codes); the walk passes that leaf by.
#include "ts_bvh_layout.h" // LEAF, FAN, Leaf, BvhView, bvh_view: shared with the other queries on the index
#include "ts_bvh_launch.h"
#include "ts_bvh_walk.h"

#include <algorithm>

namespace
{
constexpr uint32_t CODE_INELIGIBLE = 0x40000000u; // above every 30-bit Morton code

struct BuildCarve
{
    float *cent;
    uint32_t *codes[2], *ids[2];
    Box *partial;
    void *sort_temp;
    int npartial;
    size_t bytes;
};

BuildCarve build_carve(void *ws, int F)
{
    BuildCarve c;
    const size_t n = (size_t)(F > 0 ? F : 0);
    c.npartial = 256;
    char *p = (char *)ts_align_up((size_t)ws);
    auto take = [&](size_t bytes) { char *q = p; p += ts_align_up(bytes); return q; };
    c.cent = (float *)take(n * 12);
    c.codes[0] = (uint32_t *)take(n * 4); c.codes[1] = (uint32_t *)take(n * 4);
    c.ids[0] = (uint32_t *)take(n * 4); c.ids[1] = (uint32_t *)take(n * 4);
    c.partial = (Box *)take((size_t)c.npartial * sizeof(Box));
    // the radix sort's tables shrink where its chunk length grows (TS_RS_SMALL_BELOW): never less than just below that size
    size_t sort_bytes = ts_radix_scratch_bytes(n);
    if (n > (size_t)TS_RS_SMALL_BELOW) sort_bytes = std::max(sort_bytes, ts_radix_scratch_bytes((size_t)TS_RS_SMALL_BELOW));
    c.sort_temp = take(sort_bytes);
    c.bytes = (size_t)(p - (char *)ws);
    return c;
}

// ---- build ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) face_centroid_kernel(int V, int F, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                             const uint8_t *__restrict__ keep, float *__restrict__ cent)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const float nan = __uint_as_float(0x7FC00000u);
    float cx = nan, cy = nan, cz = nan;
    const int32_t i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if ((!keep || keep[f]) && (uint32_t)i0 < (uint32_t)V && (uint32_t)i1 < (uint32_t)V && (uint32_t)i2 < (uint32_t)V)
    {
        const float *p0 = vertices + 3 * (size_t)i0, *p1 = vertices + 3 * (size_t)i1, *p2 = vertices + 3 * (size_t)i2;
        const float x0 = p0[0], y0 = p0[1], z0 = p0[2], x1 = p1[0], y1 = p1[1], z1 = p1[2], x2 = p2[0], y2 = p2[1], z2 = p2[2];
        if (all_finite(x0, y0, z0) && all_finite(x1, y1, z1) && all_finite(x2, y2, z2))
        {
            cx = (float)((((double)x0 + (double)x1) + (double)x2) / 3.0); // in double: the sum of three finite floats does not overflow
            cy = (float)((((double)y0 + (double)y1) + (double)y2) / 3.0);
            cz = (float)((((double)z0 + (double)z1) + (double)z2) / 3.0);
        }
    }
    cent[3 * (size_t)f] = cx; cent[3 * (size_t)f + 1] = cy; cent[3 * (size_t)f + 2] = cz;
}

__device__ __forceinline__ uint32_t quantise10(double v, float lo, float hi)
{
    const double t = ((v - (double)lo) / ((double)hi - (double)lo)) * 1023.0; // 0/0 for a flat box: NaN -> 0
    return t >= 0.0 ? (uint32_t)fmin(t, 1023.0) : 0u;
}

__device__ __forceinline__ uint32_t code_of(double x, double y, double z, const Box &b)
{
    return prep_morton(quantise10(x, b.mnx, b.mxx)) | (prep_morton(quantise10(y, b.mny, b.mxy)) << 1) | (prep_morton(quantise10(z, b.mnz, b.mxz)) << 2);
}

__global__ void __launch_bounds__(256) face_code_kernel(int F, const float *__restrict__ cent, const Box *__restrict__ bb, uint32_t *__restrict__ codes,
                                                         uint32_t *__restrict__ ids)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const float x = cent[3 * (size_t)f], y = cent[3 * (size_t)f + 1], z = cent[3 * (size_t)f + 2];
    codes[f] = x == x ? code_of(x, y, z, *bb) : CODE_INELIGIBLE;
    ids[f] = (uint32_t)f;
}

// one lane per leaf: its LEAF sorted faces gathered, the padding slots cleared, its box (level 0 of the tree) and its slice of the sorted codes
__global__ void __launch_bounds__(256) leaf_kernel(int F, int nleaves, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                    const uint32_t *__restrict__ codes_sorted, const uint32_t *__restrict__ ids_sorted,
                                                    uint32_t *__restrict__ codes_out, Leaf *__restrict__ leaves, Box *__restrict__ nodes)
{
    const int leaf = blockIdx.x * 256 + threadIdx.x;
    if (leaf >= nleaves) return;
    const float inf = __uint_as_float(0x7F800000u);
    Box box = {inf, inf, inf, -inf, -inf, -inf};
    Leaf *out = leaves + leaf;
    for (int j = 0; j < LEAF; j++)
    {
        const size_t slot = (size_t)leaf * LEAF + j;
        int32_t id = -1;
        float c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (slot < (size_t)F)
        {
            const uint32_t code = codes_sorted[slot];
            codes_out[slot] = code;
            if (code < CODE_INELIGIBLE) // eligible: its indices lie in [0, V) and its coordinates are finite (face_centroid_kernel)
            {
                id = (int32_t)ids_sorted[slot];
#pragma unroll
                for (int k = 0; k < 3; k++)
                {
                    const float *p = vertices + 3 * (size_t)faces[3 * (size_t)id + k];
                    c[3 * k] = p[0]; c[3 * k + 1] = p[1]; c[3 * k + 2] = p[2];
                    box.mnx = fminf(box.mnx, p[0]); box.mny = fminf(box.mny, p[1]); box.mnz = fminf(box.mnz, p[2]);
                    box.mxx = fmaxf(box.mxx, p[0]); box.mxy = fmaxf(box.mxy, p[1]); box.mxz = fmaxf(box.mxz, p[2]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 9; k++) out->v[j][k] = c[k];
        out->id[j] = id;
    }
    nodes[leaf] = box;
}

// one lane per node of a level: the union of its (up to FAN) children of the level below
__global__ void __launch_bounds__(256) union_kernel(int count, int count_below, const Box *__restrict__ below, Box *__restrict__ level)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    const float inf = __uint_as_float(0x7F800000u);
    Box box = {inf, inf, inf, -inf, -inf, -inf};
    const int c0 = k * FAN, c1 = min(count_below - c0, FAN); // k < count = ceil(count_below / FAN): c0 < count_below, no overflow
    for (int c = 0; c < c1; c++)
    {
        const Box b = below[c0 + c];
        box.mnx = fminf(box.mnx, b.mnx); box.mny = fminf(box.mny, b.mny); box.mnz = fminf(box.mnz, b.mnz);
        box.mxx = fmaxf(box.mxx, b.mxx); box.mxy = fmaxf(box.mxy, b.mxy); box.mxz = fmaxf(box.mxz, b.mxz);
    }
    level[k] = box;
}

// ---- query ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

__device__ __forceinline__ double axis_excess(double lo, double hi, double q)
{
    const double below = lo - q, above = q - hi;
    return below > 0.0 ? below : (above > 0.0 ? above : 0.0);
}

// L(q, box) of the header
__device__ __forceinline__ double box_bound(double qx, double qy, double qz, float mnx, float mny, float mnz, float mxx, float mxy, float mxz)
{
    const double ex = axis_excess((double)mnx, (double)mxx, qx), ey = axis_excess((double)mny, (double)mxy, qy), ez = axis_excess((double)mnz, (double)mxz, qz);
    return (ex * ex + ey * ey) + ez * ez;
}

struct Closest
{
    double d, px, py, pz;
};

// seg(p0, p1) of the header; replaces `best` when strictly smaller (or when it is the first candidate)
__device__ __forceinline__ void seg_candidate(double qx, double qy, double qz, double p0x, double p0y, double p0z, double p1x, double p1y, double p1z,
                                              bool first, Closest &best)
{
    const double dx = p1x - p0x, dy = p1y - p0y, dz = p1z - p0z, wx = qx - p0x, wy = qy - p0y, wz = qz - p0z;
    const double den = dot3(dx, dy, dz, dx, dy, dz);
    double t = 0.0;
    if (den != 0.0)
    {
        t = dot3(wx, wy, wz, dx, dy, dz) / den;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    }
    const double tx = t * dx, ty = t * dy, tz = t * dz;
    const double rx = wx - tx, ry = wy - ty, rz = wz - tz;
    const double v = dot3(rx, ry, rz, rx, ry, rz);
    if (first || v < best.d)
    {
        best.d = v; best.px = p0x + tx; best.py = p0y + ty; best.pz = p0z + tz;
    }
}

// D(q, T) of the header and the winning candidate's point
__device__ __forceinline__ Closest point_triangle(double qx, double qy, double qz, double ax, double ay, double az, double bx, double by, double bz,
                                                  double cx, double cy, double cz)
{
    Closest best;
    seg_candidate(qx, qy, qz, ax, ay, az, bx, by, bz, true, best);
    seg_candidate(qx, qy, qz, bx, by, bz, cx, cy, cz, false, best);
    seg_candidate(qx, qy, qz, cx, cy, cz, ax, ay, az, false, best);
    const double e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double nn = dot3(nx, ny, nz, nx, ny, nz);
    if (nn > 0.0)
    {
        const double wax = qx - ax, way = qy - ay, waz = qz - az;
        const double s1 = dot3(e1y * waz - e1z * way, e1z * wax - e1x * waz, e1x * way - e1y * wax, nx, ny, nz);
        const double fx = cx - bx, fy = cy - by, fz = cz - bz, wbx = qx - bx, wby = qy - by, wbz = qz - bz;
        const double s2 = dot3(fy * wbz - fz * wby, fz * wbx - fx * wbz, fx * wby - fy * wbx, nx, ny, nz);
        const double gx = ax - cx, gy = ay - cy, gz = az - cz, wcx = qx - cx, wcy = qy - cy, wcz = qz - cz;
        const double s3 = dot3(gy * wcz - gz * wcy, gz * wcx - gx * wcz, gx * wcy - gy * wcx, nx, ny, nz);
        if (s1 >= 0.0 && s2 >= 0.0 && s3 >= 0.0)
        {
            const double s = dot3(wax, way, waz, nx, ny, nz);
            const double v = (s * s) / nn;
            if (v < best.d)
            {
                const double k = s / nn;
                best.d = v; best.px = qx - k * nx; best.py = qy - k * ny; best.pz = qz - k * nz;
            }
        }
    }
    return best;
}

__global__ void __launch_bounds__(TPB) closest_kernel(int Q, int F, int nleaves, int nlevels, const float4 *__restrict__ qsp, const Box *__restrict__ bbox,
                                                       const uint32_t *__restrict__ codes, const Leaf *__restrict__ leaves, const Box *__restrict__ nodes,
                                                       int32_t *__restrict__ face, double *__restrict__ dist2, float *__restrict__ point,
                                                       unsigned long long *leaf_visits)
{
    __shared__ WalkShared ws;
    walk_levels(ws, nleaves);
    const float nanf_ = __uint_as_float(0x7FC00000u);
    const double inf = __longlong_as_double(0x7FF0000000000000ll), nan = __longlong_as_double(0x7FF8000000000000ll);
    const WalkQuery q = walk_query(Q, qsp);
    const double qx = (double)q.p.x, qy = (double)q.p.y, qz = (double)q.p.z;
    double best = inf;
    uint32_t bestid = 0xFFFFFFFFu;
    float bpx = nanf_, bpy = nanf_, bpz = nanf_;
    unsigned visits = 0;

    const unsigned long long alive = __ballot(q.live);
    if (alive != 0ull) // wave-uniform
    {
        // the wave's mean query: orders the children and picks the seed leaf; any value would do for the result
        double mx = q.live ? qx : 0.0, my = q.live ? qy : 0.0, mz = q.live ? qz : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
        {
            mx += __shfl_xor(mx, o); my += __shfl_xor(my, o); mz += __shfl_xor(mz, o);
        }
        const double n_alive = (double)__popcll(alive);
        mx /= n_alive; my /= n_alive; mz /= n_alive;

        auto visit_leaf = [&](int leaf) {
            visits++;
            for_each_face(leaves[leaf], [&](int32_t id, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
                const double lt = box_bound(qx, qy, qz, fminf(fminf(ax, bx), cx), fminf(fminf(ay, by), cy), fminf(fminf(az, bz), cz),
                                            fmaxf(fmaxf(ax, bx), cx), fmaxf(fmaxf(ay, by), cy), fmaxf(fmaxf(az, bz), cz));
                if (!q.live || lt > best) return; // D' >= L(q, AABB(T)) > best: neither a gain nor a tie
                const Closest c = point_triangle(qx, qy, qz, ax, ay, az, bx, by, bz, cx, cy, cz);
                const double d = c.d > lt ? c.d : lt;
                if (d < best || (d == best && (uint32_t)id < bestid))
                {
                    best = d; bestid = (uint32_t)id;
                    bpx = (float)c.px; bpy = (float)c.py; bpz = (float)c.pz;
                }
            });
        };

        // seed: the leaf at the lower bound of the mean query's code among the sorted face codes
        const Box bb = *bbox;
        const uint32_t mcode = code_of(mx, my, mz, bb);
        int lo = 0, hi = F; // the first slot whose code is >= mcode, F when there is none
        while (lo < hi)
        {
            const int mid = lo + (hi - lo) / 2;
            if (codes[mid] < mcode) lo = mid + 1;
            else hi = mid;
        }
        const int seed = __builtin_amdgcn_readfirstlane(min(lo, F - 1) / LEAF); // F >= 1 here: seed < nleaves
        visit_leaf(seed);

        bvh_walk<true>(
            ws, nlevels, nodes,
            [&](int, uint32_t, uint32_t, const Box &b) {
                const double lq = box_bound(qx, qy, qz, b.mnx, b.mny, b.mnz, b.mxx, b.mxy, b.mxz);
                return __ballot(q.live && !(lq > best)) != 0ull; // strict: an equal bound may hide a smaller face index
            },
            [&](int leaf) {
                if (leaf != seed) visit_leaf(leaf);
            },
            [&](const Box &cb) { return (float)box_bound(mx, my, mz, cb.mnx, cb.mny, cb.mnz, cb.mxx, cb.mxy, cb.mxz); });
    }

    if (q.inside)
    {
        face[q.pid] = bestid == 0xFFFFFFFFu ? -1 : (int32_t)bestid;
        dist2[q.pid] = q.live ? best : nan;
        if (point)
        {
            point[3 * (size_t)q.pid] = bpx; point[3 * (size_t)q.pid + 1] = bpy; point[3 * (size_t)q.pid + 2] = bpz;
        }
    }
    if (leaf_visits && (threadIdx.x & 63) == 0 && visits) atomicAdd(leaf_visits, (unsigned long long)visits);
}

// F == 0: nobody has a face
__global__ void __launch_bounds__(256) no_faces_kernel(int Q, const float *__restrict__ queries, int32_t *__restrict__ face, double *__restrict__ dist2,
                                                        float *__restrict__ point)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    const bool finite = all_finite(queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2]);
    const float nan = __uint_as_float(0x7FC00000u);
    face[i] = -1;
    dist2[i] = __longlong_as_double(finite ? 0x7FF0000000000000ll : 0x7FF8000000000000ll);
    if (point)
    {
        point[3 * (size_t)i] = nan; point[3 * (size_t)i + 1] = nan; point[3 * (size_t)i + 2] = nan;
    }
}
} // namespace

size_t ts_bvh_bytes(int F) { return bvh_view(nullptr, F).bytes; }

size_t ts_bvh_build_workspace_bytes(int F) { return build_carve(nullptr, F).bytes + TS_ALIGN; }

hipError_t ts_bvh_build(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, void *bvh, void *ws, hipStream_t s)
{
    if (F <= 0) return hipSuccess;
    const BvhView b = bvh_view(bvh, F);
    const BuildCarve c = build_carve(ws, F);
    const unsigned fblocks = (unsigned)(((size_t)F + 255) / 256);
    hipLaunchKernelGGL(face_centroid_kernel, dim3(fblocks), dim3(256), 0, s, V, F, vertices, faces, keep, c.cent);
    hipLaunchKernelGGL(bbox_partial_kernel<true>, dim3(c.npartial), dim3(TPB), 0, s, F, c.cent, c.partial);
    hipLaunchKernelGGL(bbox_finish_kernel<true>, dim3(1), dim3(64), 0, s, c.npartial, c.partial, b.bbox);
    hipLaunchKernelGGL(face_code_kernel, dim3(fblocks), dim3(256), 0, s, F, c.cent, b.bbox, c.codes[0], c.ids[0]);
    const int at = ts_radix_sort_pairs(c.codes, c.ids, (size_t)F, 31, c.sort_temp, s); // 30 Morton bits + the ineligible bit; stable
    hipLaunchKernelGGL(leaf_kernel, dim3((unsigned)((b.nleaves + 255) / 256)), dim3(256), 0, s, F, b.nleaves, vertices, faces, c.codes[at], c.ids[at],
                       b.codes, b.leaves, b.nodes);
    for (int l = 1; l < b.nlevels; l++)
        hipLaunchKernelGGL(union_kernel, dim3((unsigned)((b.count[l] + 255) / 256)), dim3(256), 0, s, b.count[l], b.count[l - 1],
                           b.nodes + b.offset[l - 1], b.nodes + b.offset[l]);
    return hipGetLastError();
}

size_t ts_bvh_closest_workspace_bytes(int Q) { return query_carve_bytes(Q) + TS_ALIGN; }

hipError_t ts_bvh_closest(int Q, const float *queries, int F, const void *bvh, int32_t *face, double *dist2, float *point,
                          unsigned long long *leaf_visits, void *ws, hipStream_t s)
{
    if (Q <= 0) return hipSuccess;
    if (F <= 0)
    {
        hipLaunchKernelGGL(no_faces_kernel, dim3((unsigned)(((size_t)Q + 255) / 256)), dim3(256), 0, s, Q, queries, face, dist2, point);
        return hipGetLastError();
    }
    const BvhView b = bvh_view(const_cast<void *>(bvh), F);
    const KnnCarve cq = knn_carve((void *)ts_align_up((size_t)ws), Q);
    const hipError_t e = knn_prepare<true>(Q, queries, cq, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(closest_kernel, dim3((unsigned)(((size_t)Q + TPB - 1) / TPB)), dim3(TPB), 0, s, Q, F, b.nleaves, b.nlevels, cq.sp, b.bbox, b.codes, b.leaves, b.nodes, face, dist2,
                       point, leaf_visits);
    return hipGetLastError();
}
