// mesh_overlap.hip -- the overlap query of the triangle index that mesh_bvh.hip's build wrote (csrc/ts_bvh_layout.h): which faces of the
// index does a triangle meet, for every face of a mesh at once (include/ts_overlap.h).
//
// Built with -ffp-contract=off: the plane values and the segment tests round every operation (the header's text).  Every sum is an integer
// atomic and a pair is evaluated by one lane alone, so neither the order of the walk nor the company in the wave changes a result; only the
// order of the pair list depends on them, and the sort call removes that.
//
// Query.  The queries are the leaf slots of the QUERY index: the build sorted them by Morton code, so there is no front half, no radix sort
// and no workspace.  One wave owns 64 consecutive slots (8 leaves), one per lane; a slot with id < 0 is a dead lane.  The walk is
// csrc/ts_bvh_walk.h, children in index order.  What is this kernel's own: every lane keeps its nine coordinates, its face box, its id and,
// in self mode, its three vertex indices; a node is entered when some live lane's box overlaps the node's; at a leaf the partner's words
// are wave-uniform loads (in self mode its three indices are one more, from `faces`), and a lane goes on iff the partner takes part, the
// boxes overlap and, in self mode, its own id is below the partner's: each unordered pair is evaluated once.  The plane values come first
// and most candidates leave on "apart".
//
// Sort.  Two stable radix sorts over (key, position) records, by the second entry and then by the first, as sort_half_edges
// (ts_mesh_edges.h) orders its edges; pairs and kinds are gathered into the workspace and copied back.
#include "ts_bvh_layout.h"
#include "ts_bvh_walk.h"
#include "ts_mesh_common.h"
#include "ts_overlap_launch.h"

namespace
{
constexpr int KIND_CROSSING = 1, KIND_COPLANAR = 2, KIND_DUPLICATE = 3;
// stats words of the header; CURSOR is the list's cursor while the kernel runs and 0 afterwards
constexpr int S_CANDIDATES = 0, S_ADJACENT = 1, S_CROSSING = 2, S_COPLANAR = 3, S_DUPLICATE = 4, S_DEGENERATE = 5, S_STORED = 6, S_CURSOR = 7;

struct P3
{
    double x, y, z;
};

__device__ __forceinline__ P3 widen(float x, float y, float z) { return {(double)x, (double)y, (double)z}; }

// (b - a) . ((c - a) x (d - a))
__device__ __forceinline__ double orient(const P3 &a, const P3 &b, const P3 &c, const P3 &d)
{
    const double ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z, wx = d.x - a.x, wy = d.y - a.y,
                 wz = d.z - a.z;
    const double cx = vy * wz - vz * wy, cy = vz * wx - vx * wz, cz = vx * wy - vy * wx;
    return (ux * cx + uy * cy) + uz * cz;
}

// seg(p, q, sp, sq; t0, t1, t2) of the header
__device__ __forceinline__ bool seg_meets(const P3 &p, const P3 &q, double sp, double sq, const P3 &t0, const P3 &t1, const P3 &t2)
{
    if ((sp > 0.0 && sq > 0.0) || (sp < 0.0 && sq < 0.0) || (sp == 0.0 && sq == 0.0)) return false;
    const double e0 = orient(p, q, t0, t1), e1 = orient(p, q, t1, t2), e2 = orient(p, q, t2, t0);
    return (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
}

// 0 apart, 1 coplanar, 2 neither: the plane values v0..v2 of one face's vertices, `skip` the shared one (-1: none)
__device__ __forceinline__ int side_of(double v0, double v1, double v2, int skip)
{
    const int n = skip < 0 ? 3 : 2;
    const bool u0 = skip != 0, u1 = skip != 1, u2 = skip != 2;
    const int pos = (int)(u0 && v0 > 0.0) + (int)(u1 && v1 > 0.0) + (int)(u2 && v2 > 0.0);
    const int neg = (int)(u0 && v0 < 0.0) + (int)(u1 && v1 < 0.0) + (int)(u2 && v2 < 0.0);
    const int zero = (int)(u0 && v0 == 0.0) + (int)(u1 && v1 == 0.0) + (int)(u2 && v2 == 0.0);
    return pos == n || neg == n ? 0 : (zero == n ? 1 : 2);
}

// the kind of the pair A = (a0, a1, a2), B = (b0, b1, b2); sa, sb: which vertex of A and of B is the shared one, -1 and -1 for none
__device__ __forceinline__ int pair_kind(const P3 &a0, const P3 &a1, const P3 &a2, const P3 &b0, const P3 &b1, const P3 &b2, int sa, int sb)
{
    const double pB0 = sb == 0 ? 0.0 : orient(a0, a1, a2, b0), pB1 = sb == 1 ? 0.0 : orient(a0, a1, a2, b1),
                 pB2 = sb == 2 ? 0.0 : orient(a0, a1, a2, b2);
    const int sideB = side_of(pB0, pB1, pB2, sb);
    if (sideB == 0) return 0; // most candidates end here
    const double pA0 = sa == 0 ? 0.0 : orient(b0, b1, b2, a0), pA1 = sa == 1 ? 0.0 : orient(b0, b1, b2, a1),
                 pA2 = sa == 2 ? 0.0 : orient(b0, b1, b2, a2);
    const int sideA = side_of(pA0, pA1, pA2, sa);
    if (sideA == 0) return 0;
    if (sideB == 1 || sideA == 1) return KIND_COPLANAR;
    bool hit;
    if (sa < 0)
        hit = seg_meets(a0, a1, pA0, pA1, b0, b1, b2) || seg_meets(a1, a2, pA1, pA2, b0, b1, b2) || seg_meets(a2, a0, pA2, pA0, b0, b1, b2) ||
              seg_meets(b0, b1, pB0, pB1, a0, a1, a2) || seg_meets(b1, b2, pB1, pB2, a0, a1, a2) || seg_meets(b2, b0, pB2, pB0, a0, a1, a2);
    else
    {
        // the edge opposite the shared vertex, in the direction it has in the list a0 a1, a1 a2, a2 a0
        const P3 &ap = sa == 0 ? a1 : (sa == 1 ? a2 : a0), &aq = sa == 0 ? a2 : (sa == 1 ? a0 : a1);
        const double asp = sa == 0 ? pA1 : (sa == 1 ? pA2 : pA0), asq = sa == 0 ? pA2 : (sa == 1 ? pA0 : pA1);
        const P3 &bp = sb == 0 ? b1 : (sb == 1 ? b2 : b0), &bq = sb == 0 ? b2 : (sb == 1 ? b0 : b1);
        const double bsp = sb == 0 ? pB1 : (sb == 1 ? pB2 : pB0), bsq = sb == 0 ? pB2 : (sb == 1 ? pB0 : pB1);
        hit = seg_meets(ap, aq, asp, asq, b0, b1, b2) || seg_meets(bp, bq, bsp, bsq, a0, a1, a2);
    }
    return hit ? KIND_CROSSING : 0;
}

__device__ __forceinline__ float min3f(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float max3f(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

__device__ __forceinline__ bool boxes_overlap(const Box &a, const Box &b)
{
    return a.mnx <= b.mxx && b.mnx <= a.mxx && a.mny <= b.mxy && b.mny <= a.mxy && a.mnz <= b.mxz && b.mnz <= a.mxz;
}

__device__ __forceinline__ unsigned long long wave_total(unsigned v)
{
    unsigned long long t = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    return t;
}

// this lane's query: the face in leaf slot `slot` of the query index.  live: it takes part
struct FaceQuery
{
    float v[9];
    Box box;
    int32_t id, i0, i1, i2;
    bool live;
};

// slots = 8 nleaves of the query index; faces: self mode only.  An eligible slot holds a face id < F whose indices lie in [0, V) (leaf_kernel)
template <bool SELF>
__device__ __forceinline__ FaceQuery face_query(size_t slot, size_t slots, const Leaf *__restrict__ leaves, const int32_t *__restrict__ faces)
{
    FaceQuery q;
    q.id = -1; q.i0 = 0; q.i1 = 1; q.i2 = 2;
#pragma unroll
    for (int k = 0; k < 9; k++) q.v[k] = 0.0f;
    if (slot < slots)
    {
        const Leaf &lf = leaves[slot / LEAF];
        const int j = (int)(slot % LEAF);
        q.id = lf.id[j];
        if (q.id >= 0)
        {
#pragma unroll
            for (int k = 0; k < 9; k++) q.v[k] = lf.v[j][k];
            if (SELF)
            {
                q.i0 = faces[3 * (size_t)q.id]; q.i1 = faces[3 * (size_t)q.id + 1]; q.i2 = faces[3 * (size_t)q.id + 2];
            }
        }
    }
    q.live = q.id >= 0 && q.i0 != q.i1 && q.i1 != q.i2 && q.i0 != q.i2;
    q.box = {min3f(q.v[0], q.v[3], q.v[6]), min3f(q.v[1], q.v[4], q.v[7]), min3f(q.v[2], q.v[5], q.v[8]),
             max3f(q.v[0], q.v[3], q.v[6]), max3f(q.v[1], q.v[4], q.v[7]), max3f(q.v[2], q.v[5], q.v[8])};
    return q;
}

// FA, FB >= 1.  SELF: the walked index is the query index (leaves_b == leaves_a, FB == FA), count_b is unused.  The grid covers the slots
// of the query index and, for the degenerate count of cross mode, FB lanes.
template <bool SELF>
__global__ void __launch_bounds__(TPB) overlap_kernel(int FA, size_t slots_a, const Leaf *__restrict__ leaves_a, const int32_t *__restrict__ faces, int FB,
                                                       int nleaves_b, int nlevels_b, const Leaf *__restrict__ leaves_b, const Box *__restrict__ nodes_b,
                                                       int32_t *__restrict__ count_a, int32_t *__restrict__ count_b, unsigned long long *__restrict__ stats,
                                                       int capacity, int32_t *__restrict__ pairs, uint8_t *__restrict__ kind, unsigned long long *leaf_visits)
{
    __shared__ WalkShared ws;
    walk_levels(ws, nleaves_b);
    const size_t slot = (size_t)blockIdx.x * TPB + threadIdx.x;
    const FaceQuery q = face_query<SELF>(slot, slots_a, leaves_a, faces);
    const P3 a0 = widen(q.v[0], q.v[1], q.v[2]), a1 = widen(q.v[3], q.v[4], q.v[5]), a2 = widen(q.v[6], q.v[7], q.v[8]);

    // the sorted slots [0, F) hold the F faces of a mesh, the eligible ones first: a slot below F that does not take part is a degenerate face
    unsigned degenerate = (unsigned)(slot < (size_t)FA && !q.live);
    if (!SELF && slot < (size_t)FB) degenerate += (unsigned)(leaves_b[slot / LEAF].id[slot % LEAF] < 0);

    unsigned candidates = 0, adjacent = 0, crossing = 0, coplanar = 0, duplicate = 0, visits = 0;

    if (__ballot(q.live) != 0ull) // wave-uniform
        bvh_walk<false>(
            ws, nlevels_b, nodes_b, [&](int, uint32_t, uint32_t, const Box &b) { return __ballot(q.live && boxes_overlap(q.box, b)) != 0ull; },
            [&](int leaf) {
                visits++;
                for_each_face(leaves_b[leaf], [&](int32_t id, float bx0, float by0, float bz0, float bx1, float by1, float bz1, float bx2, float by2,
                                                  float bz2) {
                    int32_t j0 = 0, j1 = 1, j2 = 2;
                    if (SELF)
                    {
                        j0 = faces[3 * (size_t)id]; j1 = faces[3 * (size_t)id + 1]; j2 = faces[3 * (size_t)id + 2];
                        if (j0 == j1 || j1 == j2 || j0 == j2) return; // wave-uniform: the partner does not take part
                    }
                    const Box pb = {min3f(bx0, bx1, bx2), min3f(by0, by1, by2), min3f(bz0, bz1, bz2),
                                    max3f(bx0, bx1, bx2), max3f(by0, by1, by2), max3f(bz0, bz1, bz2)};
                    if (!q.live || !boxes_overlap(q.box, pb) || (SELF && !(q.id < id))) return;
                    candidates++;
                    int sa = -1, sb = -1, k = 0;
                    if (SELF)
                    {
                        // where each of this face's indices sits in the partner, -1: nowhere.  Both triples are pairwise different
                        const int m0 = q.i0 == j0 ? 0 : (q.i0 == j1 ? 1 : (q.i0 == j2 ? 2 : -1));
                        const int m1 = q.i1 == j0 ? 0 : (q.i1 == j1 ? 1 : (q.i1 == j2 ? 2 : -1));
                        const int m2 = q.i2 == j0 ? 0 : (q.i2 == j1 ? 1 : (q.i2 == j2 ? 2 : -1));
                        const int shared = (int)(m0 >= 0) + (int)(m1 >= 0) + (int)(m2 >= 0);
                        if (shared == 2)
                        {
                            adjacent++;
                            return;
                        }
                        if (shared == 3) k = KIND_DUPLICATE;
                        if (shared == 1)
                        {
                            sa = m0 >= 0 ? 0 : (m1 >= 0 ? 1 : 2);
                            sb = m0 >= 0 ? m0 : (m1 >= 0 ? m1 : m2);
                        }
                    }
                    if (k == 0) k = pair_kind(a0, a1, a2, widen(bx0, by0, bz0), widen(bx1, by1, bz1), widen(bx2, by2, bz2), sa, sb);
                    if (k == 0) return;
                    if (k == KIND_CROSSING)
                    {
                        crossing++;
                        int32_t *other = SELF ? count_a : count_b; // id < the F of that mesh: the build wrote it
                        if (other) atomicAdd(other + id, 1);
                    }
                    else if (k == KIND_COPLANAR) coplanar++;
                    else duplicate++;
                    const unsigned long long at = atomicAdd(stats + S_CURSOR, 1ull);
                    if (at < (unsigned long long)capacity)
                    {
                        pairs[2 * (size_t)at] = q.id; pairs[2 * (size_t)at + 1] = id;
                        kind[at] = (uint8_t)k;
                    }
                });
            },
            NoChildKey());

    // a lane's own hits: q.id < FA.  In self mode partners add to the same word
    if (q.live && crossing) atomicAdd(count_a + q.id, (int32_t)crossing);

    const unsigned long long t_cand = wave_total(candidates), t_adj = wave_total(adjacent), t_cross = wave_total(crossing), t_copl = wave_total(coplanar),
                             t_dup = wave_total(duplicate), t_deg = wave_total(degenerate);
    if ((threadIdx.x & 63) == 0)
    {
        if (t_cand) atomicAdd(stats + S_CANDIDATES, t_cand);
        if (t_adj) atomicAdd(stats + S_ADJACENT, t_adj);
        if (t_cross) atomicAdd(stats + S_CROSSING, t_cross);
        if (t_copl) atomicAdd(stats + S_COPLANAR, t_copl);
        if (t_dup) atomicAdd(stats + S_DUPLICATE, t_dup);
        if (t_deg) atomicAdd(stats + S_DEGENERATE, t_deg);
        if (leaf_visits && visits) atomicAdd(leaf_visits, (unsigned long long)visits);
    }
}

// after the walk: what the list holds, and the cursor's word back to 0
__global__ void finish_stats_kernel(unsigned long long *__restrict__ stats, int capacity)
{
    const unsigned long long total = stats[S_CROSSING] + stats[S_COPLANAR] + stats[S_DUPLICATE];
    stats[S_STORED] = total < (unsigned long long)capacity ? total : (unsigned long long)capacity;
    stats[S_CURSOR] = 0ull;
}

// ---- sort ----------------------------------------------------------------------------------------------------------------------------
struct SortCarve
{
    uint32_t *k[2], *v[2];
    int32_t *pairs;
    uint8_t *kind;
    void *scratch;
    size_t bytes;
};

SortCarve sort_carve(void *ws, int P)
{
    SortCarve c;
    const size_t n = (size_t)(P > 0 ? P : 0);
    char *p = (char *)ts_align_up((size_t)ws);
    auto take = [&](size_t bytes) { char *q = p; p += ts_align_up(bytes); return q; };
    c.k[0] = (uint32_t *)take(n * 4); c.k[1] = (uint32_t *)take(n * 4);
    c.v[0] = (uint32_t *)take(n * 4); c.v[1] = (uint32_t *)take(n * 4);
    c.pairs = (int32_t *)take(n * 8);
    c.kind = (uint8_t *)take(n);
    // the radix sort's tables shrink where its chunk length grows (TS_RS_SMALL_BELOW): never less than just below that size
    size_t sort_bytes = ts_radix_scratch_bytes(n);
    if (n > (size_t)TS_RS_SMALL_BELOW) sort_bytes = std::max(sort_bytes, ts_radix_scratch_bytes((size_t)TS_RS_SMALL_BELOW));
    c.scratch = take(sort_bytes);
    c.bytes = (size_t)(p - (char *)ws);
    return c;
}

// key[j] = column `col` of pair at[j] (at == nullptr: of pair j, and val[j] = j)
__global__ void __launch_bounds__(256) pair_keys_kernel(int P, const int32_t *__restrict__ pairs, int col, const uint32_t *__restrict__ at,
                                                         uint32_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P) return;
    const uint32_t src = at ? at[j] : (uint32_t)j; // a value of the sort: < P
    key[j] = (uint32_t)pairs[2 * (size_t)src + col];
    if (!at) val[j] = (uint32_t)j;
}

__global__ void __launch_bounds__(256) gather_pairs_kernel(int P, const uint32_t *__restrict__ at, const int32_t *__restrict__ pairs,
                                                            const uint8_t *__restrict__ kind, int32_t *__restrict__ pairs_out, uint8_t *__restrict__ kind_out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P) return;
    const uint32_t src = at[j]; // < P
    pairs_out[2 * (size_t)j] = pairs[2 * (size_t)src]; pairs_out[2 * (size_t)j + 1] = pairs[2 * (size_t)src + 1];
    kind_out[j] = kind[src];
}
} // namespace

size_t ts_overlap_bvh_bytes(int F) { return bvh_view(nullptr, F).bytes; }

size_t ts_overlap_sort_workspace_bytes(int P) { return sort_carve(nullptr, P).bytes + TS_ALIGN; }

hipError_t ts_overlap_query(int FA, const void *bvh_a, const int32_t *faces, int FB, const void *bvh_b, int32_t *count_a, int32_t *count_b,
                            uint64_t *stats, int capacity, int32_t *pairs, uint8_t *kind, unsigned long long *leaf_visits, hipStream_t s)
{
    const bool self = faces != nullptr;
    hipError_t e = mesh_fill(stats, 0, 8 * sizeof(uint64_t), s);
    if (e == hipSuccess && FA > 0) e = mesh_fill(count_a, 0, (size_t)FA * sizeof(int32_t), s);
    if (e == hipSuccess && !self && count_b && FB > 0) e = mesh_fill(count_b, 0, (size_t)FB * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    if (FA <= 0 || (!self && FB <= 0)) return hipSuccess;
    const BvhView a = bvh_view(const_cast<void *>(bvh_a), FA);
    const BvhView b = self ? a : bvh_view(const_cast<void *>(bvh_b), FB);
    const size_t slots = (size_t)a.nleaves * LEAF, lanes = self ? slots : std::max(slots, (size_t)FB);
    const dim3 grid((unsigned)((lanes + TPB - 1) / TPB));
    unsigned long long *st = (unsigned long long *)stats;
    if (self)
        hipLaunchKernelGGL(overlap_kernel<true>, grid, dim3(TPB), 0, s, FA, slots, a.leaves, faces, FA, a.nleaves, a.nlevels, a.leaves, a.nodes, count_a,
                           (int32_t *)nullptr, st, capacity, pairs, kind, leaf_visits);
    else
        hipLaunchKernelGGL(overlap_kernel<false>, grid, dim3(TPB), 0, s, FA, slots, a.leaves, (const int32_t *)nullptr, FB, b.nleaves, b.nlevels, b.leaves,
                           b.nodes, count_a, count_b, st, capacity, pairs, kind, leaf_visits);
    hipLaunchKernelGGL(finish_stats_kernel, dim3(1), dim3(1), 0, s, st, capacity);
    return hipGetLastError();
}

hipError_t ts_overlap_sort_pairs(int P, int bits_first, int bits_second, int32_t *pairs, uint8_t *kind, void *ws, hipStream_t s)
{
    if (P <= 0) return hipSuccess;
    const SortCarve c = sort_carve(ws, P);
    const unsigned nb = (unsigned)(((size_t)P + 255) / 256);
    hipLaunchKernelGGL(pair_keys_kernel, dim3(nb), dim3(256), 0, s, P, pairs, 1, (const uint32_t *)nullptr, c.k[0], c.v[0]);
    const int at = ts_radix_sort_pairs(c.k, c.v, (size_t)P, bits_second, c.scratch, s); // by the second entry, stable
    hipLaunchKernelGGL(pair_keys_kernel, dim3(nb), dim3(256), 0, s, P, pairs, 0, c.v[at], c.k[at ^ 1], (uint32_t *)nullptr);
    // the gathered first entries are the next keys; the values stay where the first sort left them
    uint32_t *const k2[2] = {c.k[at ^ 1], c.k[at]}, *const v2[2] = {c.v[at], c.v[at ^ 1]};
    const int at2 = ts_radix_sort_pairs(k2, v2, (size_t)P, bits_first, c.scratch, s); // then by the first, stable: (first, second) order
    hipLaunchKernelGGL(gather_pairs_kernel, dim3(nb), dim3(256), 0, s, P, v2[at2], pairs, kind, c.pairs, c.kind);
    hipError_t e = mesh_copy(pairs, c.pairs, (size_t)P * 8, s);
    if (e == hipSuccess) e = mesh_copy(kind, c.kind, (size_t)P, s);
    return e == hipSuccess ? hipGetLastError() : e;
}
