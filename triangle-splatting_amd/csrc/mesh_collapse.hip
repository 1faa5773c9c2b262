// mesh_collapse.hip -- one round of half-edge collapses of the short edges of an indexed mesh (include/ts_collapse.h).
//
// The arithmetic is float64 on the fp32 inputs widened, every operation rounded: the unit is built with -ffp-contract=off.  The only atomics
// are the integer adds of the counters.  The unit clears and copies nothing with a fill or a copy: every output element is written by the
// kernel that owns its index, and the four counters are cleared by the first kernel of the round (begin_kernel), in stream order.
//
// Edges.  The sort-by-edge front (csrc/ts_mesh_edges.h) leaves the half-edges of the faces that take part in (lo, hi) order;
// csrc/ts_mesh_edge_ids.h numbers the edges, bounds their runs and hands the ids to the half-edges.
//
// Rings.  One more stable radix sort orders the 3 F corner records by their vertex (the sentinel key V for a face that does not take part):
// the ring of v is the run of key v, found by two binary searches of the vertex's own thread.  Rings are walked, never stored: a per-thread
// array indexed at run time would go to scratch.
//
// Round.  One thread per edge flags the clean edges; one per vertex decides FREE or HELD; one per edge slot classifies -- only a short
// eligible edge walks a ring, at most two of at most TSP_MAX_RING corners -- one per vertex takes the best candidate among its edges, one
// per vertex the best among its closed ring; one per edge decides the winners and writes vertex_target; one per face maps its indices.
#include "ts_collapse_launch.h"
#include "ts_mesh_edge_ids.h"

namespace
{
constexpr uint8_t NO_EDGE = 0, NOT_ELIGIBLE = 1, LONG_ENOUGH = 2, GUARDED = 3, LOST = 4, COLLAPSED = 5; // TSP_*
constexpr uint8_t GUARD_LINK = 1, GUARD_LONG = 2, GUARD_NORMAL = 4, GUARD_HELD = 8;                    // TSP_GUARD_*
constexpr int MARK_SHORTER = 1;     // TSP_MARK_SHORTER; anything else is TSP_MARK_VERTEX_LIMIT (api_collapse.hip checks)
constexpr uint32_t MAX_RING = 64;   // TSP_MAX_RING
constexpr uint32_t NONE = 0xFFFFFFFFu; // no candidate
constexpr uint8_t HELD = 0, FREE = 1;

// ---- the first kernel of the round -------------------------------------------------------------------------------------------------------
// One workgroup: the four counters and the workspace's edge count (read as E = 0 where the front does not run) start at zero.
__global__ void __launch_bounds__(64) begin_kernel(unsigned long long *totals, uint32_t *total)
{
    if (threadIdx.x < 4) totals[threadIdx.x] = 0ull;
    if (total && threadIdx.x < 4) total[threadIdx.x] = 0u;
}

// One thread = one vertex, where there are no faces: nothing collapses.
__global__ void __launch_bounds__(256) identity_kernel(int V, int32_t *__restrict__ vertex_target)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < V) vertex_target[v] = v;
}

// One thread = one face: its three half-edge records and its three corner records (key: the corner's vertex).
__global__ void __launch_bounds__(256) records_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep,
                                                       uint32_t *__restrict__ key, uint32_t *__restrict__ val, uint32_t *__restrict__ ring_key,
                                                       uint32_t *__restrict__ ring_val)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int32_t v[3];
    const bool ok = face_takes_part(V, (size_t)f, faces, keep, v);
    half_edge_records(V, (size_t)f, ok, v, key, val);
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const size_t c = 3 * (size_t)f + k;
        ring_key[c] = ok ? (uint32_t)v[k] : (uint32_t)V;
        ring_val[c] = (uint32_t)c;
    }
}

// One thread = one edge below E: clean iff its run holds two half-edges that leave different vertices.
__global__ void __launch_bounds__(256) edge_flags_kernel(size_t N, const int32_t *__restrict__ faces, const uint32_t *__restrict__ sval,
                                                          const uint32_t *__restrict__ start, const uint32_t *__restrict__ end,
                                                          const uint32_t *__restrict__ total, uint8_t *__restrict__ clean)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N || e >= (size_t)*total) return;
    const uint32_t j = start[e];
    clean[e] = end[e] - j == 2 && faces[sval[j]] != faces[sval[j + 1]];
}

// the first position of the N ascending keys that is not below `want`
__device__ __forceinline__ uint32_t lower_bound(size_t N, const uint32_t *__restrict__ keys, uint32_t want)
{
    size_t l = 0, r = N;
    while (l < r)
    {
        const size_t mid = l + (r - l) / 2;
        if (keys[mid] < want) l = mid + 1;
        else r = mid;
    }
    return (uint32_t)l;
}

__device__ __forceinline__ uint32_t prev_corner(uint32_t c) { return c % 3u == 0u ? c + 2u : c - 1u; }

// One thread = one vertex: the bounds of its ring among the sorted corners, its class, and vertex_target's identity.  A corner of the ring
// belongs to a face that takes part, so both half-edges at it carry an edge id in [0, E).
__global__ void __launch_bounds__(256) vertex_class_kernel(int V, size_t N, const float *__restrict__ vertices, const uint8_t *__restrict__ pinned,
                                                            const uint32_t *__restrict__ ring_key, const uint32_t *__restrict__ ring_val,
                                                            const int32_t *__restrict__ half_edge_edge, const uint8_t *__restrict__ clean,
                                                            uint32_t *__restrict__ ring_start, uint32_t *__restrict__ ring_end,
                                                            uint8_t *__restrict__ vclass, int32_t *__restrict__ vertex_target)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const uint32_t rs = lower_bound(N, ring_key, (uint32_t)v), re = lower_bound(N, ring_key, (uint32_t)v + 1u);
    ring_start[v] = rs; ring_end[v] = re;
    const float *p = vertices + 3 * (size_t)v;
    bool is_free = re > rs && re - rs <= MAX_RING && finite32(p[0]) && finite32(p[1]) && finite32(p[2]) && !(pinned && pinned[v]);
    if (is_free)
        for (uint32_t j = rs; j < re; j++)
        {
            const uint32_t h = ring_val[j];
            is_free = is_free && clean[half_edge_edge[h]] && clean[half_edge_edge[prev_corner(h)]];
        }
    vclass[v] = is_free ? FREE : HELD;
    if (vertex_target) vertex_target[v] = v;
}

// ---- the guards --------------------------------------------------------------------------------------------------------------------------
struct D3
{
    double x, y, z;
};
__device__ __forceinline__ D3 sub(const D3 &p, const D3 &q) { return {p.x - q.x, p.y - q.y, p.z - q.z}; }
__device__ __forceinline__ double dot(const D3 &s, const D3 &t) { return (s.x * t.x + s.y * t.y) + s.z * t.z; }
__device__ __forceinline__ D3 cross(const D3 &s, const D3 &t) { return {s.y * t.z - s.z * t.y, s.z * t.x - s.x * t.z, s.x * t.y - s.y * t.x}; }

__device__ __forceinline__ D3 row(const float *__restrict__ vertices, int32_t i)
{
    const float *p = vertices + 3 * (size_t)i;
    return {(double)p[0], (double)p[1], (double)p[2]};
}
__device__ __forceinline__ bool finite_row(const float *__restrict__ vertices, int32_t i)
{
    const float *p = vertices + 3 * (size_t)i;
    return finite32(p[0]) && finite32(p[1]) && finite32(p[2]);
}

// length2 of include/ts_collapse.h: from the smaller index to the larger
__device__ __forceinline__ double length2(int32_t i, const D3 &pi, int32_t j, const D3 &pj)
{
    const D3 d = i < j ? sub(pj, pi) : sub(pi, pj);
    return (d.x * d.x + d.y * d.y) + d.z * d.z;
}

// is (m, M) among the N sorted positions?  The sentinels (V, V) sort last and equal no pair of vertices.
__device__ __forceinline__ bool table_has(size_t N, const uint32_t *__restrict__ smin, const uint32_t *__restrict__ smax, uint32_t m, uint32_t M)
{
    size_t l = 0, r = N;
    while (l < r)
    {
        const size_t mid = l + (r - l) / 2;
        const uint32_t a = smin[mid], b = smax[mid];
        if (a < m || (a == m && b < M)) l = mid + 1;
        else r = mid;
    }
    return l < N && smin[l] == m && smax[l] == M;
}

__device__ __forceinline__ uint32_t priority(uint32_t lo, uint32_t hi, uint32_t seed)
{
    uint32_t h = seed * 0x9E3779B1u + lo;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h += hi; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

struct Table // the sorted half-edges and the sorted corners
{
    size_t N;
    const uint32_t *smin, *smax, *ring_val;
};

// The guards of the direction r -> k over the whole ring [rs, re) of a FREE r, without early exit: the mask of those that fail.  Every
// corner of the ring belongs to a face that takes part, so x and y are in [0, V).
__device__ __forceinline__ uint8_t direction_guards(const Table &t, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                    uint32_t rs, uint32_t re, int32_t k, int32_t c, int32_t d, const D3 &pr, const D3 &pk,
                                                    double max2, double M)
{
    uint8_t mask = 0;
    for (uint32_t j = rs; j < re; j++)
    {
        const uint32_t h = t.ring_val[j];
        const int32_t x = faces[next_corner(h)], y = faces[next_corner(next_corner(h))];
        if (x == k) continue; // the face on the edge where k follows r; the other one has y == k
        const D3 px = row(vertices, x);
        if (x != c && x != d && table_has(t.N, t.smin, t.smax, (uint32_t)min(x, k), (uint32_t)max(x, k))) mask |= GUARD_LINK;
        if (!(length2(k, pk, x, px) <= max2)) mask |= GUARD_LONG;
        if (y == k) continue;
        if ((x == c && y == d) || (x == d && y == c)) mask |= GUARD_LINK;
        const D3 py = row(vertices, y);
        const D3 n0 = cross(sub(px, pr), sub(py, pr)), n1 = cross(sub(px, pk), sub(py, pk));
        const double Q0 = dot(n0, n0), Q1 = dot(n1, n1), D = dot(n0, n1);
        if (!(Q1 > 0.0 && (Q0 == 0.0 || (D > 0.0 && D * D >= (M * Q0) * Q1)))) mask |= GUARD_NORMAL;
    }
    return mask;
}

struct ShortRule
{
    int mode;                  // TSP_MARK_*
    double min2, max2, M;      // (double)min_edge squared, (double)max_edge squared, (double)min_cos squared
    const float *vertex_limit; // V floats in TSP_MARK_VERTEX_LIMIT
};

// One thread = one edge slot, e < N = 3 F.  Below E (*total): lo and hi from the head of the run (both in [0, V): the face took part); a run
// of two holds the half-edges sval[j] < sval[j + 1], both below N, whose faces took part: every vertex index read is in [0, V).  Past E: the
// fill values.  A candidate leaves as LOST with its length2 and its priority; winners_kernel promotes it.
__global__ void __launch_bounds__(256) classify_kernel(Table t, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                        const uint32_t *__restrict__ sval, const uint32_t *__restrict__ start,
                                                        const uint32_t *__restrict__ end, const uint32_t *__restrict__ total,
                                                        const uint8_t *__restrict__ vclass, const uint32_t *__restrict__ ring_start,
                                                        const uint32_t *__restrict__ ring_end, ShortRule rule, uint32_t seed,
                                                        int32_t *__restrict__ edge_vertices, uint8_t *__restrict__ edge_state,
                                                        int32_t *__restrict__ edge_removed, uint8_t *__restrict__ edge_guard,
                                                        double *__restrict__ cand_l2, uint32_t *__restrict__ prio, unsigned long long *totals)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t n[4] = {0, 0, 0, 0};
    if (e < t.N)
    {
        int32_t lo = -1, hi = -1, removed = -1;
        uint8_t state = NO_EDGE, mask = 0;
        if (e < (size_t)*total)
        {
            const uint32_t j = start[e];
            lo = (int32_t)t.smin[j]; hi = (int32_t)t.smax[j];
            state = NOT_ELIGIBLE;
            n[0] = 1;
            const bool lo_free = vclass[lo] == FREE, hi_free = vclass[hi] == FREE;
            if (end[e] - j == 2 && (lo_free || hi_free))
            {
                uint32_t h0 = sval[j], h1 = sval[j + 1];
                const int32_t from0 = faces[h0], from1 = faces[h1];
                if (from0 != from1) // opposite directions
                {
                    if (from0 != lo) { const uint32_t s = h0; h0 = h1; h1 = s; } // h0 runs lo -> hi
                    const int32_t c = faces[next_corner(next_corner(h0))], d = faces[next_corner(next_corner(h1))];
                    if (c != d && finite_row(vertices, lo) && finite_row(vertices, hi) && finite_row(vertices, c) && finite_row(vertices, d))
                    {
                        state = LONG_ENOUGH;
                        const D3 plo = row(vertices, lo), phi = row(vertices, hi);
                        const double l2 = length2(lo, plo, hi, phi);
                        bool is_short;
                        if (rule.mode == MARK_SHORTER) is_short = l2 < rule.min2;
                        else
                        {
                            const float la = rule.vertex_limit[lo], lb = rule.vertex_limit[hi];
                            const double L = (double)(lb < la ? lb : la);
                            is_short = la == la && lb == lb && l2 < L * L;
                        }
                        if (is_short)
                        {
                            state = GUARDED;
                            n[1] = 1;
                            if (hi_free)
                            {
                                const uint8_t g = direction_guards(t, vertices, faces, ring_start[hi], ring_end[hi], lo, c, d, phi, plo, rule.max2, rule.M);
                                if (g == 0) removed = hi;
                                mask |= g;
                            }
                            else mask |= GUARD_HELD;
                            if (removed < 0)
                            {
                                if (lo_free)
                                {
                                    const uint8_t g = direction_guards(t, vertices, faces, ring_start[lo], ring_end[lo], hi, c, d, plo, phi, rule.max2, rule.M);
                                    if (g == 0) removed = lo;
                                    mask |= g;
                                }
                                else mask |= GUARD_HELD;
                            }
                            if (removed >= 0)
                            {
                                state = LOST;
                                n[2] = 1;
                                cand_l2[e] = l2;
                                prio[e] = priority((uint32_t)lo, (uint32_t)hi, seed);
                            }
                        }
                    }
                }
            }
        }
        edge_vertices[2 * e] = lo; edge_vertices[2 * e + 1] = hi;
        edge_state[e] = state;
        edge_removed[e] = removed;
        edge_guard[e] = mask;
    }
    count4_into(totals, n);
}

// ---- selection ---------------------------------------------------------------------------------------------------------------------------
// does candidate a come before candidate b?  (length2 ascending, priority descending, edge id ascending); NONE comes last
__device__ __forceinline__ bool comes_first(uint32_t a, uint32_t b, const double *__restrict__ cand_l2, const uint32_t *__restrict__ prio)
{
    if (a == NONE || a == b) return false;
    if (b == NONE) return true;
    const double la = cand_l2[a], lb = cand_l2[b];
    if (la != lb) return la < lb;
    const uint32_t pa = prio[a], pb = prio[b];
    if (pa != pb) return pa > pb;
    return a < b;
}

// One thread = one vertex: the first candidate among the edges at it.  Every edge at v lies in a ring face of v, as the half-edge that leaves
// v or the one that arrives.
__global__ void __launch_bounds__(256) best_kernel(int V, const uint32_t *__restrict__ ring_val, const uint32_t *__restrict__ ring_start,
                                                    const uint32_t *__restrict__ ring_end, const int32_t *__restrict__ half_edge_edge,
                                                    const uint8_t *__restrict__ edge_state, const double *__restrict__ cand_l2,
                                                    const uint32_t *__restrict__ prio, uint32_t *__restrict__ best)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    uint32_t b = NONE;
    for (uint32_t j = ring_start[v], re = ring_end[v]; j < re; j++)
    {
        const uint32_t h = ring_val[j];
        const uint32_t e0 = (uint32_t)half_edge_edge[h], e1 = (uint32_t)half_edge_edge[prev_corner(h)];
        if (edge_state[e0] == LOST && comes_first(e0, b, cand_l2, prio)) b = e0;
        if (edge_state[e1] == LOST && comes_first(e1, b, cand_l2, prio)) b = e1;
    }
    best[v] = b;
}

// One thread = one vertex: the first among best[u] over v and the vertices adjacent to it, the two other corners of every ring face.
__global__ void __launch_bounds__(256) best2_kernel(int V, const int32_t *__restrict__ faces, const uint32_t *__restrict__ ring_val,
                                                     const uint32_t *__restrict__ ring_start, const uint32_t *__restrict__ ring_end,
                                                     const double *__restrict__ cand_l2, const uint32_t *__restrict__ prio,
                                                     const uint32_t *__restrict__ best, uint32_t *__restrict__ best2)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    uint32_t b = best[v];
    for (uint32_t j = ring_start[v], re = ring_end[v]; j < re; j++)
    {
        const uint32_t h = ring_val[j];
        const uint32_t bx = best[faces[next_corner(h)]], by = best[faces[next_corner(next_corner(h))]];
        if (comes_first(bx, b, cand_l2, prio)) b = bx;
        if (comes_first(by, b, cand_l2, prio)) b = by;
    }
    best2[v] = b;
}

// One thread = one edge slot: a candidate that is the first of the closed rings of both its ends collapses.  Every lane reaches count_into.
__global__ void __launch_bounds__(256) winners_kernel(size_t N, const uint32_t *__restrict__ total, const int32_t *__restrict__ edge_vertices,
                                                       const int32_t *__restrict__ edge_removed, const uint32_t *__restrict__ best2,
                                                       uint8_t *__restrict__ edge_state, int32_t *__restrict__ vertex_target,
                                                       unsigned long long *totals)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t won = 0;
    if (e < N && e < (size_t)*total && edge_state[e] == LOST)
    {
        const int32_t lo = edge_vertices[2 * e], hi = edge_vertices[2 * e + 1];
        if (best2[lo] == (uint32_t)e && best2[hi] == (uint32_t)e)
        {
            won = 1;
            edge_state[e] = COLLAPSED;
            const int32_t r = edge_removed[e];
            if (vertex_target) vertex_target[r] = r == lo ? hi : lo;
        }
    }
    count_into(totals + 3, won);
}

// ---- the collapse ------------------------------------------------------------------------------------------------------------------------
// One thread = one face.  A face that takes part maps its indices through vertex_target; two equal indices delete it.
__global__ void __launch_bounds__(256) apply_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep,
                                                     const int32_t *__restrict__ vertex_target, int32_t *__restrict__ out_faces,
                                                     uint8_t *__restrict__ out_keep)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const size_t at = 3 * (size_t)f;
    const int32_t a = faces[at], b = faces[at + 1], c = faces[at + 2];
    int32_t v[3];
    int32_t o0 = a, o1 = b, o2 = c;
    uint8_t kept = !keep || keep[f];
    if (face_takes_part(V, (size_t)f, faces, keep, v))
    {
        const int32_t m0 = vertex_target[a], m1 = vertex_target[b], m2 = vertex_target[c];
        if (m0 == m1 || m1 == m2 || m0 == m2) kept = 0;
        else { o0 = m0; o1 = m1; o2 = m2; }
    }
    out_faces[at] = o0; out_faces[at + 1] = o1; out_faces[at + 2] = o2;
    out_keep[f] = kept;
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------
struct CollapseCarve
{
    EdgeSortCarve sort;
    EdgeIdCarve ids;
    uint32_t *rk[2], *rv[2]; // the corner records, N words each
    uint32_t *prio, *ring_start, *ring_end, *best, *best2;
    double *cand_l2;
    uint8_t *clean, *vclass;
    size_t bytes;
};
CollapseCarve collapse_carve(void *ws, size_t V, size_t F)
{
    CollapseCarve c;
    Carver w(ws);
    const size_t N = 3 * F;
    c.sort = edge_sort_carve(w, N);
    c.ids = edge_id_carve(w, N);
    c.rk[0] = w.words(N); c.rk[1] = w.words(N); c.rv[0] = w.words(N); c.rv[1] = w.words(N);
    c.prio = w.words(N);
    c.cand_l2 = (double *)w.bytes(N * sizeof(double));
    c.clean = (uint8_t *)w.bytes(N);
    c.ring_start = w.words(V); c.ring_end = w.words(V); c.best = w.words(V); c.best2 = w.words(V);
    c.vclass = (uint8_t *)w.bytes(V);
    c.bytes = w.used();
    return c;
}
} // namespace

size_t ts_collapse_workspace_bytes(int V, int F)
{
    return collapse_carve(nullptr, (size_t)(V > 0 ? V : 0), (size_t)(F > 0 ? F : 0)).bytes + 2 * TS_ALIGN;
}

hipError_t ts_collapse_round(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, const uint8_t *pinned, int mode,
                             float min_edge, const float *vertex_limit, float max_edge, float min_cos, uint32_t seed, int32_t *out_faces,
                             uint8_t *out_keep, int32_t *vertex_target, int32_t *edge_vertices, uint8_t *edge_state, int32_t *edge_removed,
                             uint8_t *edge_guard, unsigned long long *totals, void *ws, hipStream_t s)
{
    const size_t f = (size_t)(F > 0 ? F : 0), N = 3 * f;
    const CollapseCarve c = collapse_carve(F > 0 ? ws : nullptr, (size_t)V, f);
    const unsigned nf = blocks256(f), nh = blocks256(N), nv = blocks256((size_t)V);
    hipLaunchKernelGGL(begin_kernel, dim3(1), dim3(64), 0, s, totals, F > 0 ? c.ids.total : nullptr);
    if (F <= 0)
    {
        if (V > 0 && vertex_target) hipLaunchKernelGGL(identity_kernel, dim3(nv), dim3(256), 0, s, V, vertex_target); // no ring, no class
        return hipGetLastError();
    }
    Table t{N, nullptr, nullptr, nullptr};
    const uint32_t *sval = nullptr;
    if (V > 0)
    {
        hipLaunchKernelGGL(records_kernel, dim3(nf), dim3(256), 0, s, V, F, faces, keep, c.sort.k[0], c.sort.v[0], c.rk[0], c.rv[0]);
        const SortedEdges edges = sort_half_edges(V, N, faces, c.sort, s);
        number_edges(V, N, edges, c.ids, s);
        const int at = ts_radix_sort_pairs(c.rk, c.rv, N, bit_length((uint32_t)V), c.sort.scratch, s); // the corners by vertex, stable
        t = Table{N, edges.smin, edges.smax, c.rv[at]};
        sval = edges.sval;
        hipLaunchKernelGGL(edge_flags_kernel, dim3(nh), dim3(256), 0, s, N, faces, sval, (const uint32_t *)c.ids.start, (const uint32_t *)c.ids.end,
                           (const uint32_t *)c.ids.total, c.clean);
        hipLaunchKernelGGL(vertex_class_kernel, dim3(nv), dim3(256), 0, s, V, N, vertices, pinned, (const uint32_t *)c.rk[at], t.ring_val,
                           (const int32_t *)c.ids.half_edge_edge, (const uint8_t *)c.clean, c.ring_start, c.ring_end, c.vclass, vertex_target);
    }
    const double lmin = (double)min_edge, lmax = (double)max_edge, m = (double)min_cos;
    const ShortRule rule{mode, lmin * lmin, lmax * lmax, m * m, vertex_limit};
    // with V == 0 the edge count is the zero of begin_kernel: every slot writes its fill values and reads nothing else
    hipLaunchKernelGGL(classify_kernel, dim3(nh), dim3(256), 0, s, t, vertices, faces, sval, (const uint32_t *)c.ids.start,
                       (const uint32_t *)c.ids.end, (const uint32_t *)c.ids.total, (const uint8_t *)c.vclass, (const uint32_t *)c.ring_start,
                       (const uint32_t *)c.ring_end, rule, seed, edge_vertices, edge_state, edge_removed, edge_guard, c.cand_l2, c.prio, totals);
    if (V > 0)
    {
        hipLaunchKernelGGL(best_kernel, dim3(nv), dim3(256), 0, s, V, t.ring_val, (const uint32_t *)c.ring_start, (const uint32_t *)c.ring_end,
                           (const int32_t *)c.ids.half_edge_edge, (const uint8_t *)edge_state, (const double *)c.cand_l2, (const uint32_t *)c.prio,
                           c.best);
        hipLaunchKernelGGL(best2_kernel, dim3(nv), dim3(256), 0, s, V, faces, t.ring_val, (const uint32_t *)c.ring_start,
                           (const uint32_t *)c.ring_end, (const double *)c.cand_l2, (const uint32_t *)c.prio, (const uint32_t *)c.best, c.best2);
        hipLaunchKernelGGL(winners_kernel, dim3(nh), dim3(256), 0, s, N, (const uint32_t *)c.ids.total, (const int32_t *)edge_vertices,
                           (const int32_t *)edge_removed, (const uint32_t *)c.best2, edge_state, vertex_target, totals);
    }
    if (out_faces)
        hipLaunchKernelGGL(apply_kernel, dim3(nf), dim3(256), 0, s, V, F, faces, keep, (const int32_t *)vertex_target, out_faces, out_keep);
    return hipGetLastError();
}
