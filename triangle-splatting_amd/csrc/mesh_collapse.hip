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
//
// Shared with mesh_decimate.hip through csrc/ts_collapse_round.h, defined there once: records_kernel (face_takes_part(), half_edge_records()),
// edge_flags_kernel, vertex_class_kernel, direction_guards, priority, table_has, apply_kernel, and the bodies of the selection over an
// order -- best_of_edges, best_of_ring, decide_winner (count_into() of the winners).  This unit's order is LengthOrder below.
#include "ts_collapse_launch.h"
#include "ts_mesh_edge_ids.h"
#include "ts_collapse_round.h"

namespace
{
constexpr uint8_t LONG_ENOUGH = 2; // TSP_LONG_ENOUGH; the other states, the guard bits and TSP_MAX_RING: csrc/ts_collapse_round.h
constexpr int MARK_SHORTER = 1;    // TSP_MARK_SHORTER; anything else is TSP_MARK_VERTEX_LIMIT (api_collapse.hip checks)

// ---- the first kernel of the round -------------------------------------------------------------------------------------------------------
// One workgroup: the four counters and the workspace's edge count (read as E = 0 where the front does not run) start at zero.
__global__ void __launch_bounds__(64) begin_kernel(unsigned long long *totals, uint32_t *total)
{
    if (threadIdx.x < 4) totals[threadIdx.x] = 0ull;
    if (total && threadIdx.x < 4) total[threadIdx.x] = 0u;
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
// (length2 ascending, priority descending, edge id ascending); NONE comes last
struct LengthOrder
{
    const double *cand_l2;
    const uint32_t *prio;
    __device__ __forceinline__ bool comes_first(uint32_t a, uint32_t b) const
    {
        if (a == NONE || a == b) return false;
        if (b == NONE) return true;
        const double la = cand_l2[a], lb = cand_l2[b];
        if (la != lb) return la < lb;
        const uint32_t pa = prio[a], pb = prio[b];
        if (pa != pb) return pa > pb;
        return a < b;
    }
};

// One thread = one vertex: the first candidate among the edges at it (best_of_edges).
__global__ void __launch_bounds__(256) best_kernel(int V, Rings g, const int32_t *__restrict__ half_edge_edge, const uint8_t *__restrict__ edge_state,
                                                    LengthOrder order, uint32_t *__restrict__ best)
{
    best_of_edges(V, g, half_edge_edge, edge_state, order, best);
}

// One thread = one vertex: the first among best[u] over v and the vertices adjacent to it (best_of_ring).
__global__ void __launch_bounds__(256) best2_kernel(int V, const int32_t *__restrict__ faces, Rings g, LengthOrder order,
                                                     const uint32_t *__restrict__ best, uint32_t *__restrict__ best2)
{
    best_of_ring(V, faces, g, order, best, best2);
}

// One thread = one edge slot (decide_winner): the winners count into totals[3] through count_into().
__global__ void __launch_bounds__(256) winners_kernel(size_t N, const uint32_t *__restrict__ total, const int32_t *__restrict__ edge_vertices,
                                                       const int32_t *__restrict__ edge_removed, const uint32_t *__restrict__ best2,
                                                       uint8_t *__restrict__ edge_state, int32_t *__restrict__ vertex_target,
                                                       unsigned long long *totals)
{
    decide_winner(N, total, edge_vertices, edge_removed, best2, edge_state, vertex_target, totals + 3);
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
        const Rings g{t.ring_val, c.ring_start, c.ring_end};
        const LengthOrder order{c.cand_l2, c.prio};
        hipLaunchKernelGGL(best_kernel, dim3(nv), dim3(256), 0, s, V, g, (const int32_t *)c.ids.half_edge_edge, (const uint8_t *)edge_state, order,
                           c.best);
        hipLaunchKernelGGL(best2_kernel, dim3(nv), dim3(256), 0, s, V, faces, g, order, (const uint32_t *)c.best, c.best2);
        hipLaunchKernelGGL(winners_kernel, dim3(nh), dim3(256), 0, s, N, (const uint32_t *)c.ids.total, (const int32_t *)edge_vertices,
                           (const int32_t *)edge_removed, (const uint32_t *)c.best2, edge_state, vertex_target, totals);
    }
    if (out_faces)
        hipLaunchKernelGGL(apply_kernel, dim3(nf), dim3(256), 0, s, V, F, faces, keep, (const int32_t *)vertex_target, out_faces, out_keep);
    return hipGetLastError();
}
