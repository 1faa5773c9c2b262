// mesh_decimate.hip -- one round of half-edge collapses ordered by quadric error, with a budget, and the vertex quadrics that feed and
// follow it (include/ts_decimate.h).
//
// The arithmetic is float64 on the fp32 inputs widened, every operation rounded: the unit is built with -ffp-contract=off.  The only atomics
// are the integer adds of the counters.  The unit clears and copies nothing with a fill or a copy: every output element is written by the
// kernel that owns its index, and the five counters are cleared by the first kernel of the round (begin_kernel), in stream order.
//
// The front -- half-edge and corner records, the sort by edge, the edge ids, the sort of the corners by vertex, the clean-edge flags, the
// vertex classes -- and the guards, the priority, the selection and the face map are mesh_collapse.hip's, shared through
// csrc/ts_collapse_round.h.  This unit's own: the quadric accumulation (one thread per vertex walking its ring), the classification of both
// directions with their costs, the ranking, and the quadric merge.
//
// Ranking.  Three stable 32-bit radix sorts over the 3 F edge slots, least significant key first: the inverted priority, the low word of
// the cost, the high word of the cost.  A slot without a candidate carries all ones in every key: above the high word of every finite cost,
// so the candidates come first and the position of a candidate is its rank.  The slots start in edge order and the sorts are stable, so
// equal (cost, priority) fall back to the edge id.
//
// A quadric is held in ten named scalars (Quadric), never in a per-thread array indexed at run time: that would go to scratch.
#include "ts_decimate_launch.h"
#include "ts_collapse_round.h"

namespace
{
constexpr uint8_t TOO_COSTLY = 2, DEFERRED = 6; // TSZ_*; the other states, the guard bits and the ring bound: csrc/ts_collapse_round.h

// ---- the first kernel of the round -------------------------------------------------------------------------------------------------------
// One workgroup: the five counters and the workspace's edge count (read as E = 0 where the front does not run) start at zero.
__global__ void __launch_bounds__(64) begin_kernel(unsigned long long *totals, uint32_t *total)
{
    if (threadIdx.x < 5) totals[threadIdx.x] = 0ull;
    if (total && threadIdx.x < 4) total[threadIdx.x] = 0u;
}

// ---- quadrics ----------------------------------------------------------------------------------------------------------------------------
struct Quadric // a00 a01 a02 a11 a12 a22 b0 b1 b2 c, in the vertex's own frame
{
    double a00, a01, a02, a11, a12, a22, b0, b1, b2, c;
};
__device__ __forceinline__ Quadric load_quadric(const double *__restrict__ q, int32_t v)
{
    const double *p = q + 10 * (size_t)v;
    return {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]};
}

// A_r d per row, and cost_r = (dot(d, A_r d) + (dot(b_r, d) + dot(b_r, d))) + c_r, unclamped
__device__ __forceinline__ double cost_of_removed(const Quadric &q, const D3 &d, D3 &Ad)
{
    Ad.x = (q.a00 * d.x + q.a01 * d.y) + q.a02 * d.z;
    Ad.y = (q.a01 * d.x + q.a11 * d.y) + q.a12 * d.z;
    Ad.z = (q.a02 * d.x + q.a12 * d.y) + q.a22 * d.z;
    const D3 b{q.b0, q.b1, q.b2};
    const double bd = dot(b, d);
    return (dot(d, Ad) + (bd + bd)) + q.c;
}

// The cost of r -> k: false if it is not finite; a negative cost and -0 become +0.
__device__ __forceinline__ bool direction_cost(const double *__restrict__ quadrics, int32_t r, int32_t k, const D3 &pr, const D3 &pk, double &cost)
{
    const Quadric q = load_quadric(quadrics, r);
    D3 Ad;
    const double c = cost_of_removed(q, sub(pk, pr), Ad) + quadrics[10 * (size_t)k + 9];
    if (!finite64(c)) return false;
    cost = c > 0.0 ? c : 0.0;
    return true;
}

// One thread = one vertex: its ring among the sorted corners, walked in ascending corner index; every ring face whose nine coordinates are
// finite adds the outer product of its unnormalised normal.  With N == 0 no key is read and every row is zero.
__global__ void __launch_bounds__(256) quadrics_kernel(int V, size_t N, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                        const uint32_t *__restrict__ ring_key, const uint32_t *__restrict__ ring_val,
                                                        double *__restrict__ out)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
    if (finite_row(vertices, v))
    {
        const uint32_t rs = lower_bound(N, ring_key, (uint32_t)v), re = lower_bound(N, ring_key, (uint32_t)v + 1u);
        const D3 pv = row(vertices, v);
        for (uint32_t j = rs; j < re; j++)
        {
            const uint32_t h = ring_val[j];
            const int32_t x = faces[next_corner(h)], y = faces[next_corner(next_corner(h))]; // in [0, V): the face takes part
            if (!finite_row(vertices, x) || !finite_row(vertices, y)) continue;
            const D3 n = cross(sub(row(vertices, x), pv), sub(row(vertices, y), pv));
            a00 = a00 + n.x * n.x; a01 = a01 + n.x * n.y; a02 = a02 + n.x * n.z;
            a11 = a11 + n.y * n.y; a12 = a12 + n.y * n.z; a22 = a22 + n.z * n.z;
        }
    }
    double *q = out + 10 * (size_t)v;
    q[0] = a00; q[1] = a01; q[2] = a02; q[3] = a11; q[4] = a12; q[5] = a22;
    q[6] = 0.0; q[7] = 0.0; q[8] = 0.0; q[9] = 0.0;
}

// ---- classification ----------------------------------------------------------------------------------------------------------------------
struct CostRule
{
    double max_cost, max2, M; // (double)max_cost, (double)max_edge squared, (double)min_cos squared
};

// One thread = one edge slot, e < N = 3 F.  Below E (*total): lo and hi from the head of the run (both in [0, V): the face took part); a run
// of two holds the half-edges sval[j] < sval[j + 1], both below N, whose faces took part: every vertex index read is in [0, V).  Past E: the
// fill values.  A candidate leaves as LOST with its cost and the inverted priority as its first sort key; every slot writes its sort record.
__global__ void __launch_bounds__(256) classify_kernel(Table t, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                        const double *__restrict__ quadrics, const uint32_t *__restrict__ sval,
                                                        const uint32_t *__restrict__ start, const uint32_t *__restrict__ end,
                                                        const uint32_t *__restrict__ total, const uint8_t *__restrict__ vclass,
                                                        const uint32_t *__restrict__ ring_start, const uint32_t *__restrict__ ring_end,
                                                        CostRule rule, uint32_t seed, int32_t *__restrict__ edge_vertices,
                                                        uint8_t *__restrict__ edge_state, int32_t *__restrict__ edge_removed,
                                                        uint8_t *__restrict__ edge_guard, double *__restrict__ edge_cost,
                                                        uint32_t *__restrict__ sort_key, uint32_t *__restrict__ sort_val, unsigned long long *totals)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t n[4] = {0, 0, 0, 0};
    uint32_t costly = 0;
    if (e < t.N)
    {
        int32_t lo = -1, hi = -1, removed = -1;
        uint8_t state = NO_EDGE, mask = 0;
        double cost = __longlong_as_double(0x7FF0000000000000ll); // +inf
        uint32_t key = 0xFFFFFFFFu;
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
                        const D3 plo = row(vertices, lo), phi = row(vertices, hi);
                        bool guards_passed = false;
                        double chosen = 0.0, found;
                        if (hi_free)
                        {
                            const uint8_t g = direction_guards(t, vertices, faces, ring_start[hi], ring_end[hi], lo, c, d, phi, plo, rule.max2, rule.M);
                            mask |= g;
                            if (g == 0)
                            {
                                guards_passed = true;
                                if (direction_cost(quadrics, hi, lo, phi, plo, found))
                                {
                                    cost = found;
                                    if (found <= rule.max_cost) { removed = hi; chosen = found; }
                                }
                            }
                        }
                        else mask |= GUARD_HELD;
                        if (lo_free)
                        {
                            const uint8_t g = direction_guards(t, vertices, faces, ring_start[lo], ring_end[lo], hi, c, d, plo, phi, rule.max2, rule.M);
                            mask |= g;
                            if (g == 0)
                            {
                                guards_passed = true;
                                if (direction_cost(quadrics, lo, hi, plo, phi, found))
                                {
                                    if (found < cost) cost = found;
                                    if (found <= rule.max_cost && (removed < 0 || found < chosen)) { removed = lo; chosen = found; } // a tie stays with hi
                                }
                            }
                        }
                        else mask |= GUARD_HELD;
                        if (removed >= 0)
                        {
                            state = LOST;
                            n[1] = 1;
                            cost = chosen;
                            key = ~priority((uint32_t)lo, (uint32_t)hi, seed);
                        }
                        else if (guards_passed)
                        {
                            state = TOO_COSTLY; // cost: the smaller finite one of the directions that passed their guards, +inf if none
                            costly = 1;
                        }
                        else
                        {
                            state = GUARDED;
                            cost = __longlong_as_double(0x7FF0000000000000ll);
                        }
                    }
                }
            }
        }
        edge_vertices[2 * e] = lo; edge_vertices[2 * e + 1] = hi;
        edge_state[e] = state;
        edge_removed[e] = removed;
        edge_guard[e] = mask;
        edge_cost[e] = cost;
        sort_key[e] = key;
        sort_val[e] = (uint32_t)e;
    }
    count4_into(totals, n);
    count_into(totals + 4, costly);
}

// ---- ranking -----------------------------------------------------------------------------------------------------------------------------
// One thread = one sorted position: the next key of the slot there, a word of its cost; all ones where the slot holds no candidate.
__global__ void __launch_bounds__(256) cost_word_kernel(size_t N, const uint32_t *__restrict__ sorted_val, const uint8_t *__restrict__ edge_state,
                                                         const double *__restrict__ edge_cost, int high, uint32_t *__restrict__ key)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const uint32_t e = sorted_val[j]; // a permutation of [0, N)
    uint32_t k = 0xFFFFFFFFu;
    if (edge_state[e] == LOST)
    {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(edge_cost[e]);
        k = high ? (uint32_t)(bits >> 32) : (uint32_t)bits;
    }
    key[j] = k;
}

// One thread = one sorted position: the slot there learns its rank; a candidate at or past the budget is DEFERRED.  Every lane reaches
// count_into.
__global__ void __launch_bounds__(256) rank_kernel(size_t N, const uint32_t *__restrict__ sorted_val, uint32_t budget, uint32_t *__restrict__ rank,
                                                    uint8_t *__restrict__ edge_state, unsigned long long *totals)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t in_budget = 0;
    if (j < N)
    {
        const uint32_t e = sorted_val[j];
        rank[e] = (uint32_t)j;
        if (edge_state[e] == LOST)
        {
            if (j < (size_t)budget) in_budget = 1;
            else edge_state[e] = DEFERRED;
        }
    }
    count_into(totals + 2, in_budget);
}

// ---- selection ---------------------------------------------------------------------------------------------------------------------------
// the unique ranks stand for (cost ascending, priority descending, edge id ascending); NONE comes last
struct RankOrder
{
    const uint32_t *rank;
    __device__ __forceinline__ bool comes_first(uint32_t a, uint32_t b) const
    {
        if (a == NONE || a == b) return false;
        if (b == NONE) return true;
        return rank[a] < rank[b];
    }
};

__global__ void __launch_bounds__(256) best_kernel(int V, Rings g, const int32_t *__restrict__ half_edge_edge, const uint8_t *__restrict__ edge_state,
                                                    RankOrder order, uint32_t *__restrict__ best)
{
    best_of_edges(V, g, half_edge_edge, edge_state, order, best);
}

__global__ void __launch_bounds__(256) best2_kernel(int V, const int32_t *__restrict__ faces, Rings g, RankOrder order,
                                                     const uint32_t *__restrict__ best, uint32_t *__restrict__ best2)
{
    best_of_ring(V, faces, g, order, best, best2);
}

__global__ void __launch_bounds__(256) winners_kernel(size_t N, const uint32_t *__restrict__ total, const int32_t *__restrict__ edge_vertices,
                                                       const int32_t *__restrict__ edge_removed, const uint32_t *__restrict__ best2,
                                                       uint8_t *__restrict__ edge_state, int32_t *__restrict__ vertex_target,
                                                       unsigned long long *totals)
{
    decide_winner(N, total, edge_vertices, edge_removed, best2, edge_state, vertex_target, totals + 3);
}

// ---- the quadrics follow the collapse ----------------------------------------------------------------------------------------------------
// One thread = one vertex, every row of out_quadrics.  v is the k of a winner e iff best2[v] == e, e collapsed, v is an end of e and not its
// r: a winner is best2 of both its ends, and at distance two no vertex is the k of two winners.  Every other row is copied word for word.
// best2 == nullptr (no faces or no vertices classified): a copy.
__global__ void __launch_bounds__(256) merge_kernel(int V, const float *__restrict__ vertices, const double *__restrict__ quadrics,
                                                     const uint32_t *__restrict__ best2, const int32_t *__restrict__ edge_vertices,
                                                     const uint8_t *__restrict__ edge_state, const int32_t *__restrict__ edge_removed,
                                                     double *__restrict__ out)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    int32_t r = -1;
    if (best2)
    {
        const uint32_t e = best2[v];
        if (e != NONE && edge_state[e] == COLLAPSED)
        {
            const int32_t lo = edge_vertices[2 * (size_t)e], hi = edge_vertices[2 * (size_t)e + 1], gone = edge_removed[e];
            if ((v == lo || v == hi) && gone != v) r = gone;
        }
    }
    double *to = out + 10 * (size_t)v;
    if (r < 0)
    {
        const unsigned long long *from = (const unsigned long long *)(quadrics + 10 * (size_t)v);
        unsigned long long *words = (unsigned long long *)to;
        const unsigned long long w0 = from[0], w1 = from[1], w2 = from[2], w3 = from[3], w4 = from[4], w5 = from[5], w6 = from[6], w7 = from[7],
                                 w8 = from[8], w9 = from[9];
        words[0] = w0; words[1] = w1; words[2] = w2; words[3] = w3; words[4] = w4; words[5] = w5; words[6] = w6; words[7] = w7; words[8] = w8;
        words[9] = w9;
        return;
    }
    const Quadric qk = load_quadric(quadrics, v), qr = load_quadric(quadrics, r);
    D3 Ad;
    const double cost_r = cost_of_removed(qr, sub(row(vertices, v), row(vertices, r)), Ad);
    to[0] = qk.a00 + qr.a00; to[1] = qk.a01 + qr.a01; to[2] = qk.a02 + qr.a02;
    to[3] = qk.a11 + qr.a11; to[4] = qk.a12 + qr.a12; to[5] = qk.a22 + qr.a22;
    to[6] = qk.b0 + (Ad.x + qr.b0); to[7] = qk.b1 + (Ad.y + qr.b1); to[8] = qk.b2 + (Ad.z + qr.b2);
    to[9] = qk.c + cost_r;
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------
struct DecimateCarve
{
    EdgeSortCarve sort;
    EdgeIdCarve ids;
    uint32_t *rk[2], *rv[2];  // the corner records, N words each
    uint32_t *ck[2], *cv[2];  // the ranking's records, N words each
    uint32_t *rank, *ring_start, *ring_end, *best, *best2;
    uint8_t *clean, *vclass;
    size_t bytes;
};
DecimateCarve decimate_carve(void *ws, size_t V, size_t F)
{
    DecimateCarve c;
    Carver w(ws);
    const size_t N = 3 * F;
    c.sort = edge_sort_carve(w, N);
    c.ids = edge_id_carve(w, N);
    c.rk[0] = w.words(N); c.rk[1] = w.words(N); c.rv[0] = w.words(N); c.rv[1] = w.words(N);
    c.ck[0] = w.words(N); c.ck[1] = w.words(N); c.cv[0] = w.words(N); c.cv[1] = w.words(N);
    c.rank = w.words(N);
    c.clean = (uint8_t *)w.bytes(N);
    c.ring_start = w.words(V); c.ring_end = w.words(V); c.best = w.words(V); c.best2 = w.words(V);
    c.vclass = (uint8_t *)w.bytes(V);
    c.bytes = w.used();
    return c;
}
} // namespace

size_t ts_decimate_workspace_bytes(int V, int F)
{
    return decimate_carve(nullptr, (size_t)(V > 0 ? V : 0), (size_t)(F > 0 ? F : 0)).bytes + 2 * TS_ALIGN;
}

hipError_t ts_decimate_quadrics(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, double *out_quadrics, void *ws,
                                hipStream_t s)
{
    if (V <= 0) return hipSuccess; // no row to write
    const size_t f = (size_t)(F > 0 ? F : 0), N = 3 * f;
    const unsigned nv = blocks256((size_t)V);
    if (F <= 0)
    {
        hipLaunchKernelGGL(quadrics_kernel, dim3(nv), dim3(256), 0, s, V, (size_t)0, vertices, faces, (const uint32_t *)nullptr,
                           (const uint32_t *)nullptr, out_quadrics);
        return hipGetLastError();
    }
    const DecimateCarve c = decimate_carve(ws, (size_t)V, f);
    hipLaunchKernelGGL(records_kernel, dim3(blocks256(f)), dim3(256), 0, s, V, F, faces, keep, c.sort.k[0], c.sort.v[0], c.rk[0], c.rv[0]);
    const int at = ts_radix_sort_pairs(c.rk, c.rv, N, bit_length((uint32_t)V), c.sort.scratch, s); // the corners by vertex, stable
    hipLaunchKernelGGL(quadrics_kernel, dim3(nv), dim3(256), 0, s, V, N, vertices, faces, (const uint32_t *)c.rk[at], (const uint32_t *)c.rv[at],
                       out_quadrics);
    return hipGetLastError();
}

hipError_t ts_decimate_round(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, const uint8_t *pinned,
                             const double *quadrics, float max_cost, int max_collapses, float max_edge, float min_cos, uint32_t seed,
                             int32_t *out_faces, uint8_t *out_keep, int32_t *vertex_target, double *out_quadrics, int32_t *edge_vertices,
                             uint8_t *edge_state, int32_t *edge_removed, uint8_t *edge_guard, double *edge_cost, unsigned long long *totals,
                             void *ws, hipStream_t s)
{
    const size_t f = (size_t)(F > 0 ? F : 0), N = 3 * f;
    const DecimateCarve c = decimate_carve(F > 0 ? ws : nullptr, (size_t)V, f);
    const unsigned nf = blocks256(f), nh = blocks256(N), nv = blocks256((size_t)V);
    hipLaunchKernelGGL(begin_kernel, dim3(1), dim3(64), 0, s, totals, F > 0 ? c.ids.total : nullptr);
    if (F <= 0)
    {
        if (V > 0 && vertex_target)
        {
            hipLaunchKernelGGL(identity_kernel, dim3(nv), dim3(256), 0, s, V, vertex_target); // no ring, no class
            hipLaunchKernelGGL(merge_kernel, dim3(nv), dim3(256), 0, s, V, vertices, quadrics, (const uint32_t *)nullptr, (const int32_t *)nullptr,
                               (const uint8_t *)nullptr, (const int32_t *)nullptr, out_quadrics);
        }
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
    const double lmax = (double)max_edge, m = (double)min_cos;
    const CostRule rule{(double)max_cost, lmax * lmax, m * m};
    // with V == 0 the edge count is the zero of begin_kernel: every slot writes its fill values and reads nothing else
    hipLaunchKernelGGL(classify_kernel, dim3(nh), dim3(256), 0, s, t, vertices, faces, quadrics, sval, (const uint32_t *)c.ids.start,
                       (const uint32_t *)c.ids.end, (const uint32_t *)c.ids.total, (const uint8_t *)c.vclass, (const uint32_t *)c.ring_start,
                       (const uint32_t *)c.ring_end, rule, seed, edge_vertices, edge_state, edge_removed, edge_guard, edge_cost, c.ck[0], c.cv[0],
                       totals);
    if (V > 0)
    {
        // by the inverted priority, then by the low and by the high word of the cost, each stable: (cost, priority descending, edge) order
        const int a0 = ts_radix_sort_pairs(c.ck, c.cv, N, 32, c.sort.scratch, s);
        hipLaunchKernelGGL(cost_word_kernel, dim3(nh), dim3(256), 0, s, N, (const uint32_t *)c.cv[a0], (const uint8_t *)edge_state,
                           (const double *)edge_cost, 0, c.ck[a0 ^ 1]);
        uint32_t *const k1[2] = {c.ck[a0 ^ 1], c.ck[a0]}, *const v1[2] = {c.cv[a0], c.cv[a0 ^ 1]};
        const int a1 = ts_radix_sort_pairs(k1, v1, N, 32, c.sort.scratch, s);
        hipLaunchKernelGGL(cost_word_kernel, dim3(nh), dim3(256), 0, s, N, (const uint32_t *)v1[a1], (const uint8_t *)edge_state,
                           (const double *)edge_cost, 1, k1[a1 ^ 1]);
        uint32_t *const k2[2] = {k1[a1 ^ 1], k1[a1]}, *const v2[2] = {v1[a1], v1[a1 ^ 1]};
        const int a2 = ts_radix_sort_pairs(k2, v2, N, 32, c.sort.scratch, s);
        hipLaunchKernelGGL(rank_kernel, dim3(nh), dim3(256), 0, s, N, (const uint32_t *)v2[a2], (uint32_t)max_collapses, c.rank, edge_state, totals);
        const Rings g{t.ring_val, c.ring_start, c.ring_end};
        const RankOrder order{c.rank};
        hipLaunchKernelGGL(best_kernel, dim3(nv), dim3(256), 0, s, V, g, (const int32_t *)c.ids.half_edge_edge, (const uint8_t *)edge_state, order,
                           c.best);
        hipLaunchKernelGGL(best2_kernel, dim3(nv), dim3(256), 0, s, V, faces, g, order, (const uint32_t *)c.best, c.best2);
        hipLaunchKernelGGL(winners_kernel, dim3(nh), dim3(256), 0, s, N, (const uint32_t *)c.ids.total, (const int32_t *)edge_vertices,
                           (const int32_t *)edge_removed, (const uint32_t *)c.best2, edge_state, vertex_target, totals);
    }
    if (out_faces)
    {
        hipLaunchKernelGGL(apply_kernel, dim3(nf), dim3(256), 0, s, V, F, faces, keep, (const int32_t *)vertex_target, out_faces, out_keep);
        if (V > 0)
            hipLaunchKernelGGL(merge_kernel, dim3(nv), dim3(256), 0, s, V, vertices, quadrics, (const uint32_t *)c.best2,
                               (const int32_t *)edge_vertices, (const uint8_t *)edge_state, (const int32_t *)edge_removed, out_quadrics);
    }
    return hipGetLastError();
}
