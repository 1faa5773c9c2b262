// mesh_contract.hip -- one round of edge contractions ordered by quadric error, with a budget: the survivor of an edge between two FREE
// vertices moves to the regularised minimum of the edge's quadric, rounded to fp32 first and judged there (include/ts_contract.h).
//
// The arithmetic is float64 on the fp32 inputs widened, every operation rounded: the unit is built with -ffp-contract=off.  The only atomics
// are the integer adds of the counters.  The unit clears and copies nothing with a fill or a copy: every output element is written by the
// kernel that owns its index, and the five counters are cleared by the first kernel of the round (begin_kernel), in stream order.
//
// The front -- half-edge and corner records, the sort by edge, the edge ids, the sort of the corners by vertex, the clean-edge flags, the
// vertex classes -- the guards of an edge with a held end, the priority, the selection and the face map are csrc/ts_collapse_round.h's, as
// mesh_decimate.hip launches them.  This unit's own: the edge quadric, the solve and the clamp, the guards of a placed edge over the rings of
// both ends at p*, the ranking, and the kernel that follows the winners (quadrics in the survivor's new frame, the moved vertex, the blend).
//
// classify_kernel is the hot one: every edge with two FREE ends loads twenty float64 words, solves a 3 x 3 system and walks two rings, each
// corner a 12-byte row gather or two and a binary search.  The eligibility tests (the run of two, the classes, c != d, the twelve finite
// coordinates) come before the first quadric word is loaded; an edge that is not eligible costs what it costs in mesh_decimate.hip.
//
// A quadric is held in ten named scalars (Quadric), never in a per-thread array indexed at run time: that would go to scratch.
#include "ts_contract_launch.h"
#include "ts_collapse_round.h"

namespace
{
constexpr uint8_t TOO_COSTLY = 2, DEFERRED = 6; // TSU_*; the other states, the guard bits and the ring bound: csrc/ts_collapse_round.h
constexpr uint32_t NAN32 = 0x7FC00000u;         // edge_position where there is no candidate

// ---- the first kernel of the round -------------------------------------------------------------------------------------------------------
// One workgroup: the five counters and the workspace's edge count (read as E = 0 where the front does not run) start at zero.
__global__ void __launch_bounds__(64) begin_kernel(unsigned long long *totals, uint32_t *total)
{
    if (threadIdx.x < 5) totals[threadIdx.x] = 0ull;
    if (total && threadIdx.x < 4) total[threadIdx.x] = 0u;
}

// ---- quadrics ----------------------------------------------------------------------------------------------------------------------------
struct Quadric // a00 a01 a02 a11 a12 a22 b0 b1 b2 c, in a vertex's own frame
{
    double a00, a01, a02, a11, a12, a22, b0, b1, b2, c;
};
__device__ __forceinline__ Quadric load_quadric(const double *__restrict__ q, int32_t v)
{
    const double *p = q + 10 * (size_t)v;
    return {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]};
}

// A y per row, and (dot(y, A y) + (dot(b, y) + dot(b, y))) + c, unclamped: cost_r of a removed vertex at y = d, the cost of an edge at y'
__device__ __forceinline__ double quadric_at(const Quadric &q, const D3 &y, D3 &Ay)
{
    Ay.x = (q.a00 * y.x + q.a01 * y.y) + q.a02 * y.z;
    Ay.y = (q.a01 * y.x + q.a11 * y.y) + q.a12 * y.z;
    Ay.z = (q.a02 * y.x + q.a12 * y.y) + q.a22 * y.z;
    const D3 b{q.b0, q.b1, q.b2};
    const double by = dot(b, y);
    return (dot(y, Ay) + (by + by)) + q.c;
}

// The quadric of the edge in the frame of k: A = A_k + A_r, b = b_k + (A_r d + b_r), c = c_k + cost_r, with d = p_k - p_r.
__device__ __forceinline__ Quadric edge_quadric(const double *__restrict__ quadrics, int32_t r, int32_t k, const D3 &d)
{
    const Quadric qr = load_quadric(quadrics, r);
    D3 Ad;
    const double cost_r = quadric_at(qr, d, Ad);
    const Quadric qk = load_quadric(quadrics, k);
    return {qk.a00 + qr.a00, qk.a01 + qr.a01, qk.a02 + qr.a02, qk.a11 + qr.a11, qk.a12 + qr.a12, qk.a22 + qr.a22,
            qk.b0 + (Ad.x + qr.b0), qk.b1 + (Ad.y + qr.b1), qk.b2 + (Ad.z + qr.b2), qk.c + cost_r};
}

// The cost of the half-edge collapse r -> k onto a held k: false if it is not finite; a negative cost and -0 become +0.
__device__ __forceinline__ bool direction_cost(const double *__restrict__ quadrics, int32_t r, int32_t k, const D3 &d, double &cost)
{
    const Quadric q = load_quadric(quadrics, r);
    D3 Ad;
    const double c = quadric_at(q, d, Ad) + quadrics[10 * (size_t)k + 9];
    if (!finite64(c)) return false;
    cost = c > 0.0 ? c : 0.0;
    return true;
}

__device__ __forceinline__ double reach_axis(double y, double m, double h) { return y - m > h ? m + h : (y - m < -h ? m - h : y); }

// y of the placement: the regularised minimum of q around the midpoint m = -0.5 d, within h = reach max|d_i| of it per axis; m where a test fails
__device__ __forceinline__ D3 place(const Quadric &q, const D3 &d, double lambda, double reach)
{
    const D3 m{-0.5 * d.x, -0.5 * d.y, -0.5 * d.z};
    D3 y = m;
    const double tr = (q.a00 + q.a11) + q.a22;
    if (finite64(tr) && tr > 0.0)
    {
        const double mu = lambda * tr;
        const double a00 = q.a00 + mu, a11 = q.a11 + mu, a22 = q.a22 + mu, a01 = q.a01, a02 = q.a02, a12 = q.a12;
        const double r0 = mu * m.x - q.b0, r1 = mu * m.y - q.b1, r2 = mu * m.z - q.b2;
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double det = (a00 * c00 + a01 * c01) + a02 * c02;
        if (finite64(det) && det > 0.0)
        {
            const double y0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
            const double y1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
            const double y2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
            if (finite64(y0) && finite64(y1) && finite64(y2)) y = D3{y0, y1, y2};
        }
    }
    const double h = reach * fmax(fmax(fabs(d.x), fabs(d.y)), fabs(d.z));
    if (!(h > 0.0)) return m;
    return {reach_axis(y.x, m.x, h), reach_axis(y.y, m.y, h), reach_axis(y.z, m.z, h)};
}

// ---- classification ----------------------------------------------------------------------------------------------------------------------
struct PlaceRule
{
    double max_cost, max2, M, lambda, reach; // (double)max_cost, (double)max_edge squared, (double)min_cos squared, (double)lambda, (double)reach
};

// The guards of a placed edge over the whole rings of r (side 0) and of k (side 1), without early exit: the mask of those that fail.  Both
// ends are FREE, so each ring has at most MAX_RING corners, and every corner belongs to a face that takes part: x and y are in [0, V).
__device__ __forceinline__ uint8_t placed_guards(const Table &t, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                 const uint32_t *__restrict__ ring_start, const uint32_t *__restrict__ ring_end, int32_t r,
                                                 int32_t k, int32_t c, int32_t d, const D3 &pr, const D3 &pk, const D3 &ps, double max2, double M)
{
    uint8_t mask = 0;
#pragma unroll 1
    for (int side = 0; side < 2; side++)
    {
        const int32_t v = side ? k : r, other = side ? r : k;
        const D3 pv = side ? pk : pr;
        for (uint32_t j = ring_start[v], re = ring_end[v]; j < re; j++)
        {
            const uint32_t h = t.ring_val[j];
            const int32_t x = faces[next_corner(h)], y = faces[next_corner(next_corner(h))];
            if (x == other) continue; // a face on the edge; the other one has y == other
            const D3 px = row(vertices, x);
            if (side == 0 && x != c && x != d && table_has(t.N, t.smin, t.smax, (uint32_t)min(x, k), (uint32_t)max(x, k))) mask |= GUARD_LINK;
            const D3 l = sub(px, ps);
            if (!(dot(l, l) <= max2)) mask |= GUARD_LONG;
            if (y == other) continue;
            if (side == 0 && ((x == c && y == d) || (x == d && y == c))) mask |= GUARD_LINK;
            const D3 py = row(vertices, y);
            const D3 n0 = cross(sub(px, pv), sub(py, pv)), n1 = cross(sub(px, ps), sub(py, ps));
            const double Q0 = dot(n0, n0), Q1 = dot(n1, n1), D = dot(n0, n1);
            if (!(Q1 > 0.0 && (Q0 == 0.0 || (D > 0.0 && D * D >= (M * Q0) * Q1)))) mask |= GUARD_NORMAL;
        }
    }
    return mask;
}

// One thread = one edge slot, e < N = 3 F.  Below E (*total): lo and hi from the head of the run (both in [0, V): the face took part); a run
// of two holds the half-edges sval[j] < sval[j + 1], both below N, whose faces took part: every vertex index read is in [0, V).  Past E: the
// fill values.  A candidate leaves as LOST with its cost, its p* and the inverted priority as its first sort key; every slot writes its
// sort record and its three words of edge_position.
__global__ void __launch_bounds__(256) classify_kernel(Table t, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                        const double *__restrict__ quadrics, const uint32_t *__restrict__ sval,
                                                        const uint32_t *__restrict__ start, const uint32_t *__restrict__ end,
                                                        const uint32_t *__restrict__ total, const uint8_t *__restrict__ vclass,
                                                        const uint32_t *__restrict__ ring_start, const uint32_t *__restrict__ ring_end,
                                                        PlaceRule rule, uint32_t seed, int32_t *__restrict__ edge_vertices,
                                                        uint8_t *__restrict__ edge_state, int32_t *__restrict__ edge_removed,
                                                        uint8_t *__restrict__ edge_guard, double *__restrict__ edge_cost,
                                                        uint32_t *__restrict__ edge_position, uint32_t *__restrict__ sort_key,
                                                        uint32_t *__restrict__ sort_val, unsigned long long *totals)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t n[4] = {0, 0, 0, 0};
    uint32_t costly = 0;
    if (e < t.N)
    {
        int32_t lo = -1, hi = -1, removed = -1;
        uint8_t state = NO_EDGE, mask = 0;
        double cost = __longlong_as_double(0x7FF0000000000000ll); // +inf
        uint32_t key = 0xFFFFFFFFu, s0 = NAN32, s1 = NAN32, s2 = NAN32;
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
                        const int32_t r = hi_free ? hi : lo, k = hi_free ? lo : hi; // both FREE: k = lo
                        const D3 pr = row(vertices, r), pk = row(vertices, k);
                        const D3 dk = sub(pk, pr);
                        const float *fk = vertices + 3 * (size_t)k;
                        float f0 = fk[0], f1 = fk[1], f2 = fk[2]; // p*: p_k where the survivor stays
                        uint8_t g;
                        bool has_cost = false;
                        double found = 0.0;
                        if (lo_free && hi_free)
                        {
                            const Quadric q = edge_quadric(quadrics, r, k, dk);
                            const D3 y = place(q, dk, rule.lambda, rule.reach);
                            f0 = (float)(pk.x + y.x); f1 = (float)(pk.y + y.y); f2 = (float)(pk.z + y.z);
                            const D3 ps{(double)f0, (double)f1, (double)f2};
                            D3 Ay; // the cost comes before the walks, so that the ten scalars of the quadric are not live across them
                            const double at = quadric_at(q, sub(ps, pk), Ay);
                            has_cost = finite64(at);
                            found = at > 0.0 ? at : 0.0;
                            g = placed_guards(t, vertices, faces, ring_start, ring_end, r, k, c, d, pr, pk, ps, rule.max2, rule.M);
                        }
                        else
                        {
                            mask = GUARD_HELD; // the direction that would remove the held end is not walked
                            g = direction_guards(t, vertices, faces, ring_start[r], ring_end[r], k, c, d, pr, pk, rule.max2, rule.M);
                            if (g == 0) has_cost = direction_cost(quadrics, r, k, dk, found);
                        }
                        mask |= g;
                        if (g != 0) state = GUARDED;
                        else if (has_cost && found <= rule.max_cost)
                        {
                            state = LOST;
                            n[1] = 1;
                            removed = r;
                            cost = found;
                            key = ~priority((uint32_t)lo, (uint32_t)hi, seed);
                            s0 = __float_as_uint(f0); s1 = __float_as_uint(f1); s2 = __float_as_uint(f2);
                        }
                        else
                        {
                            state = TOO_COSTLY; // its cost, +inf if it has none
                            costly = 1;
                            if (has_cost) cost = found;
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
        edge_position[3 * e] = s0; edge_position[3 * e + 1] = s1; edge_position[3 * e + 2] = s2;
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

// ---- what follows a winner ---------------------------------------------------------------------------------------------------------------
// One thread = one vertex: its row of out_quadrics and of out_vertices and its word of vertex_blend.  v is the k of a winner e iff
// best2[v] == e, e collapsed, v is an end of e and not its r: a winner is best2 of both its ends, and at distance two no vertex is the k of
// two winners.  The survivor was placed iff both ends are FREE; its p* is read back from edge_position, so y' here is y' there bit for bit.
// Every other row is copied word for word.  best2 == nullptr (no faces or no vertices classified): copies and zeros.
__global__ void __launch_bounds__(256) follow_kernel(int V, const float *__restrict__ vertices, const double *__restrict__ quadrics,
                                                      const uint32_t *__restrict__ best2, const uint8_t *__restrict__ vclass,
                                                      const int32_t *__restrict__ edge_vertices, const uint8_t *__restrict__ edge_state,
                                                      const int32_t *__restrict__ edge_removed, const uint32_t *__restrict__ edge_position,
                                                      uint32_t *__restrict__ out_vertices, double *__restrict__ out, double *__restrict__ blend)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    int32_t r = -1;
    uint32_t won = NONE;
    bool placed = false;
    if (best2)
    {
        const uint32_t e = best2[v];
        if (e != NONE && edge_state[e] == COLLAPSED)
        {
            const int32_t lo = edge_vertices[2 * (size_t)e], hi = edge_vertices[2 * (size_t)e + 1], gone = edge_removed[e];
            if ((v == lo || v == hi) && gone != v)
            {
                r = gone;
                won = e;
                placed = vclass[lo] == FREE && vclass[hi] == FREE;
            }
        }
    }
    const uint32_t *own = (const uint32_t *)(vertices + 3 * (size_t)v);
    uint32_t *moved = out_vertices + 3 * (size_t)v;
    double *to = out + 10 * (size_t)v;
    if (r < 0)
    {
        const unsigned long long *from = (const unsigned long long *)(quadrics + 10 * (size_t)v);
        unsigned long long *words = (unsigned long long *)to;
        const unsigned long long w0 = from[0], w1 = from[1], w2 = from[2], w3 = from[3], w4 = from[4], w5 = from[5], w6 = from[6], w7 = from[7],
                                 w8 = from[8], w9 = from[9];
        const uint32_t x0 = own[0], x1 = own[1], x2 = own[2];
        words[0] = w0; words[1] = w1; words[2] = w2; words[3] = w3; words[4] = w4; words[5] = w5; words[6] = w6; words[7] = w7; words[8] = w8;
        words[9] = w9;
        moved[0] = x0; moved[1] = x1; moved[2] = x2;
        blend[v] = 0.0;
        return;
    }
    const D3 pk = row(vertices, v);
    const D3 d = sub(pk, row(vertices, r));
    const Quadric q = edge_quadric(quadrics, r, v, d);
    to[0] = q.a00; to[1] = q.a01; to[2] = q.a02; to[3] = q.a11; to[4] = q.a12; to[5] = q.a22;
    if (!placed)
    {
        const uint32_t x0 = own[0], x1 = own[1], x2 = own[2];
        to[6] = q.b0; to[7] = q.b1; to[8] = q.b2; to[9] = q.c;
        moved[0] = x0; moved[1] = x1; moved[2] = x2;
        blend[v] = 0.0;
        return;
    }
    const uint32_t s0 = edge_position[3 * (size_t)won], s1 = edge_position[3 * (size_t)won + 1], s2 = edge_position[3 * (size_t)won + 2];
    const D3 y{(double)__uint_as_float(s0) - pk.x, (double)__uint_as_float(s1) - pk.y, (double)__uint_as_float(s2) - pk.z};
    D3 Ay;
    const double cost = quadric_at(q, y, Ay);
    to[6] = q.b0 + Ay.x; to[7] = q.b1 + Ay.y; to[8] = q.b2 + Ay.z; to[9] = cost;
    moved[0] = s0; moved[1] = s1; moved[2] = s2;
    const D3 back{-d.x, -d.y, -d.z};
    const double den = dot(d, d);
    double share = 0.0;
    if (den != 0.0)
    {
        share = dot(y, back) / den;
        if (!(share > 0.0)) share = 0.0;
        if (share > 1.0) share = 1.0;
    }
    blend[v] = share;
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------
struct ContractCarve
{
    EdgeSortCarve sort;
    EdgeIdCarve ids;
    uint32_t *rk[2], *rv[2];  // the corner records, N words each
    uint32_t *ck[2], *cv[2];  // the ranking's records, N words each
    uint32_t *rank, *ring_start, *ring_end, *best, *best2;
    uint8_t *clean, *vclass;
    size_t bytes;
};
ContractCarve contract_carve(void *ws, size_t V, size_t F)
{
    ContractCarve c;
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

size_t ts_contract_workspace_bytes(int V, int F)
{
    return contract_carve(nullptr, (size_t)(V > 0 ? V : 0), (size_t)(F > 0 ? F : 0)).bytes + 2 * TS_ALIGN;
}

hipError_t ts_contract_round(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, const uint8_t *pinned,
                             const double *quadrics, float max_cost, int max_collapses, float max_edge, float min_cos, float lambda, float reach,
                             uint32_t seed, int32_t *out_faces, uint8_t *out_keep, int32_t *vertex_target, float *out_vertices,
                             double *out_quadrics, double *vertex_blend, int32_t *edge_vertices, uint8_t *edge_state, int32_t *edge_removed,
                             uint8_t *edge_guard, double *edge_cost, float *edge_position, unsigned long long *totals, void *ws, hipStream_t s)
{
    const size_t f = (size_t)(F > 0 ? F : 0), N = 3 * f;
    const ContractCarve c = contract_carve(F > 0 ? ws : nullptr, (size_t)V, f);
    const unsigned nf = blocks256(f), nh = blocks256(N), nv = blocks256((size_t)V);
    hipLaunchKernelGGL(begin_kernel, dim3(1), dim3(64), 0, s, totals, F > 0 ? c.ids.total : nullptr);
    if (F <= 0)
    {
        if (V > 0 && vertex_target)
        {
            hipLaunchKernelGGL(identity_kernel, dim3(nv), dim3(256), 0, s, V, vertex_target); // no ring, no class
            hipLaunchKernelGGL(follow_kernel, dim3(nv), dim3(256), 0, s, V, vertices, quadrics, (const uint32_t *)nullptr, (const uint8_t *)nullptr,
                               (const int32_t *)nullptr, (const uint8_t *)nullptr, (const int32_t *)nullptr, (const uint32_t *)nullptr,
                               (uint32_t *)out_vertices, out_quadrics, vertex_blend);
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
    const PlaceRule rule{(double)max_cost, lmax * lmax, m * m, (double)lambda, (double)reach};
    // with V == 0 the edge count is the zero of begin_kernel: every slot writes its fill values and reads nothing else
    hipLaunchKernelGGL(classify_kernel, dim3(nh), dim3(256), 0, s, t, vertices, faces, quadrics, sval, (const uint32_t *)c.ids.start,
                       (const uint32_t *)c.ids.end, (const uint32_t *)c.ids.total, (const uint8_t *)c.vclass, (const uint32_t *)c.ring_start,
                       (const uint32_t *)c.ring_end, rule, seed, edge_vertices, edge_state, edge_removed, edge_guard, edge_cost,
                       (uint32_t *)edge_position, c.ck[0], c.cv[0], totals);
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
            hipLaunchKernelGGL(follow_kernel, dim3(nv), dim3(256), 0, s, V, vertices, quadrics, (const uint32_t *)c.best2, (const uint8_t *)c.vclass,
                               (const int32_t *)edge_vertices, (const uint8_t *)edge_state, (const int32_t *)edge_removed,
                               (const uint32_t *)edge_position, (uint32_t *)out_vertices, out_quadrics, vertex_blend);
    }
    return hipGetLastError();
}
