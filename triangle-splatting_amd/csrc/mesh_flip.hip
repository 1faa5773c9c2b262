// mesh_flip.hip -- one round of edge flips toward the Delaunay condition on an indexed mesh (include/ts_flip.h).
//
// The arithmetic is float64 on the fp32 inputs widened, every operation rounded: the unit is built with -ffp-contract=off.  The only atomics
// are the integer adds of the counters.
//
// Edges.  The front is mesh_subdivide.hip's: the sort-by-edge front (csrc/ts_mesh_edges.h) leaves the half-edges of the faces that take part
// in (lo, hi) order, run heads (edge_run_head) become edge ids by one exclusive prefix sum (scan_columns), and the head and the tail of every
// run write its bounds.  The three small kernels of that front are this unit's own copies: the units live in different libraries.
//
// Round.  One thread per edge slot reads (lo, hi) at the head of its run, finds the two faces and their opposite vertices behind the two
// half-edges of the run, gathers the four 12-byte vertex rows and decides the state: the criterion, the binary search for the new edge over
// the sorted columns, the criterion of the new edge, flatness and fold.  A candidate writes its priority.  One scatter hands the edge ids to
// the half-edges, and one thread per edge compares a candidate with the candidates among the four other edges of its two faces.  The winners
// share no face, so there are at most F / 2: a prefix sum compacts them in ascending edge id, two stable radix sorts order their new edges
// (larger end, then smaller end), and the head of every run of equal new edges flips -- the smallest edge id, since the sorts are stable.
// One thread per face gathers its new indices: at most one of its three edges flipped.
#include "ts_flip_launch.h"
#include "ts_mesh_edges.h"
#include "ts_mesh_scan.h"

namespace
{
constexpr uint8_t NO_EDGE = 0, NOT_ELIGIBLE = 1, DELAUNAY = 2, GUARDED = 3, LOST = 4, DUPLICATE = 5, FLIPPED = 6; // TSE_*
constexpr uint32_t NONE = 0xFFFFFFFFu;                                                                           // no winner in this slot

// ---- edges -------------------------------------------------------------------------------------------------------------------------------
// One thread = one face: its three records.
__global__ void __launch_bounds__(256) records_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep,
                                                       uint32_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int32_t v[3];
    const bool ok = face_takes_part(V, (size_t)f, faces, keep, v);
    half_edge_records(V, (size_t)f, ok, v, key, val);
}

// One thread = one sorted position: 1 at the head of a run of a real edge.
__global__ void __launch_bounds__(256) heads_kernel(int V, size_t N, const uint32_t *__restrict__ smin, const uint32_t *__restrict__ smax,
                                                     uint32_t *__restrict__ head)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    head[j] = edge_run_head(V, N, j, smin, smax) != 0;
}

// One thread = one sorted position.  eid[j] holds the number of heads in front of j and becomes the edge id of the position, -1 (all bits)
// on a sentinel.  A real position lies in a run whose head was counted, so its id is below E <= N: start and end hold N words.
__global__ void __launch_bounds__(256) runs_kernel(int V, size_t N, const uint32_t *__restrict__ smin, const uint32_t *__restrict__ smax,
                                                    uint32_t *__restrict__ eid, uint32_t *__restrict__ start, uint32_t *__restrict__ end)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const uint32_t a = smin[j], b = smax[j];
    if (a >= (uint32_t)V)
    {
        eid[j] = NONE;
        return;
    }
    const bool head = j == 0 || smin[j - 1] != a || smax[j - 1] != b;
    const bool tail = j + 1 == N || smin[j + 1] != a || smax[j + 1] != b;
    const uint32_t e = eid[j] - (head ? 0u : 1u);
    eid[j] = e;
    if (head) start[e] = (uint32_t)j;
    if (tail) end[e] = (uint32_t)(j + 1);
}

// One thread = one sorted position: the half-edge there learns its edge.  sval is a permutation of [0, N), so every half-edge is written.
__global__ void __launch_bounds__(256) scatter_kernel(size_t N, const uint32_t *__restrict__ sval, const uint32_t *__restrict__ eid,
                                                       int32_t *__restrict__ half_edge_edge)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    half_edge_edge[sval[j]] = (int32_t)eid[j];
}

// ---- the criterion and the guards --------------------------------------------------------------------------------------------------------
struct D3
{
    double x, y, z;
};
__device__ __forceinline__ D3 sub(const D3 &p, const D3 &q) { return {p.x - q.x, p.y - q.y, p.z - q.z}; }
__device__ __forceinline__ double dot(const D3 &s, const D3 &t) { return (s.x * t.x + s.y * t.y) + s.z * t.z; }
__device__ __forceinline__ D3 cross(const D3 &s, const D3 &t) { return {s.y * t.z - s.z * t.y, s.z * t.x - s.x * t.z, s.x * t.y - s.y * t.x}; }

// the widened row of vertex i < V; *finite is cleared where a coordinate is not
__device__ __forceinline__ D3 row(const float *__restrict__ vertices, int32_t i, bool *finite)
{
    const float *p = vertices + 3 * (size_t)i;
    const float x = p[0], y = p[1], z = p[2];
    *finite = *finite && finite32(x) && finite32(y) && finite32(z);
    return {(double)x, (double)y, (double)z};
}

// W(p, q; r, s) of include/ts_flip.h: the angles at r and s opposite to the edge p-q sum to more than pi
__device__ __forceinline__ bool wants_flip(const D3 &p, const D3 &q, const D3 &r, const D3 &s)
{
    const D3 u = sub(p, r), v = sub(q, r), w = cross(u, v);
    const double A = dot(u, v), P = dot(w, w);
    const D3 u2 = sub(p, s), v2 = sub(q, s), w2 = cross(u2, v2);
    const double B = dot(u2, v2), Q = dot(w2, w2);
    if (A < 0.0 && B < 0.0) return P > 0.0 || Q > 0.0;
    if (A < 0.0 && B >= 0.0) return (A * A) * Q > (B * B) * P;
    if (B < 0.0 && A >= 0.0) return (B * B) * P > (A * A) * Q;
    return false;
}

// guards (iii) and (iv): the two faces are flat enough across a-b, and neither new face folds over
__device__ __forceinline__ bool flat_and_unfolded(const D3 &a, const D3 &b, const D3 &c, const D3 &d, double min_cos)
{
    const D3 n0 = cross(sub(b, a), sub(c, a)), n1 = cross(sub(a, b), sub(d, b));
    const double D = dot(n0, n1), L = dot(n0, n0) * dot(n1, n1), M = min_cos * min_cos;
    const bool flat = min_cos >= 0.0 ? (D >= 0.0 && D * D >= M * L) : (D >= 0.0 || D * D <= M * L);
    if (!flat) return false;
    const D3 S = {n0.x + n1.x, n0.y + n1.y, n0.z + n1.z};
    const D3 m0 = cross(sub(d, a), sub(c, a)), m1 = cross(sub(b, d), sub(c, d));
    return dot(m0, S) > 0.0 && dot(m1, S) > 0.0;
}

// guard (i): is (m, M) among the N sorted positions?  The sentinels (V, V) sort last and equal no pair of vertices.
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

// One thread = one edge slot, e < N = 3 F.  Below E (*total): lo and hi from the head of the run (both in [0, V): the face took part); a run
// of two holds the half-edges sval[j] < sval[j + 1], both below N, whose faces took part: every vertex index read is in [0, V).  Past E: the
// fill values.  A candidate leaves as LOST; winner_kernel and flip_kernel promote it.
__global__ void __launch_bounds__(256) classify_kernel(size_t N, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                        const uint32_t *__restrict__ smin, const uint32_t *__restrict__ smax,
                                                        const uint32_t *__restrict__ sval, const uint32_t *__restrict__ start,
                                                        const uint32_t *__restrict__ end, const uint32_t *__restrict__ total, double min_cos,
                                                        uint32_t seed, int32_t *__restrict__ edge_vertices, uint8_t *__restrict__ edge_state,
                                                        int32_t *__restrict__ edge_opposite, uint32_t *__restrict__ prio, unsigned long long *totals)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t n[4] = {0, 0, 0, 0};
    if (e < N)
    {
        int32_t lo = -1, hi = -1, oc = -1, od = -1;
        uint8_t state = NO_EDGE;
        if (e < (size_t)*total)
        {
            const uint32_t j = start[e];
            lo = (int32_t)smin[j]; hi = (int32_t)smax[j];
            state = NOT_ELIGIBLE;
            n[0] = 1;
            if (end[e] - j == 2)
            {
                uint32_t h0 = sval[j], h1 = sval[j + 1];
                const int32_t from0 = faces[h0], from1 = faces[h1];
                if (from0 != from1) // opposite directions
                {
                    if (from0 != lo) { const uint32_t t = h0; h0 = h1; h1 = t; } // h0 runs lo -> hi
                    const int32_t c = faces[next_corner(next_corner(h0))], d = faces[next_corner(next_corner(h1))];
                    if (c != d)
                    {
                        bool finite = true;
                        const D3 pa = row(vertices, lo, &finite), pb = row(vertices, hi, &finite), pc = row(vertices, c, &finite),
                                 pd = row(vertices, d, &finite);
                        if (finite)
                        {
                            oc = c; od = d;
                            state = DELAUNAY;
                            if (wants_flip(pa, pb, pc, pd))
                            {
                                state = GUARDED;
                                n[1] = 1;
                                if (!table_has(N, smin, smax, (uint32_t)min(c, d), (uint32_t)max(c, d)) && !wants_flip(pc, pd, pa, pb) &&
                                    flat_and_unfolded(pa, pb, pc, pd, min_cos))
                                {
                                    state = LOST;
                                    n[2] = 1;
                                    prio[e] = priority((uint32_t)lo, (uint32_t)hi, seed);
                                }
                            }
                        }
                    }
                }
            }
        }
        edge_vertices[2 * e] = lo; edge_vertices[2 * e + 1] = hi;
        edge_opposite[2 * e] = oc; edge_opposite[2 * e + 1] = od;
        edge_state[e] = state;
    }
    count4_into(totals, n);
}

// ---- selection ---------------------------------------------------------------------------------------------------------------------------
// One thread = one edge slot.  A candidate (LOST so far) has a run of two half-edges whose faces took part, so the four other half-edges of
// the two faces carry edge ids in [0, E).  win and rank receive the same flag: rank becomes its prefix sum.
__global__ void __launch_bounds__(256) winner_kernel(size_t N, const uint32_t *__restrict__ total, const uint32_t *__restrict__ start,
                                                      const uint32_t *__restrict__ sval, const int32_t *__restrict__ half_edge_edge,
                                                      const uint8_t *__restrict__ edge_state, const uint32_t *__restrict__ prio,
                                                      uint32_t *__restrict__ win, uint32_t *__restrict__ rank)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    uint32_t w = 0;
    if (e < (size_t)*total && edge_state[e] == LOST)
    {
        w = 1;
        const uint32_t j = start[e], mine = prio[e];
#pragma unroll
        for (int side = 0; side < 2; side++)
        {
            uint32_t h = sval[j + side];
#pragma unroll
            for (int k = 0; k < 2; k++)
            {
                h = next_corner(h);
                const int32_t o = half_edge_edge[h];
                if (o < 0 || edge_state[o] != LOST) continue;
                const uint32_t theirs = prio[o];
                if (theirs > mine || (theirs == mine && (size_t)o < e)) w = 0;
            }
        }
    }
    win[e] = w;
    rank[e] = w;
}

// One thread = one edge slot and one slot of the winners' list (cap of them).  Winners share no face, so there are at most F / 2 <= cap and a
// rank is below that; the slots from the number of winners (*winners) on take the sentinel key V, which sorts last.
__global__ void __launch_bounds__(256) compact_kernel(int V, size_t N, size_t cap, const uint32_t *__restrict__ winners,
                                                       const uint32_t *__restrict__ win, const uint32_t *__restrict__ rank,
                                                       const int32_t *__restrict__ edge_opposite, uint32_t *__restrict__ key,
                                                       uint32_t *__restrict__ val)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N && win[i])
    {
        const size_t r = rank[i];
        if (r < cap)
        {
            key[r] = (uint32_t)max(edge_opposite[2 * i], edge_opposite[2 * i + 1]);
            val[r] = (uint32_t)i;
        }
    }
    if (i < cap && i >= (size_t)*winners)
    {
        key[i] = (uint32_t)V;
        val[i] = NONE;
    }
}

// One thread = one slot of the winners' list in the order of the larger new end: the smaller new end, the next key.
__global__ void __launch_bounds__(256) smaller_end_kernel(int V, size_t cap, const uint32_t *__restrict__ val, const int32_t *__restrict__ edge_opposite,
                                                           uint32_t *__restrict__ key)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= cap) return;
    const uint32_t e = val[j];
    key[j] = e == NONE ? (uint32_t)V : (uint32_t)min(edge_opposite[2 * (size_t)e], edge_opposite[2 * (size_t)e + 1]);
}

// One thread = one slot of the winners' list in (smaller, larger, edge id) order of the new edges: the head of a run flips, the rest are
// duplicates.  Every lane reaches count_into.
__global__ void __launch_bounds__(256) flip_kernel(size_t cap, const uint32_t *__restrict__ val, const int32_t *__restrict__ edge_opposite,
                                                    uint8_t *__restrict__ edge_state, unsigned long long *totals)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t head = 0;
    const uint32_t e = j < cap ? val[j] : NONE;
    if (e != NONE)
    {
        const int32_t c = edge_opposite[2 * (size_t)e], d = edge_opposite[2 * (size_t)e + 1];
        head = 1;
        if (j > 0)
        {
            const uint32_t p = val[j - 1]; // a winner too: the sentinels sort last
            const int32_t pc = edge_opposite[2 * (size_t)p], pd = edge_opposite[2 * (size_t)p + 1];
            head = min(pc, pd) != min(c, d) || max(pc, pd) != max(c, d);
        }
        edge_state[e] = head ? FLIPPED : DUPLICATE;
    }
    count_into(totals + 3, head);
}

// ---- the flip ----------------------------------------------------------------------------------------------------------------------------
// One thread = one face, in gather form.  A face whose half-edge k lies on a flipped edge is f0 where the half-edge runs lo -> hi -- it
// becomes (a, d, c) -- and f1 otherwise -- it becomes (d, b, c).  Winners share no face: at most one k applies.
__global__ void __launch_bounds__(256) apply_kernel(int F, const int32_t *__restrict__ faces, const int32_t *__restrict__ half_edge_edge,
                                                     const uint8_t *__restrict__ edge_state, const int32_t *__restrict__ edge_vertices,
                                                     const int32_t *__restrict__ edge_opposite, int32_t *__restrict__ out_faces,
                                                     uint8_t *__restrict__ face_flipped)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const size_t at = 3 * (size_t)f;
    const int32_t v[3] = {faces[at], faces[at + 1], faces[at + 2]};
    int32_t o[3] = {v[0], v[1], v[2]};
    uint8_t flipped = 0;
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const int32_t e = half_edge_edge[at + k];
        if (e < 0 || edge_state[e] != FLIPPED) continue;
        const int32_t apex = v[(k + 2) % 3];
        if (v[k] == edge_vertices[2 * (size_t)e]) { o[0] = v[k]; o[1] = edge_opposite[2 * (size_t)e + 1]; o[2] = apex; }
        else { o[0] = apex; o[1] = v[k]; o[2] = edge_opposite[2 * (size_t)e]; }
        flipped = 1;
    }
    out_faces[at] = o[0]; out_faces[at + 1] = o[1]; out_faces[at + 2] = o[2];
    face_flipped[f] = flipped;
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------
struct FlipCarve
{
    EdgeSortCarve sort;
    uint32_t *eid, *start, *end, *prio, *win, *rank, *block_sum, *total; // total: {edges, winners}
    int32_t *half_edge_edge;
    uint32_t *wk[2], *wv[2]; // the winners' list, cap words each
    void *wscratch;
    size_t cap, bytes;
};
FlipCarve flip_carve(void *ws, size_t F)
{
    FlipCarve c;
    Carver w(ws);
    const size_t N = 3 * F;
    c.cap = F / 2 > 0 ? F / 2 : 1;
    c.sort = edge_sort_carve(w, N);
    c.eid = w.words(N); c.start = w.words(N); c.end = w.words(N); c.prio = w.words(N); c.win = w.words(N); c.rank = w.words(N);
    c.half_edge_edge = (int32_t *)w.words(N);
    c.block_sum = w.words(scan_blocks(N));
    c.total = w.words(4);
    c.wk[0] = w.words(c.cap); c.wk[1] = w.words(c.cap); c.wv[0] = w.words(c.cap); c.wv[1] = w.words(c.cap);
    c.wscratch = w.bytes(sort_scratch_bytes(c.cap));
    c.bytes = w.used();
    return c;
}
} // namespace

size_t ts_flip_workspace_bytes(int V, int F)
{
    (void)V;
    return flip_carve(nullptr, (size_t)(F > 0 ? F : 0)).bytes + 2 * TS_ALIGN;
}

hipError_t ts_flip_round(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, float min_cos, uint32_t seed,
                         int32_t *out_faces, uint8_t *face_flipped, int32_t *edge_vertices, uint8_t *edge_state, int32_t *edge_opposite,
                         unsigned long long *totals, void *ws, hipStream_t s)
{
    hipError_t e = mesh_fill(totals, 0, 4 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    if (F <= 0) return hipSuccess;
    const size_t f = (size_t)F, N = 3 * f;
    const FlipCarve c = flip_carve(ws, f);
    const unsigned nf = blocks256(f), nh = blocks256(N);
    if (V > 0)
    {
        hipLaunchKernelGGL(records_kernel, dim3(nf), dim3(256), 0, s, V, F, faces, keep, c.sort.k[0], c.sort.v[0]);
        const SortedEdges edges = sort_half_edges(V, N, faces, c.sort, s);
        hipLaunchKernelGGL(heads_kernel, dim3(nh), dim3(256), 0, s, V, N, edges.smin, edges.smax, c.eid);
        scan_columns<1>(N, {{c.eid}}, c.block_sum, c.total, s); // the flags become the number of heads in front
        hipLaunchKernelGGL(runs_kernel, dim3(nh), dim3(256), 0, s, V, N, edges.smin, edges.smax, c.eid, c.start, c.end);
        hipLaunchKernelGGL(classify_kernel, dim3(nh), dim3(256), 0, s, N, vertices, faces, edges.smin, edges.smax, edges.sval,
                           (const uint32_t *)c.start, (const uint32_t *)c.end, (const uint32_t *)c.total, (double)min_cos, seed, edge_vertices,
                           edge_state, edge_opposite, c.prio, totals);
        hipLaunchKernelGGL(scatter_kernel, dim3(nh), dim3(256), 0, s, N, edges.sval, (const uint32_t *)c.eid, c.half_edge_edge);
        hipLaunchKernelGGL(winner_kernel, dim3(nh), dim3(256), 0, s, N, (const uint32_t *)c.total, (const uint32_t *)c.start, edges.sval,
                           (const int32_t *)c.half_edge_edge, (const uint8_t *)edge_state, (const uint32_t *)c.prio, c.win, c.rank);
        scan_columns<1>(N, {{c.rank}}, c.block_sum, c.total + 1, s); // the flags become the winners' ranks
        hipLaunchKernelGGL(compact_kernel, dim3(nh), dim3(256), 0, s, V, N, c.cap, (const uint32_t *)(c.total + 1), (const uint32_t *)c.win,
                           (const uint32_t *)c.rank, (const int32_t *)edge_opposite, c.wk[0], c.wv[0]);
        const int bits = bit_length((uint32_t)V); // the sentinel V included
        const unsigned nw = blocks256(c.cap);
        const int at = ts_radix_sort_pairs(c.wk, c.wv, c.cap, bits, c.wscratch, s); // by the larger new end, stable
        hipLaunchKernelGGL(smaller_end_kernel, dim3(nw), dim3(256), 0, s, V, c.cap, (const uint32_t *)c.wv[at], (const int32_t *)edge_opposite,
                           c.wk[at ^ 1]);
        uint32_t *const k2[2] = {c.wk[at ^ 1], c.wk[at]}, *const v2[2] = {c.wv[at], c.wv[at ^ 1]};
        const int at2 = ts_radix_sort_pairs(k2, v2, c.cap, bits, c.wscratch, s); // then by the smaller: (smaller, larger, edge id) order
        hipLaunchKernelGGL(flip_kernel, dim3(nw), dim3(256), 0, s, c.cap, (const uint32_t *)v2[at2], (const int32_t *)edge_opposite, edge_state,
                           totals);
    }
    else // nothing takes part
    {
        if ((e = mesh_fill(edge_vertices, 0xFF, 2 * N * sizeof(int32_t), s)) != hipSuccess) return e;
        if ((e = mesh_fill(edge_opposite, 0xFF, 2 * N * sizeof(int32_t), s)) != hipSuccess) return e;
        if ((e = mesh_fill(edge_state, NO_EDGE, N, s)) != hipSuccess) return e;
        if (out_faces && (e = mesh_fill(c.half_edge_edge, 0xFF, N * sizeof(int32_t), s)) != hipSuccess) return e;
    }
    if (out_faces)
        hipLaunchKernelGGL(apply_kernel, dim3(nf), dim3(256), 0, s, F, faces, (const int32_t *)c.half_edge_edge, (const uint8_t *)edge_state,
                           (const int32_t *)edge_vertices, (const int32_t *)edge_opposite, out_faces, face_flipped);
    return hipGetLastError();
}
