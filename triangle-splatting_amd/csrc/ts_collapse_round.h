// ts_collapse_round.h -- what the two half-edge collapse units share, single-sourced: mesh_collapse.hip (include/ts_collapse.h, short edges
// first) and mesh_decimate.hip (include/ts_decimate.h, cheapest quadric error first).  The corner records and the clean-edge flags, the
// vertex classes with the ring bounds, the three guards of a direction (direction_guards), the 32-bit priority, the binary search of the
// edge table (table_has), and the round's selection and collapse: best, best2, the winners and the face map.
//
// The two units differ in how they order their candidates, so the selection is written once over an ORDER: a small struct passed by value
// whose comes_first(a, b) says whether candidate a comes before candidate b in the unit's total order; NONE comes last.  The bodies are
// device functions; each unit wraps them in kernels of its own, so that a kernel keeps its name and its resource figures per unit.  The
// kernels defined here are no templates: both units launch every one of them.
//
// The values of the states and bits that both headers give the same numbers are named once below (TSP_* of include/ts_collapse.h).
#pragma once
#include "ts_mesh_edge_ids.h"

namespace
{
constexpr uint8_t NO_EDGE = 0, NOT_ELIGIBLE = 1, GUARDED = 3, LOST = 4, COLLAPSED = 5;  // TSP_*; 2 is the unit's own
constexpr uint8_t GUARD_LINK = 1, GUARD_LONG = 2, GUARD_NORMAL = 4, GUARD_HELD = 8;    // TSP_GUARD_*
constexpr uint32_t MAX_RING = 64;      // TSP_MAX_RING
constexpr uint32_t NONE = 0xFFFFFFFFu; // no candidate
constexpr uint8_t HELD = 0, FREE = 1;

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

// ---- selection ---------------------------------------------------------------------------------------------------------------------------
struct Rings // the corners sorted by vertex and every vertex's run among them
{
    const uint32_t *ring_val, *ring_start, *ring_end;
};

// The body of one thread = one vertex: the first candidate, by `order`, among the edges at it.  Every edge at v lies in a ring face of v, as
// the half-edge that leaves v or the one that arrives.  A candidate is an edge whose state is LOST.
template <typename Order>
__device__ __forceinline__ void best_of_edges(int V, const Rings &g, const int32_t *__restrict__ half_edge_edge,
                                              const uint8_t *__restrict__ edge_state, const Order &order, uint32_t *__restrict__ best)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    uint32_t b = NONE;
    for (uint32_t j = g.ring_start[v], re = g.ring_end[v]; j < re; j++)
    {
        const uint32_t h = g.ring_val[j];
        const uint32_t e0 = (uint32_t)half_edge_edge[h], e1 = (uint32_t)half_edge_edge[prev_corner(h)];
        if (edge_state[e0] == LOST && order.comes_first(e0, b)) b = e0;
        if (edge_state[e1] == LOST && order.comes_first(e1, b)) b = e1;
    }
    best[v] = b;
}

// The body of one thread = one vertex: the first among best[u] over v and the vertices adjacent to it, the two other corners of every ring
// face.
template <typename Order>
__device__ __forceinline__ void best_of_ring(int V, const int32_t *__restrict__ faces, const Rings &g, const Order &order,
                                             const uint32_t *__restrict__ best, uint32_t *__restrict__ best2)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    uint32_t b = best[v];
    for (uint32_t j = g.ring_start[v], re = g.ring_end[v]; j < re; j++)
    {
        const uint32_t h = g.ring_val[j];
        const uint32_t bx = best[faces[next_corner(h)]], by = best[faces[next_corner(next_corner(h))]];
        if (order.comes_first(bx, b)) b = bx;
        if (order.comes_first(by, b)) b = by;
    }
    best2[v] = b;
}

// The body of one thread = one edge slot: a candidate that is the first of the closed rings of both its ends collapses.  Every lane
// reaches count_into; `counter` is the unit's word for the collapsed edges.
__device__ __forceinline__ void decide_winner(size_t N, const uint32_t *__restrict__ total, const int32_t *__restrict__ edge_vertices,
                                              const int32_t *__restrict__ edge_removed, const uint32_t *__restrict__ best2,
                                              uint8_t *__restrict__ edge_state, int32_t *__restrict__ vertex_target, unsigned long long *counter)
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
    count_into(counter, won);
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
} // namespace
