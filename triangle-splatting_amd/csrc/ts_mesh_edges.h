// ts_mesh_edges.h -- the sort-by-edge front of mesh_manifold.hip and mesh_orient.hip, single-sourced: the half-edges of the faces that take
// part, in (smaller end, larger end, half-edge) order.
//
// One thread per face writes its three half-edge records (half_edge_records: key max(tail, head), value the half-edge, the sentinel key V
// for a face that does not take part, which sorts behind every real one) in a kernel of the unit's own, which initialises the unit's
// parent words and counts what the unit counts beside them.  sort_half_edges then runs a stable LSD sort by the larger end, a gather of the
// smaller end in that order, a second stable sort by the smaller end (the product's radix passes, only the bits V needs) and a gather of the
// larger end.  What a unit does with the runs of equal edges (edge_run_head, ts_mesh_common.h) is its own.
//
// Not shared on purpose: mesh_weld.hip's census keys (a face with a repeated index takes part there and yields an edge (a, a)) and
// mesh_smooth.hip's six directed records per face.
#pragma once
#include "ts_mesh_common.h"

namespace
{
// The three records of face f at 3 f .. 3 f + 2; v: the face's indices, read only where ok.  f < F.
__device__ __forceinline__ void half_edge_records(int V, size_t f, bool ok, const int32_t (&v)[3], uint32_t *__restrict__ key,
                                                  uint32_t *__restrict__ val)
{
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const size_t c = 3 * f + k;
        key[c] = ok ? (uint32_t)max(v[k], v[(k + 1) % 3]) : (uint32_t)V;
        val[c] = (uint32_t)c;
    }
}

// The sentinel keys sort last, so a position whose first key is V holds a half-edge that does not take part: its other end is V too.  A
// real half-edge's face took part when the records were written, so both ends are in [0, V); val < N by construction.
__global__ void __launch_bounds__(256) other_end_kernel(int V, size_t N, const int32_t *__restrict__ faces, const uint32_t *__restrict__ skey,
                                                         const uint32_t *__restrict__ sval, bool smaller, uint32_t *__restrict__ out)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    uint32_t r = (uint32_t)V;
    if (skey[j] < (uint32_t)V)
    {
        const uint32_t h = sval[j];
        const int32_t a = faces[h], b = faces[next_corner(h)];
        r = (uint32_t)(smaller ? min(a, b) : max(a, b));
    }
    out[j] = r;
}

struct EdgeSortCarve // N words each: the records are written to k[0], v[0]
{
    uint32_t *k[2], *v[2], *other;
    void *scratch;
};
inline EdgeSortCarve edge_sort_carve(Carver &w, size_t N)
{
    EdgeSortCarve c;
    c.k[0] = w.words(N); c.k[1] = w.words(N); c.v[0] = w.words(N); c.v[1] = w.words(N);
    c.other = w.words(N);
    c.scratch = w.bytes(sort_scratch_bytes(N));
    return c;
}

struct SortedEdges // per sorted position: the smaller end, the larger end, the half-edge
{
    const uint32_t *smin, *smax, *sval;
};
// The records of N = 3 F half-edges are in c.k[0], c.v[0]; V > 0.  Two launches besides the sorts' own.
inline SortedEdges sort_half_edges(int V, size_t N, const int32_t *faces, const EdgeSortCarve &c, hipStream_t s)
{
    const int bits = bit_length((uint32_t)V); // the sentinel V included
    const unsigned nh = blocks256(N);
    const int at = ts_radix_sort_pairs(c.k, c.v, N, bits, c.scratch, s); // by the larger end, stable
    hipLaunchKernelGGL(other_end_kernel, dim3(nh), dim3(256), 0, s, V, N, faces, c.k[at], c.v[at], true, c.k[at ^ 1]);
    // the gathered smaller ends are the next keys; the values stay where the first sort left them
    uint32_t *const k2[2] = {c.k[at ^ 1], c.k[at]}, *const v2[2] = {c.v[at], c.v[at ^ 1]};
    const int at2 = ts_radix_sort_pairs(k2, v2, N, bits, c.scratch, s); // then by the smaller end, stable: (min, max, half-edge) order
    hipLaunchKernelGGL(other_end_kernel, dim3(nh), dim3(256), 0, s, V, N, faces, k2[at2], v2[at2], false, c.other);
    return {k2[at2], c.other, v2[at2]};
}
} // namespace
