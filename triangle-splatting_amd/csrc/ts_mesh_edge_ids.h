// ts_mesh_edge_ids.h -- from the sorted half-edges of ts_mesh_edges.h to numbered edges, single-sourced: run heads (edge_run_head) become
// edge ids by one exclusive prefix sum (scan_columns, ts_mesh_scan.h), the head and the tail of every run write its bounds, and one scatter
// hands the edge ids to the half-edges.  mesh_collapse.hip includes it; mesh_subdivide.hip and mesh_flip.hip still carry the copies this
// was taken from.  The kernels are no templates: a unit that includes this header launches them (number_edges).
#pragma once
#include "ts_mesh_edges.h"
#include "ts_mesh_scan.h"

namespace
{
// One thread = one sorted position: 1 at the head of a run of a real edge.
__global__ void __launch_bounds__(256) edge_heads_kernel(int V, size_t N, const uint32_t *__restrict__ smin, const uint32_t *__restrict__ smax,
                                                          uint32_t *__restrict__ head)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    head[j] = edge_run_head(V, N, j, smin, smax) != 0;
}

// One thread = one sorted position.  eid[j] holds the number of heads in front of j and becomes the edge id of the position, -1 (all bits)
// on a sentinel.  A real position lies in a run whose head was counted, so its id is below E <= N: start and end hold N words.
__global__ void __launch_bounds__(256) edge_ids_kernel(int V, size_t N, const uint32_t *__restrict__ smin, const uint32_t *__restrict__ smax,
                                                        uint32_t *__restrict__ eid, uint32_t *__restrict__ start, uint32_t *__restrict__ end)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const uint32_t a = smin[j], b = smax[j];
    if (a >= (uint32_t)V)
    {
        eid[j] = 0xFFFFFFFFu;
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
__global__ void __launch_bounds__(256) edge_scatter_kernel(size_t N, const uint32_t *__restrict__ sval, const uint32_t *__restrict__ eid,
                                                            int32_t *__restrict__ half_edge_edge)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    half_edge_edge[sval[j]] = (int32_t)eid[j];
}

struct EdgeIdCarve // N words each but block_sum (scan_blocks(N)) and total (four words, the first is E)
{
    uint32_t *eid, *start, *end, *block_sum, *total;
    int32_t *half_edge_edge;
};
inline EdgeIdCarve edge_id_carve(Carver &w, size_t N)
{
    EdgeIdCarve c;
    c.eid = w.words(N); c.start = w.words(N); c.end = w.words(N);
    c.half_edge_edge = (int32_t *)w.words(N);
    c.block_sum = w.words(scan_blocks(N));
    c.total = w.words(4);
    return c;
}

// The sorted half-edges of N = 3 F positions become numbered edges: *c.total = E, c.start / c.end the run of every edge below E, c.eid the
// edge of every sorted position and c.half_edge_edge the edge of every half-edge (-1 where its face does not take part).  Six launches.
inline void number_edges(int V, size_t N, const SortedEdges &edges, const EdgeIdCarve &c, hipStream_t s)
{
    const unsigned nh = blocks256(N);
    hipLaunchKernelGGL(edge_heads_kernel, dim3(nh), dim3(256), 0, s, V, N, edges.smin, edges.smax, c.eid);
    scan_columns<1>(N, {{c.eid}}, c.block_sum, c.total, s); // the flags become the number of heads in front
    hipLaunchKernelGGL(edge_ids_kernel, dim3(nh), dim3(256), 0, s, V, N, edges.smin, edges.smax, c.eid, c.start, c.end);
    hipLaunchKernelGGL(edge_scatter_kernel, dim3(nh), dim3(256), 0, s, N, edges.sval, (const uint32_t *)c.eid, c.half_edge_edge);
}
} // namespace
