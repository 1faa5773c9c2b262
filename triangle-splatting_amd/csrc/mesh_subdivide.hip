// mesh_subdivide.hip -- the edge table of an indexed mesh and the conforming 1-to-2/3/4 split at the midpoints of its marked edges
// (include/ts_subdivide.h).
//
// The arithmetic is float64 on the fp32 inputs widened, every operation rounded: the unit is built with -ffp-contract=off.  The only atomics
// are the integer adds of the counters.
//
// Edges.  The sort-by-edge front shared with mesh_manifold.hip and mesh_orient.hip (csrc/ts_mesh_edges.h) leaves the half-edges of the faces
// that take part in (lo, hi) order; the records kernel is this unit's own and counts nothing.  One thread per sorted position flags the head
// of its run (edge_run_head, csrc/ts_mesh_common.h); one exclusive prefix sum of the flags (scan_columns, csrc/ts_mesh_scan.h) numbers the
// edges in that order.  A second pass over the sorted positions turns the sum into the position's edge id, in place, and the head and the tail
// of every run write its bounds.  One thread per edge reads (lo, hi) at the head of its run -- coalesced along the sorted order -- gathers the
// two 12-byte vertex rows behind them, forms length2, decides the mark and writes the use count; past E it writes the fill values.
//
// Split.  The marks are summed per block (scan_count_kernel), one workgroup turns the sums into offsets (scan_offsets_kernel), and the apply
// pass is this unit's own: every marked edge takes its rank off the running sum and writes its midpoint, attributes and (lo, hi) at once;
// every edge learns its midpoint id or -1.  One thread per sorted position scatters edge and midpoint ids to the half-edges.  One thread per
// face counts its pieces (1 + its marked edges); their exclusive prefix sum places the output faces; one thread per parent face writes them.
// The fill values past the numbers written come from two tail kernels that read the totals on the device: no host read anywhere.
#include "ts_subdivide_launch.h"
#include "ts_mesh_edges.h"
#include "ts_mesh_scan.h"

namespace
{
constexpr int MARK_ALL = 0, MARK_LONGER = 1; // TSD_MARK_ALL, TSD_MARK_LONGER; anything else is TSD_MARK_VERTEX_LIMIT (api_subdivide.hip checks)

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

__device__ __forceinline__ double quiet_nan64() { return __longlong_as_double(0x7FF8000000000000ll); }

// (dx dx + dy dy) + dz dz with d = q - p on the widened rows
__device__ __forceinline__ double squared_length(const float *__restrict__ p, const float *__restrict__ q)
{
    const double dx = (double)q[0] - (double)p[0], dy = (double)q[1] - (double)p[1], dz = (double)q[2] - (double)p[2];
    return (dx * dx + dy * dy) + dz * dz;
}

struct MarkRule
{
    int mode;                  // TSD_MARK_*
    double max2;               // (double)max_edge * (double)max_edge
    const float *vertex_limit; // V floats in TSD_MARK_VERTEX_LIMIT
};

// One thread = one edge slot, e < N = 3 F.  Below E (total[0]): lo and hi from the head of the run (both in [0, V): the face took part), the
// use count from the run's bounds, length2 and the mark from the two vertex rows.  Past E: the fill values.  Any output pointer may be null;
// vertices is read only where length2 or the mark is asked for.
__global__ void __launch_bounds__(256) edge_kernel(size_t N, const float *__restrict__ vertices, const uint32_t *__restrict__ smin,
                                                    const uint32_t *__restrict__ smax, const uint32_t *__restrict__ start,
                                                    const uint32_t *__restrict__ end, const uint32_t *__restrict__ total, MarkRule rule,
                                                    int32_t *__restrict__ edge_vertices, int32_t *__restrict__ edge_use,
                                                    double *__restrict__ edge_length2, uint32_t *__restrict__ mark, unsigned long long *counts)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t c[4] = {0, 0, 0, 0};
    if (e < N)
    {
        int32_t lo = -1, hi = -1, use = 0;
        double l2 = 0.0;
        uint32_t m = 0;
        if (e < (size_t)*total)
        {
            const uint32_t j = start[e];
            lo = (int32_t)smin[j]; hi = (int32_t)smax[j]; use = (int32_t)(end[e] - j);
            c[0] = 1; c[1] = use == 1; c[2] = use == 2; c[3] = use >= 3;
            if (edge_length2 || mark)
            {
                const float *p = vertices + 3 * (size_t)lo, *q = vertices + 3 * (size_t)hi;
                const bool fin = finite32(p[0]) && finite32(p[1]) && finite32(p[2]) && finite32(q[0]) && finite32(q[1]) && finite32(q[2]);
                l2 = fin ? squared_length(p, q) : quiet_nan64();
                if (fin)
                {
                    if (rule.mode == MARK_ALL) m = 1;
                    else if (rule.mode == MARK_LONGER) m = l2 > rule.max2;
                    else
                    {
                        const float la = rule.vertex_limit[lo], lb = rule.vertex_limit[hi];
                        if (la == la && lb == lb)
                        {
                            const double L = (double)(lb < la ? lb : la);
                            m = l2 > L * L;
                        }
                    }
                }
            }
        }
        if (edge_vertices) { edge_vertices[2 * e] = lo; edge_vertices[2 * e + 1] = hi; }
        if (edge_use) edge_use[e] = use;
        if (edge_length2) edge_length2[e] = l2;
        if (mark) mark[e] = m;
    }
    if (counts) count4_into(counts, c); // a kernel argument: the whole workgroup takes the same side
}

// One thread = one sorted position: the half-edge there learns its edge and, where mid is given, its midpoint.  sval is a permutation of
// [0, N), so every half-edge is written; an edge id that is not -1 is below E.
__global__ void __launch_bounds__(256) scatter_kernel(size_t N, const uint32_t *__restrict__ sval, const uint32_t *__restrict__ eid,
                                                       const int32_t *__restrict__ edge_mid, int32_t *__restrict__ half_edge_edge,
                                                       int32_t *__restrict__ half_edge_mid)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const uint32_t h = sval[j];
    const int32_t e = (int32_t)eid[j];
    if (half_edge_edge) half_edge_edge[h] = e;
    if (half_edge_mid) half_edge_mid[h] = e >= 0 ? edge_mid[e] : -1;
}

// ---- split -------------------------------------------------------------------------------------------------------------------------------
struct Attributes
{
    const float *values;  // V x channels, or null with channels == 0
    const uint8_t *valid; // V bytes, or null: all valid
    int channels;
};

// The apply pass of the prefix sum over the marks (block_offset: scan_offsets_kernel's), eight consecutive edges per lane as in
// csrc/ts_mesh_scan.h.  A marked edge is below E, so ev holds its ends, both in [0, V); its rank is below the number of marked edges <= N.
__global__ void __launch_bounds__(256) midpoints_kernel(int V, size_t N, const float *__restrict__ vertices, const int32_t *__restrict__ ev,
                                                         const uint32_t *__restrict__ mark, const uint32_t *__restrict__ block_offset,
                                                         Attributes at, int32_t *__restrict__ edge_mid, float *__restrict__ new_vertices,
                                                         float *__restrict__ new_attributes, uint8_t *__restrict__ new_attr_valid,
                                                         int32_t *__restrict__ new_vertex_edge)
{
    __shared__ uint32_t lds[4];
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
    uint32_t m[SCAN_PER], run = 0, all;
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++)
    {
        m[k] = base + k < N ? mark[base + k] : 0u;
        run += m[k];
    }
    run = block_offset[blockIdx.x] + block_scan256(run, lds, &all);
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++)
    {
        const size_t e = base + k;
        if (e >= N) break;
        if (!m[k])
        {
            edge_mid[e] = -1;
            continue;
        }
        const size_t r = run++;
        const int32_t lo = ev[2 * e], hi = ev[2 * e + 1];
        edge_mid[e] = (int32_t)((uint32_t)V + (uint32_t)r);
        new_vertex_edge[2 * r] = lo; new_vertex_edge[2 * r + 1] = hi;
        const float *p = vertices + 3 * (size_t)lo, *q = vertices + 3 * (size_t)hi;
#pragma unroll
        for (int a = 0; a < 3; a++) new_vertices[3 * r + a] = (float)(((double)p[a] + (double)q[a]) * 0.5);
        if (at.channels > 0)
        {
            const bool vl = !at.valid || at.valid[lo], vh = !at.valid || at.valid[hi];
            const float *al = at.values + (size_t)lo * at.channels, *ah = at.values + (size_t)hi * at.channels;
            float *out = new_attributes + r * at.channels;
            for (int ch = 0; ch < at.channels; ch++)
                out[ch] = vl && vh ? (float)(((double)al[ch] + (double)ah[ch]) * 0.5) : vl ? al[ch] : vh ? ah[ch] : 0.0f;
            new_attr_valid[r] = vl || vh;
        }
    }
}

// One thread = one new-vertex slot, r < N: the fill values from the number of marked edges (*marked) on.
__global__ void __launch_bounds__(256) vertex_tail_kernel(size_t N, const uint32_t *__restrict__ marked, int channels, float *__restrict__ new_vertices,
                                                           float *__restrict__ new_attributes, uint8_t *__restrict__ new_attr_valid,
                                                           int32_t *__restrict__ new_vertex_edge)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= N || r < (size_t)*marked) return;
    new_vertices[3 * r] = new_vertices[3 * r + 1] = new_vertices[3 * r + 2] = 0.0f;
    new_vertex_edge[2 * r] = new_vertex_edge[2 * r + 1] = -1;
    if (channels > 0)
    {
        for (int ch = 0; ch < channels; ch++) new_attributes[r * channels + ch] = 0.0f;
        new_attr_valid[r] = 0;
    }
}

// One thread = one face: 1 + the number of its half-edges with a midpoint (none where the face does not take part).
__global__ void __launch_bounds__(256) pieces_kernel(int F, const int32_t *__restrict__ half_edge_mid, uint32_t *__restrict__ pieces,
                                                      unsigned long long *totals)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    uint32_t n = 1;
    if (f < F)
    {
#pragma unroll
        for (int k = 0; k < 3; k++) n += half_edge_mid[3 * (size_t)f + k] >= 0;
        pieces[f] = n;
    }
    count_into(totals + 3, n > 1);
}

__device__ __forceinline__ void put_face(int32_t *__restrict__ out_faces, int32_t *__restrict__ parent, size_t at, int f, int32_t a, int32_t b, int32_t c)
{
    out_faces[3 * at] = a; out_faces[3 * at + 1] = b; out_faces[3 * at + 2] = c;
    parent[at] = f;
}

// One thread = one parent face; offset: the exclusive prefix sum of the piece counts, so the pieces of face f land at offset[f] .. below
// the total <= 4 F.  A midpoint id is V + r with r below the number of new vertices; two marked edges mean the face took part and all three
// of its vertices are finite and in [0, V).
__global__ void __launch_bounds__(256) emit_kernel(int V, int F, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                    const int32_t *__restrict__ half_edge_mid, const uint32_t *__restrict__ offset,
                                                    const float *__restrict__ new_vertices, int32_t *__restrict__ out_faces,
                                                    int32_t *__restrict__ out_face_parent)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int32_t v[3], m[3];
    int n = 0;
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        v[k] = faces[3 * (size_t)f + k];
        m[k] = half_edge_mid[3 * (size_t)f + k];
        n += m[k] >= 0;
    }
    const size_t at = offset[f];
    if (n == 0) put_face(out_faces, out_face_parent, at, f, v[0], v[1], v[2]);
    else if (n == 3)
    {
        put_face(out_faces, out_face_parent, at, f, v[0], m[0], m[2]);
        put_face(out_faces, out_face_parent, at + 1, f, m[0], v[1], m[1]);
        put_face(out_faces, out_face_parent, at + 2, f, m[2], m[1], v[2]);
        put_face(out_faces, out_face_parent, at + 3, f, m[0], m[1], m[2]);
    }
    else
    {
        const int k = n == 1 ? (m[0] >= 0 ? 0 : m[1] >= 0 ? 1 : 2) : (m[0] < 0 ? 0 : m[1] < 0 ? 1 : 2); // the marked corner / the unmarked one
        const int32_t a = v[k], b = v[(k + 1) % 3], c = v[(k + 2) % 3];
        if (n == 1)
        {
            put_face(out_faces, out_face_parent, at, f, a, m[k], c);
            put_face(out_faces, out_face_parent, at + 1, f, m[k], b, c);
        }
        else
        {
            const int32_t m1 = m[(k + 1) % 3], m2 = m[(k + 2) % 3];
            put_face(out_faces, out_face_parent, at, f, m1, c, m2);
            const double d1 = squared_length(vertices + 3 * (size_t)a, new_vertices + 3 * (size_t)(m1 - V));
            const double d2 = squared_length(vertices + 3 * (size_t)b, new_vertices + 3 * (size_t)(m2 - V));
            if (d1 < d2 || (d1 == d2 && a < b))
            {
                put_face(out_faces, out_face_parent, at + 1, f, a, b, m1);
                put_face(out_faces, out_face_parent, at + 2, f, a, m1, m2);
            }
            else
            {
                put_face(out_faces, out_face_parent, at + 1, f, a, b, m2);
                put_face(out_faces, out_face_parent, at + 2, f, b, m1, m2);
            }
        }
    }
}

// One thread = one output face slot, i < 4 F: -1 from the number of output faces on.  The first thread writes the three totals that are sums.
__global__ void __launch_bounds__(256) face_tail_kernel(size_t capacity, const uint32_t *__restrict__ total, int32_t *__restrict__ out_faces,
                                                         int32_t *__restrict__ out_face_parent, unsigned long long *__restrict__ totals)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0)
    {
        totals[0] = total[0]; totals[1] = total[1]; totals[2] = total[2];
    }
    if (i >= capacity || i < (size_t)total[2]) return;
    out_faces[3 * i] = out_faces[3 * i + 1] = out_faces[3 * i + 2] = -1;
    out_face_parent[i] = -1;
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------
struct SubdivideCarve
{
    EdgeSortCarve sort;
    uint32_t *eid, *start, *end, *mark, *pieces, *block_sum, *total; // total: {edges, marked, out_faces}
    int32_t *ev, *edge_mid, *half_edge_mid;
    size_t bytes;
};
SubdivideCarve subdivide_carve(void *ws, size_t F)
{
    SubdivideCarve c;
    Carver w(ws);
    const size_t N = 3 * F;
    c.sort = edge_sort_carve(w, N);
    c.eid = w.words(N); c.start = w.words(N); c.end = w.words(N); c.mark = w.words(N);
    c.ev = (int32_t *)w.words(2 * N);
    c.edge_mid = (int32_t *)w.words(N);
    c.half_edge_mid = (int32_t *)w.words(N);
    c.pieces = w.words(F);
    c.block_sum = w.words(scan_blocks(N));
    c.total = w.words(4);
    c.bytes = w.used();
    return c;
}

// The edge table of N = 3 F > 0 half-edges, V > 0: c.eid per sorted position, c.total[0] = E, then edge_kernel with the outputs given.
SortedEdges edge_table(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, const SubdivideCarve &c, const MarkRule &rule,
                       int32_t *edge_vertices, int32_t *edge_use, double *edge_length2, uint32_t *mark, unsigned long long *counts, hipStream_t s)
{
    const size_t N = 3 * (size_t)F;
    const unsigned nf = blocks256((size_t)F), nh = blocks256(N);
    hipLaunchKernelGGL(records_kernel, dim3(nf), dim3(256), 0, s, V, F, faces, keep, c.sort.k[0], c.sort.v[0]);
    const SortedEdges edges = sort_half_edges(V, N, faces, c.sort, s);
    hipLaunchKernelGGL(heads_kernel, dim3(nh), dim3(256), 0, s, V, N, edges.smin, edges.smax, c.eid);
    scan_columns<1>(N, {{c.eid}}, c.block_sum, c.total, s); // the flags become the number of heads in front
    hipLaunchKernelGGL(runs_kernel, dim3(nh), dim3(256), 0, s, V, N, edges.smin, edges.smax, c.eid, c.start, c.end);
    hipLaunchKernelGGL(edge_kernel, dim3(nh), dim3(256), 0, s, N, vertices, edges.smin, edges.smax, c.start, c.end, c.total, rule, edge_vertices,
                       edge_use, edge_length2, mark, counts);
    return edges;
}
} // namespace

size_t ts_subdivide_workspace_bytes(int V, int F)
{
    (void)V;
    return subdivide_carve(nullptr, (size_t)(F > 0 ? F : 0)).bytes + 2 * TS_ALIGN;
}

hipError_t ts_subdivide_edges(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, int32_t *edge_vertices,
                              int32_t *edge_use, double *edge_length2, int32_t *half_edge_edge, unsigned long long *counts, void *ws,
                              hipStream_t s)
{
    hipError_t e = mesh_fill(counts, 0, 4 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const size_t N = 3 * (size_t)(F > 0 ? F : 0);
    if (N == 0) return hipSuccess;
    if (V <= 0) // nothing takes part
    {
        if ((e = mesh_fill(edge_vertices, 0xFF, 2 * N * sizeof(int32_t), s)) != hipSuccess) return e;
        if ((e = mesh_fill(edge_use, 0, N * sizeof(int32_t), s)) != hipSuccess) return e;
        if (edge_length2 && (e = mesh_fill(edge_length2, 0, N * sizeof(double), s)) != hipSuccess) return e;
        return mesh_fill(half_edge_edge, 0xFF, N * sizeof(int32_t), s);
    }
    const SubdivideCarve c = subdivide_carve(ws, (size_t)F);
    const SortedEdges edges = edge_table(V, F, vertices, faces, keep, c, MarkRule{MARK_ALL, 0.0, nullptr}, edge_vertices, edge_use, edge_length2,
                                         nullptr, counts, s);
    hipLaunchKernelGGL(scatter_kernel, dim3(blocks256(N)), dim3(256), 0, s, N, edges.sval, c.eid, (const int32_t *)nullptr, half_edge_edge,
                       (int32_t *)nullptr);
    return hipGetLastError();
}

hipError_t ts_subdivide_split(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, int mode, float max_edge,
                              const float *vertex_limit, const float *attributes, const uint8_t *attr_valid, int channels, float *new_vertices,
                              float *new_attributes, uint8_t *new_attr_valid, int32_t *new_vertex_edge, int32_t *out_faces,
                              int32_t *out_face_parent, unsigned long long *totals, void *ws, hipStream_t s)
{
    hipError_t e = mesh_fill(totals, 0, 4 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    if (F <= 0) return hipSuccess;
    const size_t f = (size_t)F, N = 3 * f;
    const SubdivideCarve c = subdivide_carve(ws, f);
    const unsigned nf = blocks256(f), nh = blocks256(N);
    if ((e = mesh_fill(c.total, 0, 4 * sizeof(uint32_t), s)) != hipSuccess) return e;
    if (V > 0)
    {
        const MarkRule rule{mode, (double)max_edge * (double)max_edge, vertex_limit};
        const SortedEdges edges = edge_table(V, F, vertices, faces, keep, c, rule, c.ev, nullptr, nullptr, c.mark, nullptr, s);
        const unsigned nb = (unsigned)scan_blocks(N);
        hipLaunchKernelGGL(scan_count_kernel<1>, dim3(nb), dim3(256), 0, s, N, ScanColumns<1>{{c.mark}}, c.block_sum);
        hipLaunchKernelGGL(scan_offsets_kernel<1>, dim3(1), dim3(256), 0, s, (int)nb, c.block_sum, c.total + 1);
        hipLaunchKernelGGL(midpoints_kernel, dim3(nb), dim3(256), 0, s, V, N, vertices, (const int32_t *)c.ev, (const uint32_t *)c.mark,
                           (const uint32_t *)c.block_sum, Attributes{attributes, attr_valid, channels}, c.edge_mid, new_vertices, new_attributes,
                           new_attr_valid, new_vertex_edge);
        hipLaunchKernelGGL(scatter_kernel, dim3(nh), dim3(256), 0, s, N, edges.sval, (const uint32_t *)c.eid, (const int32_t *)c.edge_mid,
                           (int32_t *)nullptr, c.half_edge_mid);
    }
    else if ((e = mesh_fill(c.half_edge_mid, 0xFF, N * sizeof(int32_t), s)) != hipSuccess) return e; // nothing takes part
    hipLaunchKernelGGL(vertex_tail_kernel, dim3(nh), dim3(256), 0, s, N, (const uint32_t *)(c.total + 1), channels, new_vertices, new_attributes,
                       new_attr_valid, new_vertex_edge);
    hipLaunchKernelGGL(pieces_kernel, dim3(nf), dim3(256), 0, s, F, (const int32_t *)c.half_edge_mid, c.pieces, totals);
    scan_columns<1>(f, {{c.pieces}}, c.block_sum, c.total + 2, s); // the piece counts become the faces' places
    hipLaunchKernelGGL(emit_kernel, dim3(nf), dim3(256), 0, s, V, F, vertices, faces, (const int32_t *)c.half_edge_mid, (const uint32_t *)c.pieces,
                       (const float *)new_vertices, out_faces, out_face_parent);
    hipLaunchKernelGGL(face_tail_kernel, dim3(blocks256(4 * f)), dim3(256), 0, s, 4 * f, (const uint32_t *)c.total, out_faces, out_face_parent, totals);
    return hipGetLastError();
}
