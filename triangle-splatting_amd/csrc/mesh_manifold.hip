// mesh_manifold.hip -- the fans of every vertex of an indexed mesh, found and numbered, and the split that gives every extra fan a vertex
// of its own (include/ts_manifold.h).
//
// No floating-point arithmetic anywhere, so the unit needs no floating-point flags.  The atomics are integer: the compare-exchange and the
// minimum of the union-find (csrc/ts_union_find.h), the minimum that elects a vertex's keeper, the adds of the counters.
//
// Fans.  The sort-by-edge front shared with mesh_orient.hip (csrc/ts_mesh_edges.h) leaves the half-edges of the faces that take part in
// (min, max) order, ascending half-edge inside a run; the records kernel is this unit's own: it also sets the three parent words of a face
// and counts the corners.  One thread per sorted position classifies its run (edge_run_head, csrc/ts_mesh_common.h), looking at most two
// positions ahead: the head of a run of exactly two unites the two corners at either end of the edge in a parent array over
// the 3 F corners (uf_union; nobody waits for anybody) and counts the pair if both half-edges leave the same vertex; the head of a longer
// run counts a non-manifold edge and links nothing.  A flatten pass writes corner_fan[c] = root(c), the smallest corner of the fan whatever
// the order of the unions, and every root adds 1 to its vertex; a vertex pass takes the two vertex counts.
//
// Split.  One thread per corner validates its entry of corner_fan (in [0, 3 F), on a face that takes part, on the same vertex), marks the
// label as used and lowers the vertex's keeper to it.  A used label that is not its vertex's keeper is flagged; one exclusive prefix sum of
// the 3 F flags (scan_columns, csrc/ts_mesh_scan.h: per-block sums, one workgroup turns them into offsets, every block ranks its own behind
// the sum in front of it) numbers the new vertices in ascending label.  One thread per label writes the source and the label of a flagged
// one, one thread per corner writes out_faces.
#include "ts_manifold_launch.h"
#include "ts_mesh_edges.h"
#include "ts_mesh_scan.h"
#include "ts_union_find.h"

namespace
{
// ---- fans --------------------------------------------------------------------------------------------------------------------------------
// One thread = one face: its three records and the identity of its three parent words.
__global__ void __launch_bounds__(256) records_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep,
                                                       uint32_t *__restrict__ key, uint32_t *__restrict__ val, uint32_t *__restrict__ parent,
                                                       unsigned long long *counts)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    uint32_t n = 0;
    if (f < F)
    {
        int32_t v[3];
        const bool ok = face_takes_part(V, (size_t)f, faces, keep, v);
        half_edge_records(V, (size_t)f, ok, v, key, val);
#pragma unroll
        for (int k = 0; k < 3; k++) parent[3 * (size_t)f + k] = 3u * (uint32_t)f + k;
        n = ok ? 3u : 0u;
    }
    count_into(counts + 0, n);
}

// One thread = one sorted position.  The half-edges are below N and their corners' parent words with them.
__global__ void __launch_bounds__(256) link_kernel(int V, size_t N, const int32_t *__restrict__ faces, const uint32_t *__restrict__ smin,
                                                    const uint32_t *__restrict__ smax, const uint32_t *__restrict__ sval, uint32_t *parent,
                                                    unsigned long long *counts)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t nonmanifold = 0, same = 0;
    const int run = edge_run_head(V, N, j, smin, smax);
    if (run == 3) nonmanifold = 1;
    else if (run == 2) // j + 1 < N
    {
        const uint32_t h0 = sval[j], h1 = sval[j + 1];
        const uint32_t n0 = next_corner(h0), n1 = next_corner(h1);
        if (faces[h0] == faces[h1]) // both leave the same vertex: an orientation conflict, linked all the same
        {
            same = 1;
            uf_union(parent, h0, h1);
            uf_union(parent, n0, n1);
        }
        else
        {
            uf_union(parent, h0, n1);
            uf_union(parent, n0, h1);
        }
    }
    count_into(counts + 4, nonmanifold);
    count_into(counts + 5, same);
}

// One thread = one face: the roots of its three corners, or -1.  A root adds itself to its vertex, whose index was checked against V.
__global__ void __launch_bounds__(256) flatten_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep,
                                                       uint32_t *parent, int32_t *__restrict__ corner_fan, uint32_t *vertex_fans,
                                                       unsigned long long *counts)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    uint32_t roots = 0;
    if (f < F)
    {
        int32_t v[3];
        const bool ok = face_takes_part(V, (size_t)f, faces, keep, v);
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
            const uint32_t c = 3u * (uint32_t)f + k;
            int32_t fan = -1;
            if (ok)
            {
                const uint32_t r = uf_find(parent, c, false);
                fan = (int32_t)r;
                if (r == c)
                {
                    atomicAdd(vertex_fans + v[k], 1u);
                    roots++;
                }
            }
            corner_fan[c] = fan;
        }
    }
    count_into(counts + 1, roots);
}

__global__ void __launch_bounds__(256) vertex_census_kernel(int V, const uint32_t *__restrict__ vertex_fans, unsigned long long *counts)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    const uint32_t n = v < V ? vertex_fans[v] : 0u;
    count_into(counts + 2, n >= 1);
    count_into(counts + 3, n >= 2);
}

// ---- split -------------------------------------------------------------------------------------------------------------------------------
// One thread = one face.  lab[c] = the validated entry of corner_fan, or -1: in [0, 3 F), on a face that takes part, on c's vertex.
__global__ void __launch_bounds__(256) labels_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep,
                                                      const int32_t *__restrict__ corner_fan, int32_t *__restrict__ lab, uint32_t *used,
                                                      uint32_t *keeper)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int32_t v[3];
    const bool ok = face_takes_part(V, (size_t)f, faces, keep, v);
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const size_t c = 3 * (size_t)f + k;
        int32_t l = -1;
        if (ok)
        {
            const int32_t e = corner_fan[c];
            if (e >= 0 && (size_t)e < 3 * (size_t)F)
            {
                int32_t w[3];
                if (face_takes_part(V, (size_t)e / 3, faces, keep, w) && faces[e] == v[k]) l = e;
            }
        }
        lab[c] = l;
        if (l >= 0)
        {
            __hip_atomic_store(used + l, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicMin(keeper + v[k], (uint32_t)l);
        }
    }
}

// One thread = one corner, as a label: flagged iff some corner names it and it is not its vertex's keeper.  A used label passed
// labels_kernel's test, so its face takes part and faces[l] is in [0, V).
__global__ void __launch_bounds__(256) flag_kernel(size_t N, const int32_t *__restrict__ faces, const uint32_t *__restrict__ keeper, uint32_t *used)
{
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= N) return;
    uint32_t flag = 0;
    if (used[l]) flag = keeper[faces[l]] != (uint32_t)l;
    used[l] = flag;
}

// index: the exclusive prefix sum of the flags, total their sum.  The flags are gone, so a label reads its own off the sum: flagged iff the
// next index is one further.  A flagged label passed labels_kernel's test, so faces[l] is in [0, V); its index is below the number of new
// vertices, and a row is written only below the capacity.
__global__ void __launch_bounds__(256) sources_kernel(size_t N, const int32_t *__restrict__ faces, const uint32_t *__restrict__ index,
                                                       const uint32_t *__restrict__ total, int capacity,
                                                       int32_t *__restrict__ new_vertex_source, int32_t *__restrict__ new_vertex_fan)
{
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= N) return;
    const uint32_t i = index[l], next = l + 1 < N ? index[l + 1] : *total;
    if (next == i || i >= (uint32_t)capacity) return;
    new_vertex_source[i] = faces[l];
    new_vertex_fan[i] = (int32_t)l;
}

__global__ void __launch_bounds__(256) rewrite_kernel(int V, size_t N, const int32_t *__restrict__ faces, const int32_t *__restrict__ lab,
                                                       const uint32_t *__restrict__ keeper, const uint32_t *__restrict__ index,
                                                       int32_t *__restrict__ out_faces, unsigned long long *totals)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t moved = 0;
    if (c < N)
    {
        int32_t v = faces[c];
        const int32_t l = lab[c];
        if (l >= 0 && keeper[v] != (uint32_t)l)
        {
            v = (int32_t)((uint32_t)V + index[l]);
            moved = 1;
        }
        out_faces[c] = v;
    }
    count_into(totals + 1, moved);
}

__global__ void __launch_bounds__(256) split_finish_kernel(const uint32_t *__restrict__ total, unsigned long long *__restrict__ totals)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) totals[0] = *total;
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------
struct FansCarve
{
    EdgeSortCarve sort;
    uint32_t *parent;
    size_t bytes;
};
FansCarve fans_carve(void *ws, size_t F)
{
    FansCarve c;
    Carver w(ws);
    c.sort = edge_sort_carve(w, 3 * F);
    c.parent = w.words(3 * F);
    c.bytes = w.used();
    return c;
}

struct SplitCarve
{
    uint32_t *keeper, *flag, *block_sum, *total;
    int32_t *lab;
    size_t bytes;
};
SplitCarve split_carve(void *ws, size_t V, size_t F)
{
    SplitCarve c;
    Carver w(ws);
    const size_t N = 3 * F;
    c.keeper = w.words(V);
    c.lab = (int32_t *)w.words(N);
    c.flag = w.words(N);
    c.block_sum = w.words(scan_blocks(N));
    c.total = w.words(1);
    c.bytes = w.used();
    return c;
}
} // namespace

size_t ts_manifold_workspace_bytes(int V, int F)
{
    const size_t v = (size_t)(V > 0 ? V : 0), f = (size_t)(F > 0 ? F : 0);
    return std::max(fans_carve(nullptr, f).bytes, split_carve(nullptr, v, f).bytes) + 2 * TS_ALIGN;
}

hipError_t ts_manifold_fans(int V, int F, const int32_t *faces, const uint8_t *keep, int32_t *corner_fan, int32_t *vertex_fans,
                            unsigned long long *counts, void *ws, hipStream_t s)
{
    hipError_t e = mesh_fill(counts, 0, 6 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const size_t f = (size_t)(F > 0 ? F : 0), N = 3 * f;
    if (V > 0)
    {
        e = mesh_fill(vertex_fans, 0, (size_t)V * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
    }
    if (N == 0) return hipSuccess;
    if (V <= 0) return mesh_fill(corner_fan, 0xFF, N * sizeof(int32_t), s); // nothing takes part
    const FansCarve c = fans_carve(ws, f);
    const unsigned nf = blocks256(f), nh = blocks256(N);
    hipLaunchKernelGGL(records_kernel, dim3(nf), dim3(256), 0, s, V, F, faces, keep, c.sort.k[0], c.sort.v[0], c.parent, counts);
    const SortedEdges edges = sort_half_edges(V, N, faces, c.sort, s);
    hipLaunchKernelGGL(link_kernel, dim3(nh), dim3(256), 0, s, V, N, faces, edges.smin, edges.smax, edges.sval, c.parent, counts);
    hipLaunchKernelGGL(flatten_kernel, dim3(nf), dim3(256), 0, s, V, F, faces, keep, c.parent, corner_fan, (uint32_t *)vertex_fans, counts);
    hipLaunchKernelGGL(vertex_census_kernel, dim3(blocks256((size_t)V)), dim3(256), 0, s, V, (const uint32_t *)vertex_fans, counts);
    return hipGetLastError();
}

hipError_t ts_manifold_split(int V, int F, const int32_t *faces, const uint8_t *keep, const int32_t *corner_fan, int capacity, int32_t *out_faces,
                             int32_t *new_vertex_source, int32_t *new_vertex_fan, unsigned long long *totals, void *ws, hipStream_t s)
{
    hipError_t e = mesh_fill(totals, 0, 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    if (capacity > 0)
    {
        e = mesh_fill(new_vertex_source, 0xFF, (size_t)capacity * sizeof(int32_t), s); // -1 past the number of new vertices
        if (e != hipSuccess) return e;
        e = mesh_fill(new_vertex_fan, 0xFF, (size_t)capacity * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
    }
    const size_t f = (size_t)(F > 0 ? F : 0), N = 3 * f;
    if (N == 0) return hipSuccess;
    if (V <= 0) return mesh_copy(out_faces, faces, N * sizeof(int32_t), s); // nothing takes part
    const size_t v = (size_t)V;
    const SplitCarve c = split_carve(ws, v, f);
    e = mesh_fill(c.keeper, 0xFF, v * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    e = mesh_fill(c.flag, 0, N * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const unsigned nf = blocks256(f), nh = blocks256(N);
    hipLaunchKernelGGL(labels_kernel, dim3(nf), dim3(256), 0, s, V, F, faces, keep, corner_fan, c.lab, c.flag, c.keeper);
    hipLaunchKernelGGL(flag_kernel, dim3(nh), dim3(256), 0, s, N, faces, c.keeper, c.flag);
    scan_columns<1>(N, {{c.flag}}, c.block_sum, c.total, s); // the flags become their indices
    if (capacity > 0)
        hipLaunchKernelGGL(sources_kernel, dim3(nh), dim3(256), 0, s, N, faces, c.flag, c.total, capacity, new_vertex_source, new_vertex_fan);
    hipLaunchKernelGGL(rewrite_kernel, dim3(nh), dim3(256), 0, s, V, N, faces, c.lab, c.keeper, c.flag, out_faces, totals);
    hipLaunchKernelGGL(split_finish_kernel, dim3(1), dim3(256), 0, s, c.total, totals);
    return hipGetLastError();
}
