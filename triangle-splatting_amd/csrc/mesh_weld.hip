// mesh_weld.hip -- vertex welding and edge topology of an indexed triangle mesh (include/ts_weld.h).
//
// Built with -ffp-contract=off: the pair test (dx*dx + dy*dy) + dz*dz <= eps*eps rounds every operation, and so do the two bounds below.
//
// Labels.  The front half is knn.hip's (ts_knn_front.h, FINITE_ONLY): Morton-sorted points gathered as float4 (xyz, original index) and the
// min/max box of every 1024 of them; a point with a NaN or infinite coordinate stays out of every box and is stored as three NaNs, so
// every test against it fails.  One 256-lane workgroup owns a box (4 points per lane).  The relation is symmetric, so the workgroup of box
// a visits the boxes b >= a only, and inside its own box a point meets the candidates that come before it.  A box is visited when its
// box-to-box bound is <= eps*eps; it is staged through LDS (every lane reads the same candidate: LDS broadcast) and a lane skips the points
// whose box-to-point bound is above eps*eps.  Both bounds have the pair test's expression shape -- one difference of two coordinates per
// axis, then the squares, then the same sum order -- and the differences they take are never larger in magnitude than the pair's; rounding
// is monotonic, so a bound is never above the value of a pair it covers: pruning drops no pair that passes, and the result is exact.
// Every passing pair is handed to the union-find below.  The labels are its roots: the smallest index of every cluster.
//
// Union-find (uf_find / uf_union, csrc/ts_union_find.h, shared with mesh_manifold.hip and mesh_orient.hip; also the core of
// ts_weld_face_components): its invariants and its termination argument are stated there.  The flatten (label[i] = root(i)) is a launch
// of its own after all unions.
//
// Compaction.  A vertex is a root iff label[i] == i; an exclusive scan of the root flags ranks the clusters by ascending label (block
// counts, one block scanning them, block-local scan again: csrc/ts_mesh_scan.h; the count and the rank pass, which compute the flag, are
// this unit's).  "first" copies the root's position bits.  "mean" sorts 0..V-1 stably by label (ts_radix_sort_pairs), so a cluster's members are contiguous in ascending index order, and one lane walks one cluster summing in float64
// in that order.  No float atomics.
//
// Edge census.  Every kept face with three indices in [0, V) gives three (min, max) pairs; every other face gives three (V, V) sentinels.
// Two stable 32-bit sorts (by max, then by min) order the 64-bit keys; a run-length pass classifies the head of every run by looking at
// most two elements ahead (edge_run_head, csrc/ts_mesh_common.h), reduces inside the workgroup and adds to the four 64-bit counters with
// integer atomics.  A face with a repeated index takes part here and yields an edge (a, a): the keys are this unit's own, not the
// half-edge records of csrc/ts_mesh_edges.h.
#include "ts_knn_front.h"
#include "ts_mesh_scan.h"
#include "ts_union_find.h"
#include "ts_weld_launch.h"

namespace
{
__global__ void __launch_bounds__(256) uf_init_kernel(int V, uint32_t *__restrict__ parent)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < V) parent[i] = (uint32_t)i;
}

// after all unions: label[i] = root(i), in place (a word that was already flattened still names an ancestor of everything below it)
__global__ void __launch_bounds__(256) uf_flatten_kernel(int V, uint32_t *parent)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const uint32_t r = uf_find(parent, (uint32_t)i, false);
    __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- radius search --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float weld_sum(float dx, float dy, float dz) { return (dx * dx + dy * dy) + dz * dz; }

// one axis of a bound: the gap between [amn, amx] and [bmn, bmx], a single difference of two of the four coordinates, 0 when they overlap
__device__ __forceinline__ float axis_gap(float amn, float amx, float bmn, float bmx)
{
    return amn > bmx ? amn - bmx : (bmn > amx ? bmn - amx : 0.0f);
}

__device__ __forceinline__ float bound_box_box(const Box &a, const Box &b)
{
    return weld_sum(axis_gap(a.mnx, a.mxx, b.mnx, b.mxx), axis_gap(a.mny, a.mxy, b.mny, b.mxy), axis_gap(a.mnz, a.mxz, b.mnz, b.mxz));
}

__device__ __forceinline__ float bound_box_point(const Box &b, float px, float py, float pz)
{
    return weld_sum(axis_gap(px, px, b.mnx, b.mxx), axis_gap(py, py, b.mny, b.mxy), axis_gap(pz, pz, b.mnz, b.mxz));
}

__global__ void __launch_bounds__(TPB) weld_search_kernel(int P, int nboxes, float eps2, const float4 *__restrict__ sp,
                                                           const Box *__restrict__ boxes, uint32_t *parent, unsigned long long *box_visits)
{
    __shared__ float4 cand[BOX];
    const int mybox = blockIdx.x, tid = threadIdx.x;
    const Box bme = boxes[mybox];

    float px[PPT], py[PPT], pz[PPT];
    uint32_t pid[PPT];
    bool have[PPT];
#pragma unroll
    for (int q = 0; q < PPT; q++)
    {
        const int i = mybox * BOX + q * TPB + tid;
        const float nan = __uint_as_float(0x7FC00000u);
        const float4 p = i < P ? sp[i] : make_float4(nan, nan, nan, 0.0f);
        px[q] = p.x; py[q] = p.y; pz[q] = p.z; pid[q] = __float_as_uint(p.w);
        have[q] = i < P && p.x == p.x; // a non-finite point was stored as NaNs: adjacent to nothing
    }
    unsigned visited = 0;
    for (int b = mybox; b < nboxes; b++)
    {
        const Box bb = boxes[b];
        if (b != mybox && !(bound_box_box(bme, bb) <= eps2)) continue; // workgroup-uniform
        visited++;
        const int n = min(BOX, P - b * BOX);
        __syncthreads(); // previous users of `cand` are done
        for (int i = tid; i < n; i += TPB) cand[i] = sp[(size_t)b * BOX + i];
        __syncthreads();
        int limit[PPT], top = 0;
#pragma unroll
        for (int q = 0; q < PPT; q++)
        {
            limit[q] = 0;
            if (have[q] && bound_box_point(bb, px[q], py[q], pz[q]) <= eps2) limit[q] = b == mybox ? min(n, q * TPB + tid) : n;
            top = max(top, limit[q]);
        }
        for (int i = 0; i < top; i++)
        {
            const float4 c = cand[i];
#pragma unroll
            for (int q = 0; q < PPT; q++)
            {
                if (i >= limit[q]) continue;
                if (weld_sum(px[q] - c.x, py[q] - c.y, pz[q] - c.z) <= eps2) uf_union(parent, pid[q], __float_as_uint(c.w));
            }
        }
    }
    if (box_visits && tid == 0) atomicAdd(box_visits, (unsigned long long)visited);
}

// ---- faces ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) face_union_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep,
                                                         uint32_t *parent)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    int32_t v[3];
    if (f >= F || !face_in_range(V, (size_t)f, faces, keep, v)) return;
    uf_union(parent, (uint32_t)v[0], (uint32_t)v[1]);
    uf_union(parent, (uint32_t)v[1], (uint32_t)v[2]);
}

__global__ void __launch_bounds__(256) remap_faces_kernel(int V, int F, const int32_t *__restrict__ faces, const int32_t *__restrict__ remap,
                                                          int32_t *__restrict__ out_faces, uint8_t *__restrict__ keep)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int32_t v[3], w[3] = {-1, -1, -1};
    const bool ok = face_in_range(V, (size_t)f, faces, nullptr, v);
    if (ok) { w[0] = remap[v[0]]; w[1] = remap[v[1]]; w[2] = remap[v[2]]; }
    out_faces[3 * (size_t)f] = w[0]; out_faces[3 * (size_t)f + 1] = w[1]; out_faces[3 * (size_t)f + 2] = w[2];
    keep[f] = ok && w[0] != w[1] && w[1] != w[2] && w[0] != w[2];
}

// ---- compaction ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) root_count_kernel(int V, const uint32_t *__restrict__ label, uint32_t *__restrict__ block_count)
{
    __shared__ uint32_t lds[4];
    uint32_t n = 0;
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++)
        if (base + k < (size_t)V) n += label[base + k] == (uint32_t)(base + k);
    uint32_t total;
    block_scan256(n, lds, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) root_rank_kernel(int V, const uint32_t *__restrict__ label, const uint32_t *__restrict__ block_offset,
                                                        uint32_t *__restrict__ root_rank)
{
    __shared__ uint32_t lds[4];
    uint32_t n = 0;
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
    bool root[SCAN_PER];
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++)
    {
        root[k] = base + k < (size_t)V && label[base + k] == (uint32_t)(base + k);
        n += root[k];
    }
    uint32_t total, run = block_offset[blockIdx.x] + block_scan256(n, lds, &total);
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++)
        if (root[k]) root_rank[base + k] = run++;
}

// remap[i] = rank of label[i]; "first": the root's position bits go to its rank's row
__global__ void __launch_bounds__(256) remap_kernel(int V, const uint32_t *__restrict__ label, const uint32_t *__restrict__ root_rank,
                                                    const uint32_t *__restrict__ vertices, int copy_first, int32_t *__restrict__ remap,
                                                    uint32_t *__restrict__ out_vertices)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const uint32_t l = label[i];
    const uint32_t r = l < (uint32_t)V ? root_rank[l] : 0u; // a label is always < V; the test only keeps a foreign array in bounds
    remap[i] = (int32_t)r;
    if (copy_first && l == (uint32_t)i)
    {
        out_vertices[3 * (size_t)r] = vertices[3 * (size_t)i];
        out_vertices[3 * (size_t)r + 1] = vertices[3 * (size_t)i + 1];
        out_vertices[3 * (size_t)r + 2] = vertices[3 * (size_t)i + 2];
    }
}

__global__ void __launch_bounds__(256) label_keys_kernel(int V, const uint32_t *__restrict__ label, uint32_t *__restrict__ keys,
                                                         uint32_t *__restrict__ ids)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const uint32_t l = label[i];
    keys[i] = l < (uint32_t)V ? l : 0u;
    ids[i] = (uint32_t)i;
}

// one lane walks one cluster of the label-sorted order: float64 sum of the members in ascending index order, starting from the first
__global__ void __launch_bounds__(256) mean_kernel(int V, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ ids,
                                                   const uint32_t *__restrict__ root_rank, const float *__restrict__ vertices,
                                                   float *__restrict__ out_vertices)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= V) return;
    const uint32_t l = keys[j];
    if (j > 0 && keys[j - 1] == l) return; // not the head of its run
    const uint32_t first = ids[j];
    double sx = (double)vertices[3 * (size_t)first], sy = (double)vertices[3 * (size_t)first + 1], sz = (double)vertices[3 * (size_t)first + 2];
    int m = j + 1; // bounded by V
    for (; m < V && keys[m] == l; m++)
    {
        const uint32_t id = ids[m];
        sx += (double)vertices[3 * (size_t)id]; sy += (double)vertices[3 * (size_t)id + 1]; sz += (double)vertices[3 * (size_t)id + 2];
    }
    const double n = (double)(m - j);
    const uint32_t r = root_rank[l];
    out_vertices[3 * (size_t)r] = (float)(sx / n);
    out_vertices[3 * (size_t)r + 1] = (float)(sy / n);
    out_vertices[3 * (size_t)r + 2] = (float)(sz / n);
}

// ---- edge census -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) edge_keys_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep,
                                                        uint32_t *__restrict__ hi, uint32_t *__restrict__ lo)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int32_t v[3];
    const bool ok = face_in_range(V, (size_t)f, faces, keep, v);
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const uint32_t a = (uint32_t)v[k], b = (uint32_t)v[(k + 1) % 3];
        hi[3 * (size_t)f + k] = ok ? max(a, b) : (uint32_t)V;
        lo[3 * (size_t)f + k] = ok ? min(a, b) : (uint32_t)V;
    }
}

__global__ void __launch_bounds__(256) edge_runs_kernel(int V, size_t E, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi,
                                                        unsigned long long *counts)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t run = (uint32_t)edge_run_head(V, E, j, lo, hi);
    uint32_t c[4] = {run > 0, run == 1, run == 2, run == 3}; // edges, boundary, manifold, nonmanifold
    count4_into(counts, c);
}

struct SortCarve
{
    uint32_t *a[2], *b[2]; // two ping-pong pairs of n words each
    void *scratch;
};

SortCarve sort_carve(Carver &w, size_t n)
{
    SortCarve c;
    c.a[0] = w.words(n); c.a[1] = w.words(n); c.b[0] = w.words(n); c.b[1] = w.words(n);
    c.scratch = w.bytes(ts_radix_scratch_bytes(n)); // without the floor of sort_scratch_bytes: this unit's sizes stay as they were
    return c;
}

struct CompactCarve
{
    uint32_t *root_rank, *block_count;
    SortCarve sort;
    int nb;
    size_t bytes;
};

CompactCarve compact_carve(void *ws, int V)
{
    CompactCarve c;
    Carver w(ws);
    const size_t n = (size_t)(V > 0 ? V : 0);
    c.nb = (int)scan_blocks(n);
    c.root_rank = w.words(n);
    c.block_count = w.words((size_t)c.nb);
    c.sort = sort_carve(w, n);
    c.bytes = w.used();
    return c;
}

size_t census_bytes(size_t E)
{
    Carver w(nullptr);
    sort_carve(w, E);
    return w.used();
}
} // namespace

size_t ts_weld_workspace_bytes(int V, int F)
{
    const size_t labels = knn_carve(nullptr, V).bytes;
    const size_t compact = compact_carve(nullptr, V).bytes;
    const size_t census = census_bytes(3 * (size_t)(F > 0 ? F : 0));
    return std::max(labels, std::max(compact, census)) + 2 * TS_ALIGN;
}

hipError_t ts_weld_labels(int V, const float *vertices, float eps, uint32_t *label, unsigned long long *box_visits, void *ws, hipStream_t s)
{
    if (V <= 0) return hipSuccess;
    const KnnCarve c = knn_carve(ws, V);
    hipLaunchKernelGGL(uf_init_kernel, dim3(blocks256((size_t)V)), dim3(256), 0, s, V, label);
    hipError_t e = knn_prepare<true>(V, vertices, c, s);
    if (e != hipSuccess) return e;
    const float eps2 = eps * eps;
    hipLaunchKernelGGL(weld_search_kernel, dim3(c.nboxes), dim3(TPB), 0, s, V, c.nboxes, eps2, c.sp, c.boxes, label, box_visits);
    hipLaunchKernelGGL(uf_flatten_kernel, dim3(blocks256((size_t)V)), dim3(256), 0, s, V, label);
    return hipGetLastError();
}

hipError_t ts_weld_face_components(int V, int F, const int32_t *faces, const uint8_t *keep, uint32_t *label, hipStream_t s)
{
    if (V <= 0) return hipSuccess;
    hipLaunchKernelGGL(uf_init_kernel, dim3(blocks256((size_t)V)), dim3(256), 0, s, V, label);
    if (F > 0) hipLaunchKernelGGL(face_union_kernel, dim3(blocks256((size_t)F)), dim3(256), 0, s, V, F, faces, keep, label);
    hipLaunchKernelGGL(uf_flatten_kernel, dim3(blocks256((size_t)V)), dim3(256), 0, s, V, label);
    return hipGetLastError();
}

hipError_t ts_weld_compact(int V, const uint32_t *label, const float *vertices, int mode, int32_t *remap, float *out_vertices, int32_t *count,
                           void *ws, hipStream_t s)
{
    if (V <= 0) return hipSuccess;
    const CompactCarve c = compact_carve(ws, V);
    const unsigned nv = blocks256((size_t)V);
    hipError_t e = mesh_fill(out_vertices, 0, (size_t)V * 3 * sizeof(float), s); // rows V' .. V - 1 stay zero
    if (e != hipSuccess) return e;
    e = mesh_fill(c.root_rank, 0, (size_t)V * sizeof(uint32_t), s); // a foreign label that names a non-root then ranks 0: always a row of out_vertices
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(root_count_kernel, dim3(c.nb), dim3(256), 0, s, V, label, c.block_count);
    hipLaunchKernelGGL(scan_offsets_kernel<1>, dim3(1), dim3(256), 0, s, c.nb, c.block_count, (uint32_t *)count);
    hipLaunchKernelGGL(root_rank_kernel, dim3(c.nb), dim3(256), 0, s, V, label, c.block_count, c.root_rank);
    hipLaunchKernelGGL(remap_kernel, dim3(nv), dim3(256), 0, s, V, label, c.root_rank, (const uint32_t *)vertices, mode == 0 ? 1 : 0, remap,
                       (uint32_t *)out_vertices);
    if (mode != 0)
    {
        hipLaunchKernelGGL(label_keys_kernel, dim3(nv), dim3(256), 0, s, V, label, c.sort.a[0], c.sort.b[0]);
        const int at = ts_radix_sort_pairs(c.sort.a, c.sort.b, (size_t)V, bit_length((uint32_t)(V - 1)), c.sort.scratch, s);
        hipLaunchKernelGGL(mean_kernel, dim3(nv), dim3(256), 0, s, V, c.sort.a[at], c.sort.b[at], c.root_rank, vertices, out_vertices);
    }
    return hipGetLastError();
}

hipError_t ts_weld_remap_faces(int V, int F, const int32_t *faces, const int32_t *remap, int32_t *out_faces, uint8_t *keep, hipStream_t s)
{
    if (F <= 0) return hipSuccess;
    hipLaunchKernelGGL(remap_faces_kernel, dim3(blocks256((size_t)F)), dim3(256), 0, s, V, F, faces, remap, out_faces, keep);
    return hipGetLastError();
}

hipError_t ts_weld_edge_census(int V, int F, const int32_t *faces, const uint8_t *keep, unsigned long long *counts, void *ws, hipStream_t s)
{
    if (F <= 0) return hipSuccess;
    const size_t E = 3 * (size_t)F;
    Carver w(ws);
    const SortCarve c = sort_carve(w, E);
    hipError_t e = mesh_fill(counts, 0, 4 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(edge_keys_kernel, dim3(blocks256((size_t)F)), dim3(256), 0, s, V, F, faces, keep, c.a[0], c.b[0]);
    const int bits = bit_length((uint32_t)(V > 0 ? V : 0)); // the sentinel V included
    const int at = ts_radix_sort_pairs(c.a, c.b, E, bits, c.scratch, s); // by max (a = max, b = min), stable
    uint32_t *const k2[2] = {c.b[at], c.b[at ^ 1]}, *const v2[2] = {c.a[at], c.a[at ^ 1]};
    const int at2 = ts_radix_sort_pairs(k2, v2, E, bits, c.scratch, s); // then by min, stable: (min, max) order
    hipLaunchKernelGGL(edge_runs_kernel, dim3(blocks256(E)), dim3(256), 0, s, V, E, k2[at2], v2[at2], counts);
    return hipGetLastError();
}
