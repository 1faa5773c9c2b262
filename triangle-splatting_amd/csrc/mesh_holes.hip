// mesh_holes.hip -- the boundary loops of an indexed mesh, found, ordered and numbered, and the centroid fans that close them
// (include/ts_holes.h).
//
// Built with -ffp-contract=off: every float64 operation of the header's text rounds, which is what makes the fill bit-equal to
// tests/ref_mesh_holes.py.  No floating-point atomics anywhere; the atomics are integer adds and minima (the vertex census, the counters).
//
// Loops.  One thread per face looks its three half-edges up in the adjacency table (a lower-bound search in the tail's row, cut at
// num_entries) and, for a boundary one, adds to the tail's and the head's counters and lowers the tail's smallest outgoing half-edge.  One
// thread per half-edge then reads its successor off its head.  The cycles are found by pointer doubling: every half-edge holds (jump, the
// smallest label seen, an open flag) and takes over its jump target's in every round, ping-pong between two buffers, every read from the
// previous round; after ceil(log2(n)) rounds, n a bound on the longest chain, a half-edge on a cycle holds the cycle's smallest half-edge and
// one on a path holds the open flag.  The bound is min(3 F, V + 1): the tails along a chain are distinct vertices.  A second doubling pass
// (Wyllie) counts the hops to the half-edge in front of the head, the cycle cut there, which gives the rank and, at the head, the length.
// Heads and lengths are ranked by the block-sum prefix sum of two columns (scan_columns<2>, csrc/ts_mesh_scan.h).  One scatter
// writes the CSR.
//
// Fill.  One thread per loop decides its status (the length, the lone face, the finiteness of its vertices), a prefix sum of the same form
// numbers the new vertices and faces, one thread per loop sums its members' coordinates and attributes in member order, one thread per member
// finds its loop by a search in loop_offsets and writes its face.
#include "ts_holes_launch.h"
#include "ts_mesh_scan.h"

namespace
{
constexpr uint32_t OPEN = 0x80000000u, LABEL = 0x7FFFFFFFu; // the second word of a label state: the smallest label and the open flag
constexpr int32_t NOT_BOUNDARY = -2, NO_SUCCESSOR = -1;     // succ[h] otherwise: the successor
constexpr uint8_t FILLED = 0, TOO_LONG = 1, LONE_FACE = 2, DEAD = 3; // TSH_FILLED .. TSH_DEAD

int doubling_rounds(size_t n) // ceil(log2(max(n, 2)))
{
    int r = 1;
    while (r < 31 && ((size_t)1 << r) < n) r++;
    return r;
}

// ---- loops -------------------------------------------------------------------------------------------------------------------------------
// One thread = one face.  Every load of the table is at an index in [0, num_entries); the census is indexed by indices checked against V.
__global__ void __launch_bounds__(256) classify_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep,
                                                        const int32_t *__restrict__ offsets, const int32_t *__restrict__ neighbors,
                                                        const int32_t *__restrict__ edge_faces, int num_entries, int32_t *__restrict__ succ,
                                                        uint32_t *out_count, uint32_t *in_count, uint32_t *out_min, unsigned long long *counts)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    uint32_t nb = 0;
    if (f < F)
    {
        int32_t v[3];
        const bool ok = face_takes_part(V, (size_t)f, faces, keep, v);
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
            const int32_t a = v[k], b = v[(k + 1) % 3];
            const size_t h = 3 * (size_t)f + k;
            bool boundary = false;
            if (ok)
            {
                const int e1 = min(offsets[a + 1], num_entries);
                int lo = max(offsets[a], 0), hi = e1;
                while (lo < hi)
                {
                    const int m = lo + ((hi - lo) >> 1);
                    if (neighbors[m] < b) lo = m + 1;
                    else hi = m;
                }
                boundary = lo < e1 && neighbors[lo] == b && edge_faces[lo] == 1;
            }
            succ[h] = boundary ? NO_SUCCESSOR : NOT_BOUNDARY;
            if (boundary)
            {
                atomicAdd(out_count + a, 1u);
                atomicAdd(in_count + b, 1u);
                atomicMin(out_min + a, (uint32_t)h);
                nb++;
            }
        }
    }
    count_into(counts + 0, nb);
}

__global__ void __launch_bounds__(256) vertex_census_kernel(int V, const uint32_t *__restrict__ out_count, const uint32_t *__restrict__ in_count,
                                                             unsigned long long *counts)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    uint32_t n = 0;
    if (v < V)
    {
        const uint32_t o = out_count[v], i = in_count[v];
        n = (o | i) != 0 && !(o == 1 && i == 1);
    }
    count_into(counts + 3, n);
}

// One thread = one half-edge: its successor, and its state before the first doubling round.  The head of a boundary half-edge was checked
// against V by classify_kernel; out_min of a simple vertex is the half-edge that set out_count to 1, below N.
__global__ void __launch_bounds__(256) successor_kernel(size_t N, const int32_t *__restrict__ faces, int32_t *__restrict__ succ,
                                                         const uint32_t *__restrict__ out_count, const uint32_t *__restrict__ in_count,
                                                         const uint32_t *__restrict__ out_min, uint2 *__restrict__ state)
{
    const size_t h = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= N) return;
    int32_t nx = NO_SUCCESSOR;
    if (succ[h] != NOT_BOUNDARY)
    {
        const size_t f = h / 3, k = h - 3 * f;
        const int32_t b = faces[3 * f + (k + 1) % 3];
        if (out_count[b] == 1 && in_count[b] == 1)
        {
            const uint32_t o = out_min[b];
            if (o < N) nx = (int32_t)o;
        }
        succ[h] = nx;
    }
    state[h] = make_uint2((uint32_t)nx, (uint32_t)h | (nx < 0 ? OPEN : 0u));
}

__global__ void __launch_bounds__(256) label_round_kernel(size_t N, const uint2 *__restrict__ in, uint2 *__restrict__ out)
{
    const size_t h = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= N) return;
    uint2 s = in[h];
    if (s.x < N) // a jump; 0xFFFFFFFF is none
    {
        const uint2 t = in[s.x];
        s = make_uint2(t.x, min(s.y & LABEL, t.y & LABEL) | ((s.y | t.y) & OPEN));
    }
    out[h] = s;
}

// lab[h] = the head of h's loop, or -1; the Wyllie state (jump, hops to the last member) with the cycle cut in front of its head
__global__ void __launch_bounds__(256) rank_init_kernel(size_t N, const int32_t *__restrict__ succ, const uint2 *__restrict__ label,
                                                         int32_t *__restrict__ lab, uint2 *__restrict__ state)
{
    const size_t h = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= N) return;
    const int32_t nx = succ[h];
    const uint32_t l = label[h].y;
    const bool on_loop = nx >= 0 && !(l & OPEN) && l < N;
    lab[h] = on_loop ? (int32_t)l : -1;
    const bool last = !on_loop || (uint32_t)nx == l;
    state[h] = last ? make_uint2(0xFFFFFFFFu, 0u) : make_uint2((uint32_t)nx, 1u);
}

__global__ void __launch_bounds__(256) rank_round_kernel(size_t N, const uint2 *__restrict__ in, uint2 *__restrict__ out)
{
    const size_t h = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= N) return;
    uint2 s = in[h];
    if (s.x < N)
    {
        const uint2 t = in[s.x];
        s = make_uint2(t.x, s.y + t.y);
    }
    out[h] = s;
}

__global__ void __launch_bounds__(256) head_values_kernel(size_t N, const int32_t *__restrict__ lab, const uint2 *__restrict__ rank,
                                                           uint32_t *__restrict__ head_flag, uint32_t *__restrict__ head_len)
{
    const size_t h = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= N) return;
    const bool head = lab[h] >= 0 && (size_t)lab[h] == h;
    head_flag[h] = head ? 1u : 0u;
    head_len[h] = head ? rank[h].y + 1u : 0u;
}

// head_index / head_start: the two prefix sums.  A member's slot is its loop's start + its rank, below the member total <= N.
__global__ void __launch_bounds__(256) scatter_kernel(size_t N, int F, const int32_t *__restrict__ lab, const uint2 *__restrict__ rank,
                                                       const uint32_t *__restrict__ head_index, const uint32_t *__restrict__ head_start,
                                                       int32_t *__restrict__ half_edge_loop, int32_t *__restrict__ loop_offsets,
                                                       int32_t *__restrict__ loop_half_edges)
{
    const size_t h = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= N) return;
    const int32_t l = lab[h];
    if (l < 0) { half_edge_loop[h] = -1; return; }
    const uint32_t index = head_index[l], start = head_start[l];
    const size_t slot = (size_t)start + (rank[l].y - rank[h].y);
    half_edge_loop[h] = (int32_t)index;
    if (slot < N) loop_half_edges[slot] = (int32_t)h;
    if ((size_t)l == h && index <= (uint32_t)F) loop_offsets[index] = (int32_t)start;
}

// total = {loops, members}: the entries of loop_offsets from `loops` on, and the two counters
__global__ void __launch_bounds__(256) loops_finish_kernel(int F, const uint32_t *__restrict__ total, int32_t *__restrict__ loop_offsets,
                                                            unsigned long long *__restrict__ counts)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i > (size_t)F) return;
    const uint32_t loops = total[0], members = total[1];
    if (i >= loops) loop_offsets[i] = (int32_t)members;
    if (i == 0) { counts[1] = members; counts[2] = loops; }
}

// ---- fill --------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void loop_range(const int32_t *__restrict__ loop_offsets, int i, int num_members, int *start, int *end)
{
    const int a = min(max(loop_offsets[i], 0), num_members);
    *start = a;
    *end = min(max(loop_offsets[i + 1], a), num_members);
}

// the tail of member slot p, or -1 when the member or its tail is out of range
__device__ __forceinline__ int32_t member_tail(int V, int F, const int32_t *__restrict__ faces, const int32_t *__restrict__ loop_half_edges, int p)
{
    const int32_t h = loop_half_edges[p];
    if (h < 0 || (size_t)h >= 3 * (size_t)F) return -1;
    const int32_t a = faces[h];
    return (uint32_t)a < (uint32_t)V ? a : -1;
}

__global__ void __launch_bounds__(256) fill_status_kernel(int V, int F, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                           int num_loops, const int32_t *__restrict__ loop_offsets,
                                                           const int32_t *__restrict__ loop_half_edges, int num_members, int max_loop_edges,
                                                           uint8_t *__restrict__ loop_status, uint32_t *__restrict__ vertex_flag,
                                                           uint32_t *__restrict__ face_count, unsigned long long *totals)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    uint32_t filled = 0;
    if (i < num_loops)
    {
        int start, end;
        loop_range(loop_offsets, i, num_members, &start, &end);
        const int L = end - start;
        uint8_t status = FILLED;
        if (L > max_loop_edges) status = TOO_LONG;
        else
        {
            if (L == 3)
            {
                const int32_t h0 = loop_half_edges[start], h1 = loop_half_edges[start + 1], h2 = loop_half_edges[start + 2];
                const bool in_range = h0 >= 0 && h1 >= 0 && h2 >= 0 && (size_t)h0 < 3 * (size_t)F && (size_t)h1 < 3 * (size_t)F &&
                                      (size_t)h2 < 3 * (size_t)F;
                if (in_range && h0 / 3 == h1 / 3 && h1 / 3 == h2 / 3) status = LONE_FACE;
            }
            if (status == FILLED)
            {
                bool dead = L < 3;
                for (int p = start; p < end && !dead; p++)
                {
                    const int32_t a = member_tail(V, F, faces, loop_half_edges, p);
                    dead = a < 0 || !finite32(vertices[3 * (size_t)a]) || !finite32(vertices[3 * (size_t)a + 1]) ||
                           !finite32(vertices[3 * (size_t)a + 2]);
                }
                if (dead) status = DEAD;
            }
        }
        loop_status[i] = status;
        filled = status == FILLED;
        vertex_flag[i] = filled && L != 3;
        face_count[i] = filled ? (L == 3 ? 1u : (uint32_t)L) : 0u;
    }
    count_into(totals + 0, filled);
}

// One thread = one filled loop longer than 3: the sequential sums of the header, in member order.  vertex_index < the number of such loops
// <= num_loops, the extent of the three outputs.
__global__ void __launch_bounds__(256) fill_vertices_kernel(int V, int F, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                             int num_loops, const int32_t *__restrict__ loop_offsets,
                                                             const int32_t *__restrict__ loop_half_edges, int num_members,
                                                             const float *__restrict__ attributes, const uint8_t *__restrict__ attr_valid,
                                                             int channels, const uint8_t *__restrict__ loop_status,
                                                             const uint32_t *__restrict__ vertex_index, float *__restrict__ new_vertices,
                                                             float *__restrict__ new_attributes, uint8_t *__restrict__ new_attr_valid)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= num_loops || loop_status[i] != FILLED) return;
    int start, end;
    loop_range(loop_offsets, i, num_members, &start, &end);
    const int L = end - start;
    const uint32_t j = vertex_index[i];
    if (L == 3 || j >= (uint32_t)num_loops) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    uint32_t n = 0;
    for (int p = start; p < end; p++)
    {
        const int32_t a = member_tail(V, F, faces, loop_half_edges, p); // in range: the loop is not DEAD
        sx += (double)vertices[3 * (size_t)a]; sy += (double)vertices[3 * (size_t)a + 1]; sz += (double)vertices[3 * (size_t)a + 2];
        n += !attr_valid || attr_valid[a];
    }
    const double len = (double)L;
    new_vertices[3 * (size_t)j] = (float)(sx / len); new_vertices[3 * (size_t)j + 1] = (float)(sy / len); new_vertices[3 * (size_t)j + 2] = (float)(sz / len);
    if (channels <= 0) return;
    new_attr_valid[j] = n ? 1 : 0;
    for (int c = 0; c < channels; c++)
    {
        double s = 0.0;
        for (int p = start; p < end; p++)
        {
            const int32_t a = member_tail(V, F, faces, loop_half_edges, p);
            if (!attr_valid || attr_valid[a]) s += (double)attributes[(size_t)a * channels + c];
        }
        new_attributes[(size_t)j * channels + c] = n ? (float)(s / (double)n) : 0.0f;
    }
}

// One thread = one member slot.  Its loop is the first whose end lies behind the slot; a face's row is its loop's first row + the member's
// position, checked against num_members, the extent of both outputs.
__global__ void __launch_bounds__(256) fill_faces_kernel(int V, int F, const int32_t *__restrict__ faces, int num_loops,
                                                          const int32_t *__restrict__ loop_offsets, const int32_t *__restrict__ loop_half_edges,
                                                          int num_members, const uint8_t *__restrict__ loop_status,
                                                          const uint32_t *__restrict__ vertex_index, const uint32_t *__restrict__ face_start,
                                                          int32_t *__restrict__ new_faces, int32_t *__restrict__ new_face_loop)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= num_members) return;
    int lo = 0, hi = num_loops;
    while (lo < hi)
    {
        const int m = lo + ((hi - lo) >> 1);
        if (loop_offsets[m + 1] <= p) lo = m + 1;
        else hi = m;
    }
    if (lo >= num_loops || loop_status[lo] != FILLED) return;
    int start, end;
    loop_range(loop_offsets, lo, num_members, &start, &end);
    if (p < start || p >= end) return;
    const int L = end - start, at = p - start;
    if (L == 3 && at != 0) return;
    const size_t row = (size_t)face_start[lo] + (L == 3 ? 0 : at);
    if (row >= (size_t)num_members) return;
    int32_t x, y, z;
    if (L == 3)
    {
        x = member_tail(V, F, faces, loop_half_edges, start);
        y = member_tail(V, F, faces, loop_half_edges, start + 2);
        z = member_tail(V, F, faces, loop_half_edges, start + 1);
    }
    else
    {
        x = member_tail(V, F, faces, loop_half_edges, at + 1 == L ? start : p + 1);
        y = member_tail(V, F, faces, loop_half_edges, p);
        z = (int32_t)((uint32_t)V + vertex_index[lo]);
    }
    new_faces[3 * row] = x; new_faces[3 * row + 1] = y; new_faces[3 * row + 2] = z;
    new_face_loop[row] = lo;
}

__global__ void __launch_bounds__(256) fill_finish_kernel(const uint32_t *__restrict__ total, unsigned long long *__restrict__ totals)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) { totals[1] = total[0]; totals[2] = total[1]; }
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------
struct LoopsCarve
{
    uint32_t *census; // out_count, in_count, out_min: 3 x V words
    int32_t *succ, *lab;
    uint2 *state[2];
    uint32_t *head_flag, *head_len, *block_sum, *total;
    size_t bytes;
};
LoopsCarve loops_carve(void *ws, size_t V, size_t F)
{
    LoopsCarve c;
    Carver w(ws);
    const size_t N = 3 * F;
    c.census = w.words(3 * V);
    c.succ = (int32_t *)w.words(N); c.lab = (int32_t *)w.words(N);
    c.state[0] = (uint2 *)w.words(2 * N); c.state[1] = (uint2 *)w.words(2 * N);
    c.head_flag = w.words(N); c.head_len = w.words(N);
    c.block_sum = w.words(2 * scan_blocks(N));
    c.total = w.words(2);
    c.bytes = w.used();
    return c;
}

struct FillCarve
{
    uint32_t *vertex_flag, *face_count, *block_sum, *total;
    size_t bytes;
};
FillCarve fill_carve(void *ws, size_t loops)
{
    FillCarve c;
    Carver w(ws);
    c.vertex_flag = w.words(loops); c.face_count = w.words(loops);
    c.block_sum = w.words(2 * scan_blocks(loops));
    c.total = w.words(2);
    c.bytes = w.used();
    return c;
}
} // namespace

size_t ts_holes_workspace_bytes(int V, int F)
{
    const size_t v = (size_t)(V > 0 ? V : 0), f = (size_t)(F > 0 ? F : 0);
    return std::max(loops_carve(nullptr, v, f).bytes, fill_carve(nullptr, f).bytes) + 2 * TS_ALIGN;
}

hipError_t ts_holes_loops(int V, int F, const int32_t *faces, const uint8_t *keep, const int32_t *offsets, const int32_t *neighbors,
                          const int32_t *edge_faces, int num_entries, int32_t *half_edge_loop, int32_t *loop_offsets, int32_t *loop_half_edges,
                          unsigned long long *counts, void *ws, hipStream_t s)
{
    hipError_t e = mesh_fill(counts, 0, 4 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const size_t f = (size_t)(F > 0 ? F : 0), N = 3 * f;
    e = mesh_fill(loop_offsets, 0, (f + 1) * sizeof(int32_t), s);
    if (e != hipSuccess || N == 0) return e;
    e = mesh_fill(loop_half_edges, 0xFF, N * sizeof(int32_t), s); // -1 past the member total
    if (e != hipSuccess) return e;
    if (V <= 0) return mesh_fill(half_edge_loop, 0xFF, N * sizeof(int32_t), s); // nothing takes part
    const size_t v = (size_t)V;
    const LoopsCarve c = loops_carve(ws, v, f);
    uint32_t *out_count = c.census, *in_count = c.census + v, *out_min = c.census + 2 * v;
    e = mesh_fill(out_count, 0, 2 * v * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    e = mesh_fill(out_min, 0xFF, v * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const unsigned nf = blocks256(f), nh = blocks256(N);
    hipLaunchKernelGGL(classify_kernel, dim3(nf), dim3(256), 0, s, V, F, faces, keep, offsets, neighbors, edge_faces, num_entries, c.succ, out_count,
                       in_count, out_min, counts);
    hipLaunchKernelGGL(vertex_census_kernel, dim3(blocks256(v)), dim3(256), 0, s, V, out_count, in_count, counts);
    hipLaunchKernelGGL(successor_kernel, dim3(nh), dim3(256), 0, s, N, faces, c.succ, out_count, in_count, out_min, c.state[0]);
    const int rounds = doubling_rounds(std::min(N, v + 1)); // the tails along a chain are distinct vertices
    int at = 0;
    for (int r = 0; r < rounds; r++, at ^= 1) hipLaunchKernelGGL(label_round_kernel, dim3(nh), dim3(256), 0, s, N, c.state[at], c.state[at ^ 1]);
    hipLaunchKernelGGL(rank_init_kernel, dim3(nh), dim3(256), 0, s, N, c.succ, c.state[at], c.lab, c.state[at ^ 1]);
    at ^= 1;
    for (int r = 0; r < rounds; r++, at ^= 1) hipLaunchKernelGGL(rank_round_kernel, dim3(nh), dim3(256), 0, s, N, c.state[at], c.state[at ^ 1]);
    const uint2 *rank = c.state[at];
    hipLaunchKernelGGL(head_values_kernel, dim3(nh), dim3(256), 0, s, N, c.lab, rank, c.head_flag, c.head_len);
    scan_columns<2>(N, {{c.head_flag, c.head_len}}, c.block_sum, c.total, s); // head_index, head_start
    hipLaunchKernelGGL(scatter_kernel, dim3(nh), dim3(256), 0, s, N, F, c.lab, rank, c.head_flag, c.head_len, half_edge_loop, loop_offsets,
                       loop_half_edges);
    hipLaunchKernelGGL(loops_finish_kernel, dim3(blocks256(f + 1)), dim3(256), 0, s, F, c.total, loop_offsets, counts);
    return hipGetLastError();
}

hipError_t ts_holes_fill(int V, int F, const float *vertices, const int32_t *faces, int num_loops, const int32_t *loop_offsets,
                         const int32_t *loop_half_edges, int num_members, int max_loop_edges, const float *attributes, const uint8_t *attr_valid,
                         int channels, uint8_t *loop_status, float *new_vertices, float *new_attributes, uint8_t *new_attr_valid,
                         int32_t *new_faces, int32_t *new_face_loop, unsigned long long *totals, void *ws, hipStream_t s)
{
    hipError_t e = mesh_fill(totals, 0, 3 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const size_t loops = (size_t)(num_loops > 0 ? num_loops : 0), members = (size_t)(num_members > 0 ? num_members : 0);
    if (members)
    {
        e = mesh_fill(new_faces, 0xFF, 3 * members * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
        e = mesh_fill(new_face_loop, 0xFF, members * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
    }
    if (loops == 0) return hipSuccess;
    e = mesh_fill(new_vertices, 0, 3 * loops * sizeof(float), s);
    if (e != hipSuccess) return e;
    if (channels > 0)
    {
        e = mesh_fill(new_attributes, 0, loops * (size_t)channels * sizeof(float), s);
        if (e != hipSuccess) return e;
        e = mesh_fill(new_attr_valid, 0, loops, s);
        if (e != hipSuccess) return e;
    }
    const FillCarve c = fill_carve(ws, loops);
    const unsigned nl = blocks256(loops);
    hipLaunchKernelGGL(fill_status_kernel, dim3(nl), dim3(256), 0, s, V, F, vertices, faces, num_loops, loop_offsets, loop_half_edges, num_members,
                       max_loop_edges, loop_status, c.vertex_flag, c.face_count, totals);
    scan_columns<2>(loops, {{c.vertex_flag, c.face_count}}, c.block_sum, c.total, s); // vertex_index, face_start
    hipLaunchKernelGGL(fill_vertices_kernel, dim3(nl), dim3(256), 0, s, V, F, vertices, faces, num_loops, loop_offsets, loop_half_edges,
                       num_members, attributes, attr_valid, channels, loop_status, c.vertex_flag, new_vertices, new_attributes, new_attr_valid);
    if (members)
        hipLaunchKernelGGL(fill_faces_kernel, dim3(blocks256(members)), dim3(256), 0, s, V, F, faces, num_loops, loop_offsets, loop_half_edges,
                           num_members, loop_status, c.vertex_flag, c.face_count, new_faces, new_face_loop);
    hipLaunchKernelGGL(fill_finish_kernel, dim3(1), dim3(256), 0, s, c.total, totals);
    return hipGetLastError();
}
