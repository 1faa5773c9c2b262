// mesh_smooth.hip -- the one-ring of every vertex as CSR, Taubin smoothing over it, and face / vertex normals (include/ts_smooth.h).
//
// Built with -ffp-contract=off: every float64 operation of the header's text rounds, which is what makes the result bit-equal to
// tests/ref_mesh_smooth.py.  No floating-point atomics anywhere; the only atomics are integer adds to the four counters of the adjacency.
//
// Adjacency.  One thread per face writes its six directed records (src, dst) into its six slots (the sentinel V in both words of a face that
// does not take part).  Two stable LSD sorts with the product's radix passes -- by dst, then by src, only the bits V needs -- leave the records
// in (src, dst) order.  A record is a HEAD iff it differs from its predecessor; the heads are ranked by the block-sum prefix sum of
// csrc/ts_mesh_scan.h: per-block head counts, its one workgroup turns them into offsets, then every block ranks its own heads behind the
// sum in front of it (nobody waits for anybody); the flags are computed on the fly, so the count and the rank pass are this unit's own.
// A head writes its dst, the length of its run (found by an upper-bound search among the sorted records: at most 31 halvings, no walk) and
// its src into row `rank` of neighbors / edge_faces / a compact src column; the row of vertex v starts at the lower bound of v in that
// column, and one thread per vertex classifies its row.
//
// Smoothing.  The state is two V x 3 float64 buffers in the workspace; a byte per vertex holds its stencil (none / whole row / boundary entries
// only) and whether it is live, decided once.  One launch per step: a thread gathers the previous state of its live neighbours in row order,
// so every sum is sequential by definition and the two buffers ping-pong.  The last kernel clamps against the widened input and rounds once.
//
// Normals.  One thread per face for the face normals.  For the vertex normals one thread per face writes up to three incidence records
// (vertex, face) (the sentinel V in a slot it does not use); a stable sort by vertex leaves each vertex's faces ascending, the head and the
// tail of each run write the run's bounds (csrc/ts_mesh_runs.h), and ONE thread per vertex walks its run, recomputing each face's cross
// product.
#include "ts_mesh_runs.h"
#include "ts_mesh_scan.h"
#include "ts_smooth_launch.h"

namespace
{
constexpr uint8_t ST_NONE = 0, ST_ROW = 1, ST_CURVE = 2, ST_MASK = 3, LIVE = 4; // the per-vertex byte of the smoothing

// ---- adjacency -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) records_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep,
                                                       uint32_t *__restrict__ dst, uint32_t *__restrict__ src)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int32_t v[3];
    const bool ok = face_takes_part(V, (size_t)f, faces, keep, v);
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const uint32_t a = ok ? (uint32_t)v[k] : (uint32_t)V, b = ok ? (uint32_t)v[(k + 1) % 3] : (uint32_t)V;
        const size_t slot = 6 * (size_t)f + 2 * k;
        src[slot] = a; dst[slot] = b;         // (a, b)
        src[slot + 1] = b; dst[slot + 1] = a; // (b, a)
    }
}

__device__ __forceinline__ bool is_head(int V, size_t j, size_t N, const uint32_t *__restrict__ ssrc, const uint32_t *__restrict__ sdst)
{
    if (j >= N) return false;
    const uint32_t a = ssrc[j];
    if (a >= (uint32_t)V) return false; // the sentinel records sort behind every real one
    return j == 0 || ssrc[j - 1] != a || sdst[j - 1] != sdst[j];
}

__global__ void __launch_bounds__(256) head_count_kernel(int V, size_t N, const uint32_t *__restrict__ ssrc, const uint32_t *__restrict__ sdst,
                                                          uint32_t *__restrict__ block_count)
{
    __shared__ uint32_t lds[4];
    uint32_t n = 0;
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++) n += is_head(V, base + k, N, ssrc, sdst);
    uint32_t total;
    block_scan256(n, lds, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// Every head writes row `rank` of the three compact columns.  rank < the number of heads <= N, the extent of all three.
__global__ void __launch_bounds__(256) scatter_rows_kernel(int V, size_t N, const uint32_t *__restrict__ ssrc, const uint32_t *__restrict__ sdst,
                                                            const uint32_t *__restrict__ block_offset, int32_t *__restrict__ neighbors,
                                                            int32_t *__restrict__ edge_faces, uint32_t *__restrict__ row_src,
                                                            unsigned long long *counts)
{
    __shared__ uint32_t lds[4];
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
    bool head[SCAN_PER];
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++)
    {
        head[k] = is_head(V, base + k, N, ssrc, sdst);
        n += head[k];
    }
    uint32_t total, run = block_offset[blockIdx.x] + block_scan256(n, lds, &total);
    uint32_t c[4] = {n, 0, 0, 0}; // entries, boundary, manifold, nonmanifold
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++)
    {
        if (!head[k]) continue;
        const size_t j = base + k;
        const uint32_t a = ssrc[j], b = sdst[j];
        size_t lo = j + 1, hi = N; // the first position behind j whose record is above (a, b): at most 31 halvings
        while (lo < hi)
        {
            const size_t m = lo + ((hi - lo) >> 1);
            const uint32_t ma = ssrc[m];
            if (ma < a || (ma == a && sdst[m] <= b)) lo = m + 1;
            else hi = m;
        }
        const uint32_t uses = (uint32_t)(lo - j);
        if (run < N)
        {
            neighbors[run] = (int32_t)b;
            edge_faces[run] = (int32_t)uses;
            row_src[run] = a;
        }
        run++;
        c[1] += uses == 1; c[2] += uses == 2; c[3] += uses >= 3;
    }
    count4_into(counts, c);
}

// offsets[v] = the first row whose src is not below v, v = 0 .. V: at most 31 halvings of contiguous loads
__global__ void __launch_bounds__(256) row_offsets_kernel(int V, size_t N, const uint32_t *__restrict__ row_src, const uint32_t *__restrict__ entries,
                                                           int32_t *__restrict__ offsets)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v > V) return;
    size_t lo = 0, hi = min((size_t)*entries, N);
    while (lo < hi)
    {
        const size_t m = lo + ((hi - lo) >> 1);
        if (row_src[m] < (uint32_t)v) lo = m + 1;
        else hi = m;
    }
    offsets[v] = (int32_t)lo;
}

__global__ void __launch_bounds__(256) classify_kernel(int V, size_t N, const int32_t *__restrict__ offsets, const int32_t *__restrict__ edge_faces,
                                                        uint8_t *__restrict__ vertex_class)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const size_t a = (size_t)offsets[v], b = min((size_t)offsets[v + 1], N); // this call's own offsets: 0 <= a <= b <= entries
    bool one = false, many = false;
    for (size_t e = a; e < b; e++)
    {
        const int32_t uses = edge_faces[e];
        one = one || uses == 1;
        many = many || uses >= 3;
    }
    vertex_class[v] = b <= a ? 0 : many ? 3 : one ? 2 : 1; // TSS_ISOLATED, TSS_NONMANIFOLD, TSS_BOUNDARY, TSS_INTERIOR
}

// ---- smoothing -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) smooth_prepare_kernel(int V, const float *__restrict__ vertices, const uint8_t *__restrict__ vertex_class,
                                                              const uint8_t *__restrict__ pinned, int mode, double *__restrict__ q,
                                                              uint8_t *__restrict__ flag)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const float x = vertices[3 * (size_t)i], y = vertices[3 * (size_t)i + 1], z = vertices[3 * (size_t)i + 2];
    q[3 * (size_t)i] = (double)x; q[3 * (size_t)i + 1] = (double)y; q[3 * (size_t)i + 2] = (double)z;
    const bool live = finite32(x) && finite32(y) && finite32(z);
    const uint8_t cls = vertex_class[i];
    uint8_t st = ST_NONE;
    if (live && cls != 0 && !(pinned && pinned[i]))
    {
        if (mode == 2) st = ST_ROW;                                          // TSS_BOUNDARY_FREE
        else if (cls == 1) st = ST_ROW;                                      // TSS_INTERIOR
        else if (cls == 2 && mode == 1) st = ST_CURVE;                       // TSS_BOUNDARY in TSS_BOUNDARY_CURVE
    }
    flag[i] = (uint8_t)(st | (live ? LIVE : 0));
}

// One thread = one vertex.  The row is cut at num_entries and a neighbour outside [0, V) is skipped, so every load stays in the arrays the
// caller described, whatever the table holds.
__global__ void __launch_bounds__(256) smooth_step_kernel(int V, double k, const int32_t *__restrict__ offsets, const int32_t *__restrict__ neighbors,
                                                           const int32_t *__restrict__ edge_faces, int num_entries, const uint8_t *__restrict__ flag,
                                                           const double *__restrict__ qin, double *__restrict__ qout)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const double qx = qin[3 * (size_t)i], qy = qin[3 * (size_t)i + 1], qz = qin[3 * (size_t)i + 2];
    double ox = qx, oy = qy, oz = qz;
    const uint8_t st = flag[i] & ST_MASK;
    if (st != ST_NONE)
    {
        const int e0 = max(offsets[i], 0), e1 = min(offsets[i + 1], num_entries);
        double sx = 0.0, sy = 0.0, sz = 0.0;
        uint32_t n = 0;
        for (int e = e0; e < e1; e++)
        {
            if (st == ST_CURVE && edge_faces[e] != 1) continue;
            const uint32_t j = (uint32_t)neighbors[e];
            if (j >= (uint32_t)V || !(flag[j] & LIVE)) continue;
            sx += qin[3 * (size_t)j]; sy += qin[3 * (size_t)j + 1]; sz += qin[3 * (size_t)j + 2];
            n++;
        }
        if (n)
        {
            const double c = (double)n;
            const double mx = sx / c, my = sy / c, mz = sz / c;
            const double dx = mx - qx, dy = my - qy, dz = mz - qz;
            ox = qx + k * dx; oy = qy + k * dy; oz = qz + k * dz;
        }
    }
    qout[3 * (size_t)i] = ox; qout[3 * (size_t)i + 1] = oy; qout[3 * (size_t)i + 2] = oz;
}

__global__ void __launch_bounds__(256) smooth_finish_kernel(int V, const float *__restrict__ vertices, const uint8_t *__restrict__ flag,
                                                             const double *__restrict__ q, double max_move, float *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    if ((flag[i] & ST_MASK) == ST_NONE) // bit for bit
    {
        const uint32_t *src = (const uint32_t *)vertices + 3 * (size_t)i;
        uint32_t *dst = (uint32_t *)out + 3 * (size_t)i;
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
        return;
    }
#pragma unroll
    for (int a = 0; a < 3; a++)
    {
        const double q0 = (double)vertices[3 * (size_t)i + a];
        out[3 * (size_t)i + a] = (float)fmin(fmax(q[3 * (size_t)i + a], q0 - max_move), q0 + max_move);
    }
}

// ---- normals ---------------------------------------------------------------------------------------------------------------------------
// the cross product of a face whose indices are in range; false when one of its nine coordinates is not finite
__device__ __forceinline__ bool face_cross(const float *__restrict__ vertices, const int32_t (&v)[3], double (&n)[3])
{
    const float *q0 = vertices + 3 * (size_t)v[0], *q1 = vertices + 3 * (size_t)v[1], *q2 = vertices + 3 * (size_t)v[2];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; a++) finite = finite && finite32(q0[a]) && finite32(q1[a]) && finite32(q2[a]);
    const double e1x = (double)q1[0] - (double)q0[0], e1y = (double)q1[1] - (double)q0[1], e1z = (double)q1[2] - (double)q0[2];
    const double e2x = (double)q2[0] - (double)q0[0], e2y = (double)q2[1] - (double)q0[1], e2z = (double)q2[2] - (double)q0[2];
    n[0] = e1y * e2z - e1z * e2y;
    n[1] = e1z * e2x - e1x * e2z;
    n[2] = e1x * e2y - e1y * e2x;
    return finite;
}

// (float)(n / sqrt(l2)) per axis when l2 = (nx nx + ny ny) + nz nz is finite and > 0, else zeros; returns the validity
__device__ __forceinline__ bool unit_normal(const double (&n)[3], double (&u)[3])
{
    const double l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    u[0] = u[1] = u[2] = 0.0;
    if (!(finite64(l2) && l2 > 0.0)) return false;
    const double l = sqrt(l2);
    u[0] = n[0] / l; u[1] = n[1] / l; u[2] = n[2] / l;
    return true;
}

__global__ void __launch_bounds__(256) face_normals_kernel(int V, int F, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                            const uint8_t *__restrict__ keep, float *__restrict__ face_normal,
                                                            uint8_t *__restrict__ face_valid)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int32_t v[3];
    double n[3], u[3] = {0.0, 0.0, 0.0};
    bool valid = false;
    if (face_in_range(V, (size_t)f, faces, keep, v) && face_cross(vertices, v, n)) valid = unit_normal(n, u);
    face_normal[3 * (size_t)f] = (float)u[0]; face_normal[3 * (size_t)f + 1] = (float)u[1]; face_normal[3 * (size_t)f + 2] = (float)u[2];
    face_valid[f] = valid ? 1 : 0;
}

__global__ void __launch_bounds__(256) incidence_kernel(int V, int F, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                         const uint8_t *__restrict__ keep, uint32_t *__restrict__ vert, uint32_t *__restrict__ face)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int32_t v[3];
    double n[3];
    uint32_t r[3] = {(uint32_t)V, (uint32_t)V, (uint32_t)V};
    if (face_in_range(V, (size_t)f, faces, keep, v) && face_cross(vertices, v, n))
    {
        r[0] = (uint32_t)v[0];
        if (v[1] != v[0]) r[1] = (uint32_t)v[1];
        if (v[2] != v[0] && v[2] != v[1]) r[2] = (uint32_t)v[2];
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        vert[3 * (size_t)f + k] = r[k];
        face[3 * (size_t)f + k] = (uint32_t)f;
    }
}

// One thread = one vertex.  Its run's positions are bounded by 3 F, the face ids there by the incidence records (< F, their indices checked
// against V when the records were written).
__global__ void __launch_bounds__(256) vertex_normals_kernel(int V, int F, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                              const uint32_t *__restrict__ fval, const uint32_t *__restrict__ fstart,
                                                              const uint32_t *__restrict__ fend, int weighting, float *__restrict__ vertex_normal,
                                                              uint8_t *__restrict__ vertex_valid, double *__restrict__ normal_sum)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const uint32_t t0 = fstart[i], t1 = min(fend[i], 3u * (uint32_t)F);
    double s[3] = {0.0, 0.0, 0.0};
    for (uint32_t t = t0; t < t1; t++)
    {
        const uint32_t f = fval[t];
        const int32_t v[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
        double n[3], u[3];
        face_cross(vertices, v, n);
        if (weighting == 1) // TSS_NORMAL_UNIFORM: the unit normals of the valid faces
        {
            if (!unit_normal(n, u)) continue;
            s[0] += u[0]; s[1] += u[1]; s[2] += u[2];
        }
        else { s[0] += n[0]; s[1] += n[1]; s[2] += n[2]; }
    }
    double u[3];
    const bool valid = unit_normal(s, u);
    vertex_normal[3 * (size_t)i] = (float)u[0]; vertex_normal[3 * (size_t)i + 1] = (float)u[1]; vertex_normal[3 * (size_t)i + 2] = (float)u[2];
    vertex_valid[i] = valid ? 1 : 0;
    if (normal_sum) { normal_sum[3 * (size_t)i] = s[0]; normal_sum[3 * (size_t)i + 1] = s[1]; normal_sum[3 * (size_t)i + 2] = s[2]; }
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------
struct AdjacencyCarve
{
    uint32_t *k[2], *v[2], *block_count, *entries;
    void *scratch;
    size_t nb, bytes;
};
AdjacencyCarve adjacency_carve(void *ws, size_t F)
{
    AdjacencyCarve c;
    Carver w(ws);
    const size_t N = 6 * F;
    c.nb = scan_blocks(N);
    c.k[0] = w.words(N); c.k[1] = w.words(N); c.v[0] = w.words(N); c.v[1] = w.words(N);
    c.block_count = w.words(c.nb);
    c.entries = w.words(1);
    c.scratch = w.bytes(sort_scratch_bytes(N));
    c.bytes = w.used();
    return c;
}

struct SmoothCarve
{
    double *q[2];
    uint8_t *flag;
    size_t bytes;
};
SmoothCarve smooth_carve(void *ws, size_t V)
{
    SmoothCarve c;
    Carver w(ws);
    c.q[0] = (double *)w.bytes(V * 3 * sizeof(double)); c.q[1] = (double *)w.bytes(V * 3 * sizeof(double));
    c.flag = (uint8_t *)w.bytes(V);
    c.bytes = w.used();
    return c;
}

struct NormalCarve
{
    uint32_t *bounds; // fstart, fend: 2 x V words, cleared in one go
    uint32_t *fk[2], *fv[2];
    void *scratch;
    size_t bytes;
};
NormalCarve normal_carve(void *ws, size_t V, size_t F)
{
    NormalCarve c;
    Carver w(ws);
    c.bounds = w.words(2 * V);
    c.fk[0] = w.words(3 * F); c.fk[1] = w.words(3 * F); c.fv[0] = w.words(3 * F); c.fv[1] = w.words(3 * F);
    c.scratch = w.bytes(sort_scratch_bytes(3 * F));
    c.bytes = w.used();
    return c;
}
} // namespace

size_t ts_smooth_workspace_bytes(int V, int F)
{
    const size_t v = (size_t)(V > 0 ? V : 0), f = (size_t)(F > 0 ? F : 0);
    return std::max(adjacency_carve(nullptr, f).bytes, std::max(smooth_carve(nullptr, v).bytes, normal_carve(nullptr, v, f).bytes)) + 2 * TS_ALIGN;
}

hipError_t ts_smooth_adjacency(int V, int F, const int32_t *faces, const uint8_t *keep, int32_t *offsets, int32_t *neighbors, int32_t *edge_faces,
                               uint8_t *vertex_class, unsigned long long *counts, void *ws, hipStream_t s)
{
    hipError_t e = mesh_fill(counts, 0, 4 * sizeof(unsigned long long), s);
    if (e != hipSuccess || V <= 0) return e;
    const size_t f = (size_t)(F > 0 ? F : 0), N = 6 * f;
    if (N == 0) // every row is empty
    {
        e = mesh_fill(offsets, 0, ((size_t)V + 1) * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
        return mesh_fill(vertex_class, 0, (size_t)V, s);
    }
    const AdjacencyCarve c = adjacency_carve(ws, f);
    e = mesh_fill(neighbors, 0xFF, N * sizeof(int32_t), s); // entries from offsets[V] on stay -1 ...
    if (e != hipSuccess) return e;
    e = mesh_fill(edge_faces, 0, N * sizeof(int32_t), s); // ... and 0
    if (e != hipSuccess) return e;
    const int bits = bit_length((uint32_t)V); // the sentinel V included
    hipLaunchKernelGGL(records_kernel, dim3(blocks256(f)), dim3(256), 0, s, V, F, faces, keep, c.k[0], c.v[0]);
    const int at = ts_radix_sort_pairs(c.k, c.v, N, bits, c.scratch, s); // by dst, stable
    uint32_t *const k2[2] = {c.v[at], c.v[at ^ 1]}, *const v2[2] = {c.k[at], c.k[at ^ 1]};
    const int at2 = ts_radix_sort_pairs(k2, v2, N, bits, c.scratch, s); // then by src, stable: (src, dst) order
    const uint32_t *ssrc = k2[at2], *sdst = v2[at2];
    uint32_t *row_src = k2[at2 ^ 1]; // the partner of the sorted src column is free now
    const unsigned nb = (unsigned)c.nb;
    hipLaunchKernelGGL(head_count_kernel, dim3(nb), dim3(256), 0, s, V, N, ssrc, sdst, c.block_count);
    hipLaunchKernelGGL(scan_offsets_kernel<1>, dim3(1), dim3(256), 0, s, (int)nb, c.block_count, c.entries);
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(nb), dim3(256), 0, s, V, N, ssrc, sdst, c.block_count, neighbors, edge_faces, row_src, counts);
    hipLaunchKernelGGL(row_offsets_kernel, dim3(blocks256((size_t)V + 1)), dim3(256), 0, s, V, N, row_src, c.entries, offsets);
    hipLaunchKernelGGL(classify_kernel, dim3(blocks256((size_t)V)), dim3(256), 0, s, V, N, offsets, edge_faces, vertex_class);
    return hipGetLastError();
}

hipError_t ts_smooth_smooth(int V, const float *vertices, const int32_t *offsets, const int32_t *neighbors, const int32_t *edge_faces, int num_entries,
                            const uint8_t *vertex_class, const uint8_t *pinned, float lambda, float mu, int iterations, int boundary_mode,
                            float max_move, float *out_vertices, void *ws, hipStream_t s)
{
    if (V <= 0) return hipSuccess;
    const size_t n = (size_t)V;
    const SmoothCarve c = smooth_carve(ws, n);
    const unsigned nv = blocks256(n);
    hipLaunchKernelGGL(smooth_prepare_kernel, dim3(nv), dim3(256), 0, s, V, vertices, vertex_class, pinned, boundary_mode, c.q[0], c.flag);
    int at = 0;
    for (int it = 0; it < iterations; it++)
        for (int half = 0; half < 2; half++, at ^= 1)
            hipLaunchKernelGGL(smooth_step_kernel, dim3(nv), dim3(256), 0, s, V, (double)(half ? mu : lambda), offsets, neighbors, edge_faces,
                               num_entries, c.flag, c.q[at], c.q[at ^ 1]);
    hipLaunchKernelGGL(smooth_finish_kernel, dim3(nv), dim3(256), 0, s, V, vertices, c.flag, c.q[at], (double)max_move, out_vertices);
    return hipGetLastError();
}

hipError_t ts_smooth_face_normals(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, float *face_normal,
                                  uint8_t *face_valid, hipStream_t s)
{
    if (F <= 0) return hipSuccess;
    hipLaunchKernelGGL(face_normals_kernel, dim3(blocks256((size_t)F)), dim3(256), 0, s, V, F, vertices, faces, keep, face_normal, face_valid);
    return hipGetLastError();
}

hipError_t ts_smooth_vertex_normals(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, int weighting,
                                    float *vertex_normal, uint8_t *vertex_valid, double *normal_sum, void *ws, hipStream_t s)
{
    if (V <= 0) return hipSuccess;
    const size_t n = (size_t)V, f = (size_t)(F > 0 ? F : 0);
    const NormalCarve c = normal_carve(ws, n, f);
    hipError_t e = mesh_fill(c.bounds, 0, 2 * n * sizeof(uint32_t), s); // a vertex without a run: start == end == 0
    if (e != hipSuccess) return e;
    uint32_t *fstart = c.bounds, *fend = c.bounds + n;
    int fat = 0;
    if (f > 0)
    {
        hipLaunchKernelGGL(incidence_kernel, dim3(blocks256(f)), dim3(256), 0, s, V, F, vertices, faces, keep, c.fk[0], c.fv[0]);
        fat = ts_radix_sort_pairs(c.fk, c.fv, 3 * f, bit_length((uint32_t)V), c.scratch, s); // the sentinel V included; stable: a vertex's faces ascending
        hipLaunchKernelGGL(run_bounds_kernel, dim3(blocks256(3 * f)), dim3(256), 0, s, 3 * f, c.fk[fat], (uint32_t)V, fstart, fend);
    }
    hipLaunchKernelGGL(vertex_normals_kernel, dim3(blocks256(n)), dim3(256), 0, s, V, (int)f, vertices, faces, c.fv[fat], fstart, fend, weighting,
                       vertex_normal, vertex_valid, normal_sum);
    return hipGetLastError();
}
