// mesh_orient.hip -- every orientable piece of an indexed mesh made to wind one way, the non-orientable pieces reported, the way each piece
// faces chosen by a stated rule (include/ts_orient.h).
//
// Built with -ffp-contract=off: the signed-volume terms of mode 2 are float64 on widened fp32 and every operation rounds once, as in
// tests/ref_mesh_orient.py.  The atomics are integer: the compare-exchange and the minimum of the union-find (csrc/ts_union_find.h), the
// 64-bit maximum of a piece's largest difference, the 32- and 64-bit adds of the per-piece sums and of the counters.
//
// Front.  The sort-by-edge front shared with mesh_manifold.hip (csrc/ts_mesh_edges.h): the half-edges of the faces that take part in
// (min, max, half-edge) order.  The records kernel is this unit's own: it also sets the two parent words of a face and counts the faces.
//
// Links.  One thread per sorted position; the head of a run of exactly two unites two pairs of nodes of the doubled graph over 2 F nodes
// (2 f: f as given, 2 f + 1: f reversed): straight for half-edges that run in opposite directions, crosswise for two that leave the same
// vertex.  Flatten.  One thread per face: r0 = root(2 f), r1 = root(2 f + 1); the piece is min(r0, r1) >> 1, it is non-orientable iff
// r0 == r1, the consistency flip is r0 & 1 otherwise.  The flip and the non-orientable bit wait in face_flip until the deciding pass
// overwrites them.  Per-piece sums (faces, flips; for mode 2 the largest difference, then the quantised volume) are indexed by the anchor
// face; by_label reduces equal labels within the wave first, so that a mesh that is one piece sends one add per wave, not per face.
#include "ts_mesh_edges.h"
#include "ts_orient_launch.h"
#include "ts_union_find.h"

namespace
{
constexpr int LABEL_ROUNDS = 4; // distinct labels of a wave that are reduced before the rest of its lanes add one by one

// Every active lane hands (label, value) to commit, equal labels combined first: up to LABEL_ROUNDS times the first lane still waiting
// names its label, the lanes with that label are combined over the wave and the leader commits once; who is left commits its own.  All 64
// lanes of the wave call this together (no lane has returned); combine is associative and commutative, commit an integer atomic: the
// result does not depend on who was combined with whom.
template <typename T, typename Combine, typename Commit>
__device__ __forceinline__ void by_label(bool active, uint32_t label, T value, T identity, Combine combine, Commit commit)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(active);
    for (int round = 0; round < LABEL_ROUNDS && todo; round++)
    {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t l = __shfl(label, leader);
        const bool mine = ((todo >> lane) & 1) && label == l;
        T v = mine ? value : identity;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = combine(v, (T)__shfl_xor(v, o));
        if (lane == leader) commit(l, v);
        todo &= ~__ballot(mine);
    }
    if ((todo >> lane) & 1) commit(label, value);
}

// ---- the records of the front ----------------------------------------------------------------------------------------------------------------
// One thread = one face: its three records and the identity of its two parent words.
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
        parent[2 * (size_t)f] = 2u * (uint32_t)f;
        parent[2 * (size_t)f + 1] = 2u * (uint32_t)f + 1u;
        n = ok ? 1u : 0u;
    }
    count_into(counts + 0, n);
}

// ---- links, pieces -----------------------------------------------------------------------------------------------------------------------
// One thread = one sorted position.  The half-edges are below N = 3 F, so their faces are below F and their nodes below 2 F.
__global__ void __launch_bounds__(256) link_kernel(int V, size_t N, const int32_t *__restrict__ faces, const uint32_t *__restrict__ smin,
                                                    const uint32_t *__restrict__ smax, const uint32_t *__restrict__ sval, uint32_t *parent,
                                                    unsigned long long *counts)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t linking = 0, same = 0;
    if (edge_run_head(V, N, j, smin, smax) == 2) // a linking edge: j + 1 < N
    {
        const uint32_t h0 = sval[j], h1 = sval[j + 1];
        const uint32_t f = h0 / 3u, g = h1 / 3u;
        linking = 1;
        same = faces[h0] == faces[h1]; // both leave the same vertex: an odd link
        uf_union(parent, 2u * f, 2u * g + same);
        uf_union(parent, 2u * f + 1u, 2u * g + 1u - same);
    }
    count_into(counts + 4, linking);
    count_into(counts + 5, same);
}

// One thread = one face.  mark: the consistency flip in bit 0, the non-orientable bit in bit 1, until decide_kernel overwrites it.
__global__ void __launch_bounds__(256) flatten_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep,
                                                       uint32_t *parent, int32_t *__restrict__ face_piece, uint8_t *__restrict__ mark,
                                                       uint32_t *piece_faces, uint32_t *piece_flips, unsigned long long *counts)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    bool ok = false, twisted = false;
    uint32_t piece = 0, flip = 0;
    if (f < F)
    {
        int32_t v[3];
        ok = face_takes_part(V, (size_t)f, faces, keep, v);
        if (ok)
        {
            const uint32_t r0 = uf_find(parent, 2u * (uint32_t)f, false), r1 = uf_find(parent, 2u * (uint32_t)f + 1u, false);
            piece = min(r0, r1) >> 1;
            twisted = r0 == r1;
            flip = twisted ? 0u : (r0 & 1u);
        }
        face_piece[f] = ok ? (int32_t)piece : -1;
        mark[f] = (uint8_t)(flip | (twisted ? 2u : 0u));
    }
    const bool anchor = ok && piece == (uint32_t)f;
    count_into(counts + 1, anchor);
    count_into(counts + 2, anchor && twisted);
    count_into(counts + 3, twisted);
    // a piece's faces in the low word, its flips in the high one: a wave adds at most 64 of either
    by_label<unsigned long long>(
        ok, piece, 1ull | ((unsigned long long)flip << 32), 0ull, [](unsigned long long a, unsigned long long b) { return a + b; },
        [&](uint32_t p, unsigned long long v) {
            atomicAdd(piece_faces + p, (uint32_t)v);
            if (v >> 32) atomicAdd(piece_flips + p, (uint32_t)(v >> 32));
        });
}

// ---- mode 2: the quantised signed volume ----------------------------------------------------------------------------------------------------
// The nine differences of face f from o, slot 0 of its piece's anchor face, and whether all are finite.  The face takes part, and so does
// the anchor: all four indices are in [0, V).
__device__ __forceinline__ bool differences(size_t f, uint32_t piece, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                            double (&d)[9])
{
    const size_t o = 3 * (size_t)faces[3 * (size_t)piece];
    const double ox = (double)vertices[o], oy = (double)vertices[o + 1], oz = (double)vertices[o + 2];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const size_t x = 3 * (size_t)faces[3 * f + k];
        d[3 * k] = (double)vertices[x] - ox;
        d[3 * k + 1] = (double)vertices[x + 1] - oy;
        d[3 * k + 2] = (double)vertices[x + 2] - oz;
        finite = finite && isfinite(d[3 * k]) && isfinite(d[3 * k + 1]) && isfinite(d[3 * k + 2]);
    }
    return finite;
}

// One thread = one face: the largest |d| of a face whose differences are all finite, as the bits of a non-negative double, which order as
// integers.
__global__ void __launch_bounds__(256) largest_kernel(int F, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                       const int32_t *__restrict__ face_piece, unsigned long long *piece_largest)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int32_t piece = f < F ? face_piece[f] : -1;
    bool finite = false;
    unsigned long long bits = 0;
    if (piece >= 0)
    {
        double d[9];
        finite = differences((size_t)f, (uint32_t)piece, vertices, faces, d);
        double m = 0.0;
#pragma unroll
        for (int k = 0; k < 9; k++) m = fmax(m, fabs(d[k]));
        bits = finite ? (unsigned long long)__double_as_longlong(m) : 0ull;
    }
    by_label<unsigned long long>(
        finite, (uint32_t)piece, bits, 0ull, [](unsigned long long a, unsigned long long b) { return a > b ? a : b; },
        [&](uint32_t p, unsigned long long v) { if (v) __hip_atomic_fetch_max(piece_largest + p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
}

// One thread = one face: q = llrint(ldexp(t, k_p)), added to its piece with the sign of its consistency flip.
__global__ void __launch_bounds__(256) terms_kernel(int F, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                     const int32_t *__restrict__ face_piece, const uint8_t *__restrict__ mark,
                                                     const uint32_t *__restrict__ piece_faces, const unsigned long long *__restrict__ piece_largest,
                                                     long long *piece_volume, unsigned long long *counts)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int32_t piece = f < F ? face_piece[f] : -1;
    long long q = 0;
    uint32_t nonfinite = 0;
    if (piece >= 0)
    {
        double d[9];
        const bool finite = differences((size_t)f, (uint32_t)piece, vertices, faces, d);
        const double X = d[4] * d[8] - d[5] * d[7], Y = d[5] * d[6] - d[3] * d[8], Z = d[3] * d[7] - d[4] * d[6];
        const double t = (d[0] * X + d[1] * Y) + d[2] * Z;
        if (finite && isfinite(t))
        {
            // m_p is 0 or the difference of two fp32 values, at least 2^-149: a normal double, whose frexp exponent is its biased one - 1022
            const unsigned long long bits = piece_largest[piece];
            const int e = bits ? (int)((bits >> 52) & 0x7ffu) - 1022 : 0;
            const int k = 56 - (32 - __clz((int)piece_faces[piece])) - 3 * e;
            q = llrint(ldexp(t, k));
            if (mark[f] & 1) q = -q;
        }
        else
            nonfinite = 1;
    }
    count_into(counts + 9, nonfinite);
    by_label<long long>(
        q != 0, (uint32_t)piece, q, 0ll, [](long long a, long long b) { return a + b; },
        [&](uint32_t p, long long v) {
            if (v) __hip_atomic_fetch_add((unsigned long long *)piece_volume + p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        });
}

// ---- the decision and the faces ----------------------------------------------------------------------------------------------------------------
// One thread = one face: reads its own mark, writes its own face_flip and row.
__global__ void __launch_bounds__(256) decide_kernel(int F, int mode, const int32_t *__restrict__ faces, const int32_t *__restrict__ face_piece,
                                                      const uint32_t *__restrict__ piece_faces, const uint32_t *__restrict__ piece_flips,
                                                      const long long *__restrict__ piece_volume, uint8_t *face_flip,
                                                      int32_t *__restrict__ out_faces, unsigned long long *counts)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    uint32_t flipped = 0, inverted = 0;
    if (f < F)
    {
        const int32_t piece = face_piece[f];
        const uint32_t mark = face_flip[f];
        if (piece >= 0 && !(mark & 2u))
        {
            bool invert = false;
            if (mode == 1) invert = 2u * piece_flips[piece] > piece_faces[piece];
            else if (mode == 2) invert = piece_volume[piece] < 0;
            flipped = (mark & 1u) ^ (invert ? 1u : 0u);
            inverted = invert && piece == f;
        }
        face_flip[f] = (uint8_t)flipped;
        const int32_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        out_faces[3 * (size_t)f] = a;
        out_faces[3 * (size_t)f + 1] = flipped ? c : b;
        out_faces[3 * (size_t)f + 2] = flipped ? b : c;
    }
    count_into(counts + 7, flipped);
    count_into(counts + 8, inverted);
}

// One thread = one sorted position: the linking edges whose half-edges still run the same way once the flips are applied.
__global__ void __launch_bounds__(256) after_kernel(int V, size_t N, const int32_t *__restrict__ faces, const uint32_t *__restrict__ smin,
                                                     const uint32_t *__restrict__ smax, const uint32_t *__restrict__ sval,
                                                     const uint8_t *__restrict__ face_flip, unsigned long long *counts)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t same = 0;
    if (edge_run_head(V, N, j, smin, smax) == 2) // a linking edge: j + 1 < N
    {
        const uint32_t h0 = sval[j], h1 = sval[j + 1];
        same = (uint32_t)(faces[h0] == faces[h1]) ^ face_flip[h0 / 3u] ^ face_flip[h1 / 3u];
    }
    count_into(counts + 6, same);
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------
struct OrientCarve
{
    EdgeSortCarve sort;
    uint32_t *parent, *piece_faces, *piece_flips;
    unsigned long long *piece_largest;
    long long *piece_volume;
    void *sums;
    size_t sums_bytes, bytes;
};
OrientCarve orient_carve(void *ws, size_t F)
{
    OrientCarve c;
    Carver w(ws);
    c.sort = edge_sort_carve(w, 3 * F);
    c.parent = w.words(2 * F);
    c.sums_bytes = 24 * F; // the per-piece sums in one block, cleared by one fill (mesh_fill): the 64-bit columns first
    c.sums = w.bytes(c.sums_bytes);
    c.piece_largest = (unsigned long long *)c.sums;
    c.piece_volume = (long long *)(c.piece_largest + F);
    c.piece_faces = (uint32_t *)(c.piece_volume + F);
    c.piece_flips = c.piece_faces + F;
    c.bytes = w.used();
    return c;
}
} // namespace

size_t ts_orient_workspace_bytes(int V, int F)
{
    (void)V; // the records are per face; V only sets the number of key bits
    return orient_carve(nullptr, (size_t)(F > 0 ? F : 0)).bytes + 2 * TS_ALIGN;
}

hipError_t ts_orient_faces(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, int mode, int32_t *face_piece,
                           uint8_t *face_flip, int32_t *out_faces, unsigned long long *counts, void *ws, hipStream_t s)
{
    hipError_t e = mesh_fill(counts, 0, 10 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const size_t f = (size_t)(F > 0 ? F : 0), N = 3 * f;
    if (N == 0) return hipSuccess;
    if (V <= 0) // nothing takes part
    {
        e = mesh_fill(face_piece, 0xFF, f * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
        e = mesh_fill(face_flip, 0, f, s);
        if (e != hipSuccess) return e;
        return mesh_copy(out_faces, faces, N * sizeof(int32_t), s);
    }
    const OrientCarve c = orient_carve(ws, f);
    e = mesh_fill(c.sums, 0, c.sums_bytes, s);
    if (e != hipSuccess) return e;
    const unsigned nf = blocks256(f), nh = blocks256(N);
    hipLaunchKernelGGL(records_kernel, dim3(nf), dim3(256), 0, s, V, F, faces, keep, c.sort.k[0], c.sort.v[0], c.parent, counts);
    const SortedEdges edges = sort_half_edges(V, N, faces, c.sort, s);
    hipLaunchKernelGGL(link_kernel, dim3(nh), dim3(256), 0, s, V, N, faces, edges.smin, edges.smax, edges.sval, c.parent, counts);
    hipLaunchKernelGGL(flatten_kernel, dim3(nf), dim3(256), 0, s, V, F, faces, keep, c.parent, face_piece, face_flip, c.piece_faces,
                       c.piece_flips, counts);
    if (mode == 2)
    {
        hipLaunchKernelGGL(largest_kernel, dim3(nf), dim3(256), 0, s, F, vertices, faces, face_piece, c.piece_largest);
        hipLaunchKernelGGL(terms_kernel, dim3(nf), dim3(256), 0, s, F, vertices, faces, face_piece, face_flip, c.piece_faces, c.piece_largest,
                           c.piece_volume, counts);
    }
    hipLaunchKernelGGL(decide_kernel, dim3(nf), dim3(256), 0, s, F, mode, faces, face_piece, c.piece_faces, c.piece_flips, c.piece_volume,
                       face_flip, out_faces, counts);
    hipLaunchKernelGGL(after_kernel, dim3(nh), dim3(256), 0, s, V, N, faces, edges.smin, edges.smax, edges.sval, face_flip, counts);
    return hipGetLastError();
}
