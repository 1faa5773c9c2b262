// mesh_simplify.hip -- vertex clustering on a uniform grid with quadric error placement, and the duplicate-face sweep (include/ts_simplify.h).
//
// Built with -ffp-contract=off: every float64 operation of the header's text rounds, which is what makes the result bit-equal to
// tests/ref_mesh_simplify.py.  No floating-point atomics anywhere; the only atomics are integer adds to the two counters of the sweep.
//
// Labels.  One thread per vertex forms the 63-bit cell key as two 32-bit words (lo = cy[10:0] << 21 | cx, hi = cz << 10 | cy[20:11]); an
// invalid vertex gets all ones in both, which sorts behind every valid key (a valid hi is below 2^31).  Two stable LSD sorts of (word, index)
// with the product's radix passes -- by lo, then by hi gathered in that order -- leave the indices in (key, index) order: a run of equal keys
// holds one cluster's members ascending, and its head is the label.  Every position finds its run's head by a lower-bound search among the
// sorted keys (log2 V steps of contiguous loads): nobody waits for a neighbour and there is no scan.  Invalid vertices label themselves.
//
// Placement.  remap (the cluster ranks of ts2d_weld_compact) is the sort key, only the bits V needs: a stable sort of (rank, index) gives
// each cluster's members ascending, and the head and the tail of each run write the run's bounds (csrc/ts_mesh_runs.h).
// One thread per face writes up to three incidence records (rank, face) into its three slots (the sentinel rank V in a slot it does not use: the face does not contribute, the
// vertex is invalid, or an earlier valid vertex of the face already named the cluster); a stable sort by rank leaves each cluster's faces
// ascending.  Then ONE thread per cluster walks its member run and its face run in order, accumulates, solves, clamps and writes: the sums
// are sequential by definition, so the cost is linear in the largest cluster (the header says so).  A rank that no vertex holds (V' .. V - 1)
// writes zero rows.
//
// Duplicates.  One thread per face rotates its triple (a < b, a < c) or writes the sentinel V; three stable sorts (by c, by b, by a, each key
// gathered through the order so far) put the faces in (a, b, c, face) order.  A face whose predecessor holds the same triple is a duplicate;
// a survivor looks its reversed triple (a, c, b) up by a lower-bound search: a run of equal triples always has exactly one survivor, so the
// triple's presence is the twin's survival.
#include "ts_mesh_runs.h"
#include "ts_simplify_launch.h"

namespace
{
constexpr uint32_t KEY_INVALID = 0xFFFFFFFFu; // both words of an invalid vertex's key
constexpr int MAXC = 8;                        // TSQ_MAX_CHANNELS

// c = floor(((double)x - (double)o) / (double)cell); false unless x is finite and 0 <= c < 2^21
__device__ __forceinline__ bool cell_index(float x, float o, float cell, uint32_t &c)
{
    c = 0u;
    if (!finite32(x)) return false;
    const double g = ((double)x - (double)o) / (double)cell;
    const double fl = floor(g);
    if (!(fl >= 0.0 && fl < 2097152.0)) return false;
    c = (uint32_t)fl;
    return true;
}

__device__ __forceinline__ bool vertex_cell(const float *__restrict__ vertices, uint32_t i, float ox, float oy, float oz, float cell, uint32_t (&c)[3])
{
    const float x = vertices[3 * (size_t)i], y = vertices[3 * (size_t)i + 1], z = vertices[3 * (size_t)i + 2];
    const bool vx = cell_index(x, ox, cell, c[0]), vy = cell_index(y, oy, cell, c[1]), vz = cell_index(z, oz, cell, c[2]);
    return vx && vy && vz;
}

// ---- labels ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cell_keys_kernel(int V, const float *__restrict__ vertices, float ox, float oy, float oz, float cell,
                                                         uint32_t *__restrict__ key_lo, uint32_t *__restrict__ key_hi, uint32_t *__restrict__ sort_key,
                                                         uint32_t *__restrict__ ids)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    uint32_t c[3];
    uint32_t lo = KEY_INVALID, hi = KEY_INVALID;
    if (vertex_cell(vertices, (uint32_t)i, ox, oy, oz, cell, c))
    {
        lo = ((c[1] & 0x7FFu) << 21) | c[0];
        hi = (c[2] << 10) | (c[1] >> 11);
    }
    key_lo[i] = lo; key_hi[i] = hi;
    sort_key[i] = lo;
    ids[i] = (uint32_t)i;
}

// out[j] = table[order[j]]: the next sort's key (or a sorted column) gathered through the order so far.  order[j] < n by construction.
__global__ void __launch_bounds__(256) gather_kernel(size_t n, const uint32_t *__restrict__ table, const uint32_t *__restrict__ order,
                                                      uint32_t *__restrict__ out)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) out[j] = table[order[j]];
}

__global__ void __launch_bounds__(256) run_head_label_kernel(int V, const uint32_t *__restrict__ shi, const uint32_t *__restrict__ slo,
                                                              const uint32_t *__restrict__ sid, int32_t *__restrict__ label)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= V) return;
    const uint32_t hi = shi[j], lo = slo[j], me = sid[j];
    if (hi == KEY_INVALID) { label[me] = (int32_t)me; return; } // its own cluster
    int a = 0, b = j; // the first position in [0, j] whose key is not below mine: at most 31 halvings
    while (a < b)
    {
        const int m = a + ((b - a) >> 1);
        const uint32_t h = shi[m];
        if (h < hi || (h == hi && slo[m] < lo)) a = m + 1;
        else b = m;
    }
    label[me] = (int32_t)sid[a];
}

// ---- placement -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) member_keys_kernel(int V, const int32_t *__restrict__ remap, uint32_t *__restrict__ keys,
                                                           uint32_t *__restrict__ ids)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const uint32_t r = (uint32_t)remap[i];
    keys[i] = r < (uint32_t)V ? r : 0u; // a rank is always < V; the test only keeps a foreign array in bounds
    ids[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) incidence_kernel(int V, int F, const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                         const int32_t *__restrict__ remap, float ox, float oy, float oz, float cell,
                                                         uint32_t *__restrict__ rank, uint32_t *__restrict__ face)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int32_t v[3];
    uint32_t r[3] = {(uint32_t)V, (uint32_t)V, (uint32_t)V};
    if (face_in_range(V, (size_t)f, faces, nullptr, v))
    {
        bool valid[3], finite = true;
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
            const float *p = vertices + 3 * (size_t)v[k];
            finite = finite && finite32(p[0]) && finite32(p[1]) && finite32(p[2]);
            uint32_t c[3];
            valid[k] = vertex_cell(vertices, (uint32_t)v[k], ox, oy, oz, cell, c);
        }
        if (finite)
        {
            uint32_t q[3];
#pragma unroll
            for (int k = 0; k < 3; k++)
            {
                const uint32_t m = (uint32_t)remap[v[k]];
                q[k] = m < (uint32_t)V ? m : 0u; // as member_keys_kernel reads it
            }
            if (valid[0]) r[0] = q[0];
            if (valid[1] && !(valid[0] && q[0] == q[1])) r[1] = q[1];
            if (valid[2] && !(valid[0] && q[0] == q[2]) && !(valid[1] && q[1] == q[2])) r[2] = q[2];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        rank[3 * (size_t)f + k] = r[k];
        face[3 * (size_t)f + k] = (uint32_t)f;
    }
}

struct PlaceArgs
{
    const float *vertices;
    const int32_t *faces;
    const float *attributes;
    const uint8_t *attr_valid;
    const uint32_t *mids, *mstart, *mend, *fval, *fstart, *fend;
    float *out_vertices, *out_attributes;
    uint8_t *out_valid;
    int32_t *member_count;
    float ox, oy, oz, cell, lambda;
    int V, F, mode, C;
};

// One thread = one cluster rank.  Every index it follows is bounded: member positions by the run bounds (<= V, written by run_bounds_kernel
// from positions of the sorted list), member ids by the sort (a permutation of 0 .. V - 1), face ids by the incidence records (< F, indices
// checked there against V).
__global__ void __launch_bounds__(256) place_kernel(PlaceArgs a)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.V) return;
    const uint32_t j0 = a.mstart[r], j1 = min(a.mend[r], (uint32_t)a.V);
    const bool attrs = a.attributes != nullptr;
    float *ov = a.out_vertices + 3 * (size_t)r;
    if (j1 <= j0) // no vertex holds this rank: rows V' .. V - 1 are zero
    {
        ov[0] = 0.0f; ov[1] = 0.0f; ov[2] = 0.0f;
        a.member_count[r] = 0;
        if (attrs)
        {
            for (int ch = 0; ch < a.C; ch++) a.out_attributes[(size_t)r * a.C + ch] = 0.0f;
            a.out_valid[r] = 0;
        }
        return;
    }
    const uint32_t head = a.mids[j0];
    uint32_t c[3];
    const bool valid = vertex_cell(a.vertices, head, a.ox, a.oy, a.oz, a.cell, c);
    const double cell = (double)a.cell;
    const double ccx = (double)a.ox + cell * ((double)c[0] + 0.5), ccy = (double)a.oy + cell * ((double)c[1] + 0.5),
                 ccz = (double)a.oz + cell * ((double)c[2] + 0.5);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    double acc[MAXC];
#pragma unroll
    for (int ch = 0; ch < MAXC; ch++) acc[ch] = 0.0;
    uint32_t nattr = 0u;
    for (uint32_t j = j0; j < j1; j++)
    {
        const uint32_t id = a.mids[j];
        const float *p = a.vertices + 3 * (size_t)id;
        sx += (double)p[0] - ccx; sy += (double)p[1] - ccy; sz += (double)p[2] - ccz;
        if (attrs && (!a.attr_valid || a.attr_valid[id]))
        {
            nattr++;
            const float *q = a.attributes + (size_t)id * a.C;
#pragma unroll
            for (int ch = 0; ch < MAXC; ch++)
                if (ch < a.C) acc[ch] += (double)q[ch];
        }
    }
    const uint32_t count = j1 - j0;
    a.member_count[r] = (int32_t)count;
    if (attrs)
    {
#pragma unroll
        for (int ch = 0; ch < MAXC; ch++)
            if (ch < a.C) a.out_attributes[(size_t)r * a.C + ch] = nattr ? (float)(acc[ch] / (double)nattr) : 0.0f;
        a.out_valid[r] = nattr ? 1 : 0;
    }
    if (!valid) // its head's position, bit for bit
    {
        const uint32_t *src = (const uint32_t *)a.vertices + 3 * (size_t)head;
        uint32_t *dst = (uint32_t *)ov;
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
        return;
    }
    const double n = (double)count;
    const double mx = sx / n, my = sy / n, mz = sz / n;
    double x0 = mx, x1 = my, x2 = mz;
    if (a.mode == 1)
    {
        double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        const uint32_t t0 = a.fstart[r], t1 = min(a.fend[r], 3u * (uint32_t)a.F);
        for (uint32_t t = t0; t < t1; t++)
        {
            const uint32_t f = a.fval[t];
            const int32_t i0 = a.faces[3 * (size_t)f], i1 = a.faces[3 * (size_t)f + 1], i2 = a.faces[3 * (size_t)f + 2];
            const float *q0 = a.vertices + 3 * (size_t)i0, *q1 = a.vertices + 3 * (size_t)i1, *q2 = a.vertices + 3 * (size_t)i2;
            const double p0x = (double)q0[0] - ccx, p0y = (double)q0[1] - ccy, p0z = (double)q0[2] - ccz;
            const double p1x = (double)q1[0] - ccx, p1y = (double)q1[1] - ccy, p1z = (double)q1[2] - ccz;
            const double p2x = (double)q2[0] - ccx, p2y = (double)q2[1] - ccy, p2z = (double)q2[2] - ccz;
            const double e1x = p1x - p0x, e1y = p1y - p0y, e1z = p1z - p0z;
            const double e2x = p2x - p0x, e2y = p2y - p0y, e2z = p2z - p0z;
            const double nx = e1y * e2z - e1z * e2y;
            const double ny = e1z * e2x - e1x * e2z;
            const double nz = e1x * e2y - e1y * e2x;
            const double d = -((nx * p0x + ny * p0y) + nz * p0z);
            a00 += nx * nx; a01 += nx * ny; a02 += nx * nz; a11 += ny * ny; a12 += ny * nz; a22 += nz * nz;
            b0 += nx * d; b1 += ny * d; b2 += nz * d;
        }
        const double tr = (a00 + a11) + a22;
        if (finite64(tr) && tr > 0.0)
        {
            const double mu = (double)a.lambda * tr;
            a00 += mu; a11 += mu; a22 += mu;
            const double r0 = mu * mx - b0, r1 = mu * my - b1, r2 = mu * mz - b2;
            const double c00 = a11 * a22 - a12 * a12;
            const double c01 = a02 * a12 - a01 * a22;
            const double c02 = a01 * a12 - a02 * a11;
            const double c11 = a00 * a22 - a02 * a02;
            const double c12 = a01 * a02 - a00 * a12;
            const double c22 = a00 * a11 - a01 * a01;
            const double det = (a00 * c00 + a01 * c01) + a02 * c02;
            if (finite64(det) && det > 0.0)
            {
                const double y0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
                const double y1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
                const double y2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
                if (finite64(y0) && finite64(y1) && finite64(y2)) { x0 = y0; x1 = y1; x2 = y2; }
            }
        }
    }
    const double half = 0.5 * cell;
    x0 = fmin(fmax(x0, -half), half); x1 = fmin(fmax(x1, -half), half); x2 = fmin(fmax(x2, -half), half);
    ov[0] = (float)(ccx + x0); ov[1] = (float)(ccy + x1); ov[2] = (float)(ccz + x2);
}

// ---- duplicate faces ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rotated_triples_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep,
                                                               uint32_t *__restrict__ ta, uint32_t *__restrict__ tb, uint32_t *__restrict__ tc,
                                                               uint32_t *__restrict__ sort_key, uint32_t *__restrict__ ids)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int32_t v[3];
    uint32_t a = (uint32_t)V, b = (uint32_t)V, c = (uint32_t)V;
    if (face_takes_part(V, (size_t)f, faces, keep, v)) // keep is never null here
    {
        const uint32_t x = (uint32_t)v[0], y = (uint32_t)v[1], z = (uint32_t)v[2];
        if (x < y && x < z) { a = x; b = y; c = z; }
        else if (y < z) { a = y; b = z; c = x; } // y is the smallest (y < x, or x >= z > y)
        else { a = z; b = x; c = y; }
    }
    ta[f] = a; tb[f] = b; tc[f] = c;
    sort_key[f] = c;
    ids[f] = (uint32_t)f;
}

__global__ void __launch_bounds__(256) unique_kernel(int V, int F, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb,
                                                      const uint32_t *__restrict__ sc, const uint32_t *__restrict__ sid, uint8_t *__restrict__ keep_out,
                                                      unsigned long long *counts)
{
    __shared__ uint32_t red[4][2];
    const int j = blockIdx.x * 256 + threadIdx.x;
    uint32_t n[2] = {0u, 0u}; // duplicates, flaps
    if (j < F)
    {
        const uint32_t a = sa[j], b = sb[j], c = sc[j], f = sid[j];
        bool keep = false;
        if (a < (uint32_t)V)
        {
            const bool dup = j > 0 && sa[j - 1] == a && sb[j - 1] == b && sc[j - 1] == c;
            keep = !dup;
            n[0] = dup;
            if (keep)
            {
                int lo = 0, hi = F; // the first position whose triple is not below (a, c, b): at most 31 halvings
                while (lo < hi)
                {
                    const int m = lo + ((hi - lo) >> 1);
                    const uint32_t ma = sa[m], mb = sb[m];
                    if (ma < a || (ma == a && (mb < c || (mb == c && sc[m] < b)))) lo = m + 1;
                    else hi = m;
                }
                n[1] = lo < F && sa[lo] == a && sb[lo] == c && sc[lo] == b;
            }
        }
        keep_out[f] = keep ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 2; k++)
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n[k] += __shfl_xor(n[k], o);
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = n[0]; red[threadIdx.x >> 6][1] = n[1]; }
    __syncthreads();
    if (threadIdx.x < 2)
    {
        const uint32_t t = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (t) __hip_atomic_fetch_add(counts + threadIdx.x, (unsigned long long)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------
struct LabelCarve
{
    uint32_t *key_lo, *key_hi, *k[2], *v[2];
    void *scratch;
    size_t bytes;
};
LabelCarve label_carve(void *ws, size_t V)
{
    LabelCarve c;
    Carver w(ws);
    c.key_lo = w.words(V); c.key_hi = w.words(V);
    c.k[0] = w.words(V); c.k[1] = w.words(V); c.v[0] = w.words(V); c.v[1] = w.words(V);
    c.scratch = w.bytes(sort_scratch_bytes(V));
    c.bytes = w.used();
    return c;
}

struct PlaceCarve
{
    uint32_t *bounds; // mstart, mend, fstart, fend: 4 x V words, cleared in one go
    uint32_t *mk[2], *mv[2], *fk[2], *fv[2];
    void *scratch;
    size_t bytes;
};
PlaceCarve place_carve(void *ws, size_t V, size_t F)
{
    PlaceCarve c;
    Carver w(ws);
    c.bounds = w.words(4 * V);
    c.mk[0] = w.words(V); c.mk[1] = w.words(V); c.mv[0] = w.words(V); c.mv[1] = w.words(V);
    c.fk[0] = w.words(3 * F); c.fk[1] = w.words(3 * F); c.fv[0] = w.words(3 * F); c.fv[1] = w.words(3 * F);
    c.scratch = w.bytes(std::max(sort_scratch_bytes(V), sort_scratch_bytes(3 * F)));
    c.bytes = w.used();
    return c;
}

struct UniqueCarve
{
    uint32_t *ta, *tb, *tc, *k[2], *v[2], *extra;
    void *scratch;
    size_t bytes;
};
UniqueCarve unique_carve(void *ws, size_t F)
{
    UniqueCarve c;
    Carver w(ws);
    c.ta = w.words(F); c.tb = w.words(F); c.tc = w.words(F);
    c.k[0] = w.words(F); c.k[1] = w.words(F); c.v[0] = w.words(F); c.v[1] = w.words(F);
    c.extra = w.words(F);
    c.scratch = w.bytes(sort_scratch_bytes(F));
    c.bytes = w.used();
    return c;
}
} // namespace

size_t ts_simplify_workspace_bytes(int V, int F)
{
    const size_t v = (size_t)(V > 0 ? V : 0), f = (size_t)(F > 0 ? F : 0);
    return std::max(label_carve(nullptr, v).bytes, std::max(place_carve(nullptr, v, f).bytes, unique_carve(nullptr, f).bytes)) + 2 * TS_ALIGN;
}

hipError_t ts_simplify_labels(int V, const float *vertices, float ox, float oy, float oz, float cell, int32_t *label, void *ws, hipStream_t s)
{
    if (V <= 0) return hipSuccess;
    const size_t n = (size_t)V;
    const LabelCarve c = label_carve(ws, n);
    hipLaunchKernelGGL(cell_keys_kernel, dim3(blocks256(n)), dim3(256), 0, s, V, vertices, ox, oy, oz, cell, c.key_lo, c.key_hi, c.k[0], c.v[0]);
    const int at = ts_radix_sort_pairs(c.k, c.v, n, 32, c.scratch, s); // by the low word, stable
    uint32_t *const k2[2] = {c.k[at ^ 1], c.k[at]}, *const v2[2] = {c.v[at], c.v[at ^ 1]};
    hipLaunchKernelGGL(gather_kernel, dim3(blocks256(n)), dim3(256), 0, s, n, c.key_hi, v2[0], k2[0]);
    const int at2 = ts_radix_sort_pairs(k2, v2, n, 32, c.scratch, s); // then by the high word (the invalid flag included), stable: (key, index) order
    const uint32_t *shi = k2[at2], *sid = v2[at2];
    uint32_t *slo = k2[at2 ^ 1]; // the partner of the sorted high words is free now
    hipLaunchKernelGGL(gather_kernel, dim3(blocks256(n)), dim3(256), 0, s, n, c.key_lo, sid, slo);
    hipLaunchKernelGGL(run_head_label_kernel, dim3(blocks256(n)), dim3(256), 0, s, V, shi, slo, sid, label);
    return hipGetLastError();
}

hipError_t ts_simplify_place(int V, int F, const float *vertices, const int32_t *faces, const int32_t *remap, float ox, float oy, float oz, float cell,
                             float lambda, int mode, const float *attributes, const uint8_t *attr_valid, int C, float *out_vertices,
                             float *out_attributes, uint8_t *out_valid, int32_t *member_count, void *ws, hipStream_t s)
{
    if (V <= 0) return hipSuccess;
    const size_t n = (size_t)V, f = (size_t)(F > 0 ? F : 0);
    const PlaceCarve c = place_carve(ws, n, f);
    hipError_t e = mesh_fill(c.bounds, 0, 4 * n * sizeof(uint32_t), s); // a rank without a run: start == end == 0
    if (e != hipSuccess) return e;
    uint32_t *mstart = c.bounds, *mend = c.bounds + n, *fstart = c.bounds + 2 * n, *fend = c.bounds + 3 * n;
    hipLaunchKernelGGL(member_keys_kernel, dim3(blocks256(n)), dim3(256), 0, s, V, remap, c.mk[0], c.mv[0]);
    const int at = ts_radix_sort_pairs(c.mk, c.mv, n, bit_length((uint32_t)(V - 1)), c.scratch, s); // stable: a cluster's members ascending
    hipLaunchKernelGGL(run_bounds_kernel, dim3(blocks256(n)), dim3(256), 0, s, n, c.mk[at], (uint32_t)V, mstart, mend);
    int fat = 0;
    if (f > 0 && mode == 1)
    {
        hipLaunchKernelGGL(incidence_kernel, dim3(blocks256(f)), dim3(256), 0, s, V, F, vertices, faces, remap, ox, oy, oz, cell, c.fk[0], c.fv[0]);
        fat = ts_radix_sort_pairs(c.fk, c.fv, 3 * f, bit_length((uint32_t)V), c.scratch, s); // the sentinel V included; stable: a cluster's faces ascending
        hipLaunchKernelGGL(run_bounds_kernel, dim3(blocks256(3 * f)), dim3(256), 0, s, 3 * f, c.fk[fat], (uint32_t)V, fstart, fend);
    }
    PlaceArgs a;
    a.vertices = vertices; a.faces = faces; a.attributes = attributes; a.attr_valid = attr_valid;
    a.mids = c.mv[at]; a.mstart = mstart; a.mend = mend; a.fval = c.fv[fat]; a.fstart = fstart; a.fend = fend;
    a.out_vertices = out_vertices; a.out_attributes = out_attributes; a.out_valid = out_valid; a.member_count = member_count;
    a.ox = ox; a.oy = oy; a.oz = oz; a.cell = cell; a.lambda = lambda;
    a.V = V; a.F = (int)f; a.mode = mode; a.C = attributes ? C : 0;
    hipLaunchKernelGGL(place_kernel, dim3(blocks256(n)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t ts_simplify_unique_faces(int V, int F, const int32_t *faces, const uint8_t *keep_in, uint8_t *keep_out, unsigned long long *counts,
                                    void *ws, hipStream_t s)
{
    hipError_t e = mesh_fill(counts, 0, 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    if (F <= 0) return hipSuccess;
    const size_t n = (size_t)F;
    const UniqueCarve c = unique_carve(ws, n);
    const int bits = bit_length((uint32_t)(V > 0 ? V : 0)); // the sentinel V included
    hipLaunchKernelGGL(rotated_triples_kernel, dim3(blocks256(n)), dim3(256), 0, s, V, F, faces, keep_in, c.ta, c.tb, c.tc, c.k[0], c.v[0]);
    const int at = ts_radix_sort_pairs(c.k, c.v, n, bits, c.scratch, s); // by c
    uint32_t *const k2[2] = {c.k[at ^ 1], c.k[at]}, *const v2[2] = {c.v[at], c.v[at ^ 1]};
    hipLaunchKernelGGL(gather_kernel, dim3(blocks256(n)), dim3(256), 0, s, n, c.tb, v2[0], k2[0]);
    const int at2 = ts_radix_sort_pairs(k2, v2, n, bits, c.scratch, s); // then by b
    uint32_t *const k3[2] = {k2[at2 ^ 1], k2[at2]}, *const v3[2] = {v2[at2], v2[at2 ^ 1]};
    hipLaunchKernelGGL(gather_kernel, dim3(blocks256(n)), dim3(256), 0, s, n, c.ta, v3[0], k3[0]);
    const int at3 = ts_radix_sort_pairs(k3, v3, n, bits, c.scratch, s); // then by a: (a, b, c, face) order
    const uint32_t *sa = k3[at3], *sid = v3[at3];
    uint32_t *sb = k3[at3 ^ 1], *sc = c.extra;
    hipLaunchKernelGGL(gather_kernel, dim3(blocks256(n)), dim3(256), 0, s, n, c.tb, sid, sb);
    hipLaunchKernelGGL(gather_kernel, dim3(blocks256(n)), dim3(256), 0, s, n, c.tc, sid, sc);
    hipLaunchKernelGGL(unique_kernel, dim3(blocks256(n)), dim3(256), 0, s, V, F, sa, sb, sc, sid, keep_out, counts);
    return hipGetLastError();
}
