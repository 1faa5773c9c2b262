// ts_bvh_walk.h -- the walk of the triangle index (csrc/ts_bvh_layout.h), once, for three of the four queries that walk it: closest_kernel
// (mesh_bvh.hip), crossings_kernel (mesh_inside.hip) and winding_kernel (mesh_winding.hip).  cast_kernel (mesh_ray.hip) keeps a walk of its
// own, the text this header was made from, because it measured slower on this one; what changes here changes there.  Templates
// over the kernels' own callables, inlined into each kernel: there is no call and no pointer to a function.  Every translation unit that
// includes it gets its own internal copy.
//
// One wave owns 64 consecutive sorted queries, one per lane, and a stack of its own in LDS.  Control flow is wave-uniform: the wave pops a
// node, loads its box (the same words for every lane), skips it when no eligible face lies below, and asks the kernel's `enter` whether some
// lane needs it -- the kernel's own __ballot, on the kernel's own test.  An entered leaf goes to the kernel's `leaf`; an entered inner node
// pushes its children by one of two policies, a compile-time choice:
//   index order    (crossings_kernel, winding_kernel: sums, nothing to prune on)  the last child first, so that pops come in index order,
//                  the order of the leaves in memory; the children's boxes are not read
//   nearest first  (closest_kernel: a best-so-far to prune on)  the non-empty children's boxes are loaded, `child_key` gives a
//                  float per child, and the one with the largest key is pushed first (ties: the highest index first), so that the nearest
//                  is popped first.  The keys order the work; the result does not depend on them.
//
// Stack entry.  (level << 28) | k: node k of level `level`.  k < 2^28 (at most 2^28 leaves) and level < MAX_LEVELS = 11 < 16.  k < the
// level's node count by construction: the root is (top, 0), and a child index is bounded by the count of the level below.
//
// Stack bound.  There are at most MAX_LEVELS = 11 levels (ts_bvh_layout.h).  A pop removes one entry and pushes at most FAN children of the
// level below; leaves push nothing.  By induction the stack holds at most 1 + (FAN - 1) entries per inner level on the current path:
// STACK = 1 + (FAN - 1) (MAX_LEVELS - 1) = 71, whatever the data.  So `sp < STACK` in walk_push is always true; the test costs nothing and
// keeps a wrong proof inside its own memory.
#pragma once
#include "ts_bvh_layout.h"

#include <algorithm>

namespace
{
constexpr int WAVES = TPB / 64;

// the workspace of a query's front half (knn_carve).  The radix sort's tables shrink where its chunk length grows (TS_RS_SMALL_BELOW):
// never less than just below that size
size_t query_carve_bytes(int n)
{
    const size_t b = knn_carve(nullptr, n).bytes;
    return n > TS_RS_SMALL_BELOW ? std::max(b, knn_carve(nullptr, TS_RS_SMALL_BELOW).bytes) : b;
}

// what a walking kernel keeps in LDS: the level table and one stack per wave
struct WalkShared
{
    uint32_t lvl_off[MAX_LEVELS], lvl_cnt[MAX_LEVELS];
    uint32_t stack[WAVES][STACK];
};

// the level table follows from the leaf count alone (bvh_view).  Holds the kernel's only barrier: from here on every wave is on its own
__device__ __forceinline__ void walk_levels(WalkShared &ws, int nleaves)
{
    const int tid = threadIdx.x;
    if (tid < MAX_LEVELS)
    {
        uint32_t off = 0, cnt = (uint32_t)nleaves;
        for (int l = 0; l < tid; l++)
        {
            off += cnt;
            cnt = (cnt + FAN - 1) >> FAN_SHIFT;
        }
        ws.lvl_off[tid] = off; ws.lvl_cnt[tid] = cnt;
    }
    __syncthreads();
}

// this lane's query of the float4 array that knn_prepare<true> wrote: the point, its original index (< Q for a lane inside), and whether
// it is finite (a non-finite one was stored as NaNs).  A lane outside Q gets NaNs
struct WalkQuery
{
    float4 p;
    uint32_t pid;
    bool inside, live;
};

__device__ __forceinline__ WalkQuery walk_query(int Q, const float4 *__restrict__ qsp)
{
    const float nanf_ = __uint_as_float(0x7FC00000u);
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    WalkQuery q;
    q.inside = i < (size_t)Q;
    q.p = q.inside ? qsp[i] : make_float4(nanf_, nanf_, nanf_, 0.0f);
    q.pid = __float_as_uint(q.p.w);
    q.live = q.inside && q.p.x == q.p.x;
    return q;
}

// face(id, ax, ay, az, bx, by, bz, cx, cy, cz) for every eligible slot of a leaf; the words are wave-uniform loads
template <class Face>
__device__ __forceinline__ void for_each_face(const Leaf &lf, Face face)
{
#pragma unroll 1
    for (int j = 0; j < LEAF; j++)
    {
        const int32_t id = lf.id[j];
        if (id < 0) continue; // wave-uniform: an ineligible or padding slot
        face(id, lf.v[j][0], lf.v[j][1], lf.v[j][2], lf.v[j][3], lf.v[j][4], lf.v[j][5], lf.v[j][6], lf.v[j][7], lf.v[j][8]);
    }
}

__device__ __forceinline__ void walk_push(uint32_t *st, int &sp, int level, uint32_t k)
{
    if (sp < STACK) st[sp++] = ((uint32_t)level << 28) | k;
}

// the child key of a walk in index order: never called
struct NoChildKey
{
    __device__ float operator()(const Box &) const { return 0.0f; }
};

// enter(level, k, at, box) -> wave-uniform bool: the popped node k of `level`, `at` its index across all levels, its non-empty box
// leaf(k): an entered node of level 0
// child_key(box) -> float, NEAREST_FIRST only: the order of a non-empty child, smallest first
template <bool NEAREST_FIRST, class Enter, class LeafFn, class ChildKey>
__device__ __forceinline__ void bvh_walk(WalkShared &ws, int nlevels, const Box *__restrict__ nodes, Enter enter, LeafFn leaf, ChildKey child_key)
{
    uint32_t *st = ws.stack[threadIdx.x >> 6];
    int sp = 0;
    walk_push(st, sp, nlevels - 1, 0u); // the root: node 0 of the top level
    while (sp > 0)
    {
        const uint32_t e = __builtin_amdgcn_readfirstlane(st[--sp]);
        const int level = (int)(e >> 28);
        const uint32_t k = e & 0x0FFFFFFFu;
        const uint32_t at = __builtin_amdgcn_readfirstlane(ws.lvl_off[level] + k);
        const Box b = nodes[at];
        if (b.mnx > b.mxx) continue; // no eligible face below
        if (!enter(level, k, at, b)) continue;
        if (level == 0)
        {
            leaf((int)k);
            continue;
        }
        const uint32_t c0 = k * FAN, below = __builtin_amdgcn_readfirstlane(ws.lvl_cnt[level - 1]);
        const int nchild = (int)min(below - c0, (uint32_t)FAN); // c0 < below: k < ceil(below / FAN)
        if (!NEAREST_FIRST)
        {
            for (int c = nchild - 1; c >= 0; c--) walk_push(st, sp, level - 1, c0 + (uint32_t)c);
            continue;
        }
        const uint32_t base = __builtin_amdgcn_readfirstlane(ws.lvl_off[level - 1]) + c0;
        float key[FAN];
        unsigned want = 0;
#pragma unroll
        for (int c = 0; c < FAN; c++)
        {
            key[c] = 0.0f;
            if (c < nchild)
            {
                const Box cb = nodes[base + c];
                if (!(cb.mnx > cb.mxx))
                {
                    key[c] = child_key(cb);
                    want |= 1u << c;
                }
            }
        }
        while (want) // at most FAN pushes
        {
            int far = -1;
            float far_key = 0.0f;
#pragma unroll
            for (int c = 0; c < FAN; c++)
                if (((want >> c) & 1u) && (far < 0 || key[c] >= far_key)) { far = c; far_key = key[c]; }
            want &= ~(1u << far);
            walk_push(st, sp, level - 1, c0 + (uint32_t)far);
        }
    }
}
} // namespace
