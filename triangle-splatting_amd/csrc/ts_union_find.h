// ts_union_find.h -- the lock-free union-find of mesh_weld.hip (vertex clusters, face components) and mesh_manifold.hip (the fans of a
// vertex), single-sourced.  Device code only; every unit that includes it gets its own copy (internal linkage).
//
// Union-find (uf_find / uf_union).  parent[x] <= x at all times; parent starts as the identity.
//   * a root only ever changes by atomicCAS(&parent[big], big, small) with small < big, a non-root only by atomicMin (path halving): the
//     words only decrease, a non-root never becomes a root again, and parent[x] always names an ancestor of x;
//   * hooking the larger root under the smaller keeps every root the smallest index of its tree, so the final roots do not depend on the
//     order of the unions: the labels are a pure function of the relation;
//   * every word is read and written with agent-scope atomics (the per-CU L1 is never consulted); a value that is out of date is still an
//     ancestor, so it costs steps, not correctness.  No lane ever waits for another: there is no spinning anywhere.
//   Termination.  uf_find: x strictly decreases with every step (parent[x] < x for a non-root) and is bounded below by 0.  uf_union: a
//   failed CAS returns the word's value, which is < big, and the two finds that follow only move down: a + b strictly decreases with every
//   failed attempt and is bounded below by 0; a successful CAS or a == b ends the loop.
//   The flatten (label[i] = root(i)) is a launch of its own after all unions.
#pragma once
#include "ts2d_common.h"

namespace
{
// ---- union-find ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t uf_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x.  Terminates: every step replaces x by parent[x] < x.  With `shorten`, a non-root whose grandparent lies below its parent is
// pointed at the grandparent by atomicMin (safe beside concurrent unions: the word only decreases and still names an ancestor).
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x, bool shorten)
{
    for (;;)
    {
        const uint32_t p = uf_load(parent + x);
        if (p == x) return x;
        if (shorten)
        {
            const uint32_t g = uf_load(parent + p);
            if (g != p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        x = p;
    }
}

// Terminates: see the file header (a + b strictly decreases with every failed CAS).
__device__ __forceinline__ void uf_union(uint32_t *parent, uint32_t a, uint32_t b)
{
    a = uf_find(parent, a, true);
    b = uf_find(parent, b, true);
    while (a != b)
    {
        const uint32_t big = a > b ? a : b, small = a > b ? b : a;
        uint32_t seen = big;
        if (__hip_atomic_compare_exchange_strong(parent + big, &seen, small, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        a = uf_find(parent, seen, true); // seen < big: `big` had been hooked meanwhile
        b = uf_find(parent, small, true);
    }
}
} // namespace
