// ts_bvh_layout.h -- the layout of the triangle index that the build of mesh_bvh.hip writes (include/ts_bvh.h), as its readers see it: the
// closest-point query of mesh_bvh.hip, the ray query of mesh_ray.hip (include/ts_ray.h), the crossing counts of mesh_inside.hip
// (include/ts_inside.h), the winding number of mesh_winding.hip (include/ts_winding.h), the overlap query of mesh_overlap.hip
// (include/ts_overlap.h), whose queries are the leaves of a second index or of the same one, each a library of its own, and the moments
// pass of mesh_winding.hip, which writes one record per node beside it.  Four of the queries walk it with csrc/ts_bvh_walk.h, cast_kernel
// with a walk of its own.  Every translation unit that includes it gets its own internal copy.
//
// Leaves of LEAF consecutive Morton-sorted faces with their nine fp32 coordinates gathered (slot id -1: ineligible or padding, never
// evaluated); above them an IMPLICIT tree of fan-out FAN: node k of level l covers the leaves [k FAN^l, (k+1) FAN^l), level 0 being the
// leaves' own boxes.  A node without an eligible face has the empty box (+inf, -inf).  The layout is made of offsets from `bvh` alone and
// follows from F; a query takes every index it follows from F, never from memory.
//
// F <= 2^31 - 1 gives at most 2^28 leaves, so at most MAX_LEVELS = 11 levels (2^28, 2^25, ..., 2, 1 nodes).  STACK is what a depth-first
// walk of that tree holds at most, whatever the data: the argument stands beside the push, in ts_bvh_walk.h.
#pragma once
#include "ts_knn_front.h"

namespace
{
constexpr int LEAF = 8, FAN = 8, FAN_SHIFT = 3;
constexpr int MAX_LEVELS = 11;
constexpr int STACK = 1 + (FAN - 1) * (MAX_LEVELS - 1);

struct Leaf
{
    float v[LEAF][9];
    int32_t id[LEAF];
};

struct BvhView
{
    Box *bbox;       // of the eligible centroids
    uint32_t *codes; // F sorted codes
    Leaf *leaves;    // nleaves
    Box *nodes;      // every level, level 0 (the leaves' boxes) first
    int nleaves, nlevels;
    int count[MAX_LEVELS];
    size_t offset[MAX_LEVELS]; // of a level's first node in `nodes`
    size_t bytes;
};

BvhView bvh_view(void *base, int F)
{
    BvhView v;
    const size_t n = (size_t)(F > 0 ? F : 0);
    v.nleaves = (int)((n + LEAF - 1) / LEAF);
    v.nlevels = 0;
    size_t total = 0;
    for (int c = v.nleaves; c > 0; c = (c + FAN - 1) >> FAN_SHIFT)
    {
        v.count[v.nlevels] = c;
        v.offset[v.nlevels] = total;
        total += (size_t)c;
        v.nlevels++;
        if (c == 1) break;
    }
    char *p = (char *)base;
    auto take = [&](size_t bytes) { char *q = p; p += ts_align_up(bytes); return q; };
    v.bbox = (Box *)take(sizeof(Box));
    v.codes = (uint32_t *)take(n * 4);
    v.leaves = (Leaf *)take((size_t)v.nleaves * sizeof(Leaf));
    v.nodes = (Box *)take(total * sizeof(Box));
    v.bytes = (size_t)(p - (char *)base);
    return v;
}
} // namespace
