// ts_mesh_runs.h -- the bounds of the runs of a sorted key column, for the units that walk one run per thread (mesh_simplify.hip: a
// cluster's members and faces; mesh_smooth.hip: a vertex's faces).  A header of its own, because a kernel is emitted into every unit that
// includes its definition.
#pragma once
#include "ts_mesh_common.h"

namespace
{
// keys ascending: the head of the run of key k writes start[k], its tail end[k] (one past); keys >= limit (the sentinel) write nothing
__global__ void __launch_bounds__(256) run_bounds_kernel(size_t n, const uint32_t *__restrict__ keys, uint32_t limit, uint32_t *__restrict__ start,
                                                          uint32_t *__restrict__ end)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t k = keys[j];
    if (k >= limit) return;
    if (j == 0 || keys[j - 1] != k) start[k] = (uint32_t)j;
    if (j + 1 == n || keys[j + 1] != k) end[k] = (uint32_t)(j + 1);
}
} // namespace
