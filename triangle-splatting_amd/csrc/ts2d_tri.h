// ts2d_tri.h -- per-triangle geometry shared by the model-update rules (model_update.hip) and the trainer's regularisers
// (regularizers.hip), so that the mean side length a split / prune rule compares with a threshold and the one scaling_reg averages cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

// |a - b| as torch's GPU norm over the last dimension of three forms it: (x^2 + z^2) + y^2, no contraction, correctly rounded square root
__device__ __forceinline__ float side_len(const float *a, const float *b)
{
#pragma clang fp contract(off)
    const float x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return sqrtf((x * x + z * z) + y * y);
}
// get_scaling (VanillaTS_model.py:72-76): mean side length, sides in the order (v3 - v2, v1 - v3, v2 - v1).  Side lengths and mean are formed
// the way torch's GPU norm and mean over three elements form them -- the mean as (l1 + l3) + l2, times float(1/3) -- so that a triangle whose
// mean side lies on a threshold, or whose sides tie, is decided as in the reference (tests/test_model_ops_gpu.py)
__device__ __forceinline__ float mean_side(const float *v, float &l1, float &l2, float &l3)
{
    l1 = side_len(v + 6, v + 3);
    l2 = side_len(v + 0, v + 6);
    l3 = side_len(v + 3, v + 0);
    return ((l1 + l3) + l2) * (1.0f / 3.0f);
}
