// ts_ray_launch.h -- the launchers of mesh_ray.hip as api_ray.hip calls them (include/ts_ray.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_ray_bvh_bytes(int F); // the index size of F faces, from csrc/ts_bvh_layout.h: what the size query of include/ts_bvh.h answers
size_t ts_ray_cast_workspace_bytes(int Q);
hipError_t ts_ray_cast(int Q, const float *origins, const float *directions, const float *t_limit, double tmin, double tmax, int cull_back, int F,
                       const void *bvh, int32_t *face, double *t, float *bary, int8_t *side, unsigned long long *leaf_visits, void *ws, hipStream_t s);
