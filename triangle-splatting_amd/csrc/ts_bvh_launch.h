// ts_bvh_launch.h -- the launchers of mesh_bvh.hip as api_bvh.hip calls them (include/ts_bvh.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_bvh_bytes(int F);
size_t ts_bvh_build_workspace_bytes(int F);
hipError_t ts_bvh_build(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, void *bvh, void *ws, hipStream_t s);
size_t ts_bvh_closest_workspace_bytes(int Q);
hipError_t ts_bvh_closest(int Q, const float *queries, int F, const void *bvh, int32_t *face, double *dist2, float *point,
                          unsigned long long *leaf_visits, void *ws, hipStream_t s);
