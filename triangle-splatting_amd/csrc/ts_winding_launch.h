// ts_winding_launch.h -- the launchers of mesh_winding.hip as api_winding.hip calls them (include/ts_winding.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_winding_bvh_bytes(int F); // the index size of F faces, from csrc/ts_bvh_layout.h: what the size query of include/ts_bvh.h answers
size_t ts_winding_moments_bytes(int F);
size_t ts_winding_leaf_faces_bytes(int F);
size_t ts_winding_workspace_bytes(int Q);
hipError_t ts_winding_moments(int F, const void *bvh, double *moments, int32_t *leaf_faces, hipStream_t s);
hipError_t ts_winding_query(int Q, const float *points, double beta2, int F, const void *bvh, const double *moments, int64_t *wq, int32_t *terms,
                            void *ws, hipStream_t s);
hipError_t ts_winding_sign_distance(int Q, const double *dist2, const int64_t *wq, int64_t threshold, float *out, uint8_t *decided, hipStream_t s);
