// ts_inside_launch.h -- the launchers of mesh_inside.hip as api_inside.hip calls them (include/ts_inside.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_inside_bvh_bytes(int F); // the index size of F faces, from csrc/ts_bvh_layout.h: what the size query of include/ts_bvh.h answers
size_t ts_inside_crossings_workspace_bytes(int Q);
hipError_t ts_inside_crossings(int Q, const float *origins, const float *directions, int shared_direction, const float *t_limit, double tmin,
                               double tmax, int F, const void *bvh, int32_t *hits, int32_t *winding2, int32_t *touches,
                               unsigned long long *leaf_visits, void *ws, hipStream_t s);
hipError_t ts_inside_signed_distance(int Q, const double *dist2, const int32_t *winding2, const int32_t *touches, const int32_t *hits, int rule,
                                     int only_undecided, float *out, uint8_t *decided, hipStream_t s);
