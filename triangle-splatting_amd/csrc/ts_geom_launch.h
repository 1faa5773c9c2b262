// ts_geom_launch.h -- the launchers of mesh_distance.hip as api_geom.hip calls them (include/ts_geom.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_geom_cross_workspace_bytes(int Q, int R);
hipError_t ts_geom_nearest_cross(int Q, const float *queries, int R, const float *refs, int32_t *nearest, float *dist2,
                                 unsigned long long *box_visits, void *ws, hipStream_t s);
size_t ts_geom_sample_workspace_bytes(int F);
hipError_t ts_geom_face_areas(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, double *area, hipStream_t s);
hipError_t ts_geom_sample_surface(int V, int F, const float *vertices, const int32_t *faces, const double *area, int N, uint64_t seed,
                                  float *points, int32_t *face, void *ws, hipStream_t s);
