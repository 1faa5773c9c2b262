// ts_manifold_launch.h -- the launchers of mesh_manifold.hip as api_manifold.hip calls them (include/ts_manifold.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_manifold_workspace_bytes(int V, int F);
hipError_t ts_manifold_fans(int V, int F, const int32_t *faces, const uint8_t *keep, int32_t *corner_fan, int32_t *vertex_fans,
                            unsigned long long *counts, void *ws, hipStream_t s);
hipError_t ts_manifold_split(int V, int F, const int32_t *faces, const uint8_t *keep, const int32_t *corner_fan, int capacity, int32_t *out_faces,
                             int32_t *new_vertex_source, int32_t *new_vertex_fan, unsigned long long *totals, void *ws, hipStream_t s);
