// ts_collapse_launch.h -- the launchers of mesh_collapse.hip as api_collapse.hip calls them (include/ts_collapse.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_collapse_workspace_bytes(int V, int F);
hipError_t ts_collapse_round(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, const uint8_t *pinned, int mode,
                             float min_edge, const float *vertex_limit, float max_edge, float min_cos, uint32_t seed, int32_t *out_faces,
                             uint8_t *out_keep, int32_t *vertex_target, int32_t *edge_vertices, uint8_t *edge_state, int32_t *edge_removed,
                             uint8_t *edge_guard, unsigned long long *totals, void *ws, hipStream_t s);
