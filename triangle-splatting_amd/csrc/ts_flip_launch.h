// ts_flip_launch.h -- the launchers of mesh_flip.hip as api_flip.hip calls them (include/ts_flip.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_flip_workspace_bytes(int V, int F);
hipError_t ts_flip_round(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, float min_cos, uint32_t seed,
                         int32_t *out_faces, uint8_t *face_flipped, int32_t *edge_vertices, uint8_t *edge_state, int32_t *edge_opposite,
                         unsigned long long *totals, void *ws, hipStream_t s);
