// ts_subdivide_launch.h -- the launchers of mesh_subdivide.hip as api_subdivide.hip calls them (include/ts_subdivide.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_subdivide_workspace_bytes(int V, int F);
hipError_t ts_subdivide_edges(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, int32_t *edge_vertices,
                              int32_t *edge_use, double *edge_length2, int32_t *half_edge_edge, unsigned long long *counts, void *ws,
                              hipStream_t s);
hipError_t ts_subdivide_split(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, int mode, float max_edge,
                              const float *vertex_limit, const float *attributes, const uint8_t *attr_valid, int channels, float *new_vertices,
                              float *new_attributes, uint8_t *new_attr_valid, int32_t *new_vertex_edge, int32_t *out_faces,
                              int32_t *out_face_parent, unsigned long long *totals, void *ws, hipStream_t s);
