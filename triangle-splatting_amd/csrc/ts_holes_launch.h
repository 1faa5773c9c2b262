// ts_holes_launch.h -- the launchers of mesh_holes.hip as api_holes.hip calls them (include/ts_holes.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_holes_workspace_bytes(int V, int F);
hipError_t ts_holes_loops(int V, int F, const int32_t *faces, const uint8_t *keep, const int32_t *offsets, const int32_t *neighbors,
                          const int32_t *edge_faces, int num_entries, int32_t *half_edge_loop, int32_t *loop_offsets, int32_t *loop_half_edges,
                          unsigned long long *counts, void *ws, hipStream_t s);
hipError_t ts_holes_fill(int V, int F, const float *vertices, const int32_t *faces, int num_loops, const int32_t *loop_offsets,
                         const int32_t *loop_half_edges, int num_members, int max_loop_edges, const float *attributes, const uint8_t *attr_valid,
                         int channels, uint8_t *loop_status, float *new_vertices, float *new_attributes, uint8_t *new_attr_valid,
                         int32_t *new_faces, int32_t *new_face_loop, unsigned long long *totals, void *ws, hipStream_t s);
