// ts_smooth_launch.h -- the launchers of mesh_smooth.hip as api_smooth.hip calls them (include/ts_smooth.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_smooth_workspace_bytes(int V, int F);
hipError_t ts_smooth_adjacency(int V, int F, const int32_t *faces, const uint8_t *keep, int32_t *offsets, int32_t *neighbors, int32_t *edge_faces,
                               uint8_t *vertex_class, unsigned long long *counts, void *ws, hipStream_t s);
hipError_t ts_smooth_smooth(int V, const float *vertices, const int32_t *offsets, const int32_t *neighbors, const int32_t *edge_faces, int num_entries,
                            const uint8_t *vertex_class, const uint8_t *pinned, float lambda, float mu, int iterations, int boundary_mode,
                            float max_move, float *out_vertices, void *ws, hipStream_t s);
hipError_t ts_smooth_face_normals(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, float *face_normal,
                                  uint8_t *face_valid, hipStream_t s);
hipError_t ts_smooth_vertex_normals(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, int weighting,
                                    float *vertex_normal, uint8_t *vertex_valid, double *normal_sum, void *ws, hipStream_t s);
