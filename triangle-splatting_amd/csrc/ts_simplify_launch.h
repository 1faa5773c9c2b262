// ts_simplify_launch.h -- the launchers of mesh_simplify.hip as api_simplify.hip calls them (include/ts_simplify.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_simplify_workspace_bytes(int V, int F);
hipError_t ts_simplify_labels(int V, const float *vertices, float ox, float oy, float oz, float cell, int32_t *label, void *ws, hipStream_t s);
hipError_t ts_simplify_place(int V, int F, const float *vertices, const int32_t *faces, const int32_t *remap, float ox, float oy, float oz, float cell,
                             float lambda, int mode, const float *attributes, const uint8_t *attr_valid, int C, float *out_vertices,
                             float *out_attributes, uint8_t *out_valid, int32_t *member_count, void *ws, hipStream_t s);
hipError_t ts_simplify_unique_faces(int V, int F, const int32_t *faces, const uint8_t *keep_in, uint8_t *keep_out, unsigned long long *counts,
                                    void *ws, hipStream_t s);
