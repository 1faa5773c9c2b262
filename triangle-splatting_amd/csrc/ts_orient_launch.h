// ts_orient_launch.h -- the launchers of mesh_orient.hip as api_orient.hip calls them (include/ts_orient.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_orient_workspace_bytes(int V, int F);
hipError_t ts_orient_faces(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, int mode, int32_t *face_piece,
                           uint8_t *face_flip, int32_t *out_faces, unsigned long long *counts, void *ws, hipStream_t s);
