// ts_weld_launch.h -- the launchers of mesh_weld.hip as api.hip calls them (include/ts_weld.h is the C ABI over them).  Kept out of
// ts2d_common.h: no other unit needs them, and a declaration added there would rebuild every unit of the library.
#pragma once
#include "ts2d_common.h"
size_t ts_weld_workspace_bytes(int V, int F);
hipError_t ts_weld_labels(int V, const float *vertices, float eps, uint32_t *label, unsigned long long *box_visits, void *ws, hipStream_t s);
hipError_t ts_weld_face_components(int V, int F, const int32_t *faces, const uint8_t *keep, uint32_t *label, hipStream_t s);
hipError_t ts_weld_compact(int V, const uint32_t *label, const float *vertices, int mode, int32_t *remap, float *out_vertices, int32_t *count,
                           void *ws, hipStream_t s);
hipError_t ts_weld_remap_faces(int V, int F, const int32_t *faces, const int32_t *remap, int32_t *out_faces, uint8_t *keep, hipStream_t s);
hipError_t ts_weld_edge_census(int V, int F, const int32_t *faces, const uint8_t *keep, unsigned long long *counts, void *ws, hipStream_t s);
