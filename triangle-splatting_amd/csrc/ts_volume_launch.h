// ts_volume_launch.h -- the launchers of volume.hip as api_volume.hip calls them (include/ts_volume.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
hipError_t ts_volume_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float h, float trunc, const float *view, float tan_fovx,
                               float tan_fovy, int W, int H, const float *depth, const uint8_t *mask, int carve, long long *sum, int32_t *weight,
                               unsigned long long *updated, hipStream_t s);
hipError_t ts_volume_field(int n, const long long *sum, const int32_t *weight, int min_weight, float *field, hipStream_t s);
size_t ts_volume_extract_workspace_bytes(size_t n);
hipError_t ts_volume_extract(int nx, int ny, int nz, float ox, float oy, float oz, float h, const float *field, float iso, long long capacity,
                             float *triangles, int32_t *cell, long long *total, void *ws, hipStream_t s);
