// ts_color_launch.h -- the launchers of color_volume.hip as api_color.hip calls them (include/ts_color.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
hipError_t ts_color_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float h, float trunc, const float *view, float tan_fovx,
                              float tan_fovy, int W, int H, const float *depth, const uint8_t *mask, const float *image, long long *csum,
                              int32_t *cweight, unsigned long long *updated, hipStream_t s);
hipError_t ts_color_field(int n, const long long *csum, const int32_t *cweight, int min_weight, float *field, hipStream_t s);
hipError_t ts_color_sample(int nx, int ny, int nz, float ox, float oy, float oz, float h, int C, const float *grid, int N, const float *points,
                           float *out, uint8_t *valid, hipStream_t s);
hipError_t ts_color_interpolate(const float *view, float tan_fovx, float tan_fovy, int W, int H, int V, const float *vertices, int F,
                                const int32_t *faces, const int32_t *face_idx, int C, const float *attributes, const float *background, float *out,
                                float *bary, hipStream_t s);
