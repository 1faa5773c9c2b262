// ts_atlas_launch.h -- the launchers of mesh_atlas.hip as api_atlas.hip calls them (include/ts_atlas.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
hipError_t ts_atlas_texel_index(const float *view, float tan_fovx, float tan_fovy, int W, int H, int V, const float *vertices, int F,
                                const int32_t *faces, const int32_t *face_idx, int R, int Cx, int32_t *texel_idx, int32_t *atlas_idx, float *bary,
                                hipStream_t s);
hipError_t ts_atlas_face_totals(int F, int R, const unsigned long long *texels, unsigned long long *face_totals, hipStream_t s);
hipError_t ts_atlas_resolve(int F, int R, int Cx, int Cy, const unsigned long long *texels, const unsigned long long *face_totals, int min_count,
                            const float *face_fallback, float fill_r, float fill_g, float fill_b, float *image, uint8_t *state, uint8_t *rgb8,
                            hipStream_t s);
hipError_t ts_atlas_render(int W, int H, int Wa, int Ha, const int32_t *atlas_idx, const float *image, const float *background, float *out,
                           hipStream_t s);
