/*
 * ts_atlas.h -- C ABI of libts_atlas.so: a texture atlas for an indexed mesh, baked from views.  Every face carries R (R + 1) / 2 texels
 * of its own; the texel of a pixel follows from the barycentrics of ts_color.h's tsc_interpolate; the texels of many views are summed in
 * integers by ts_mesh.h's ts2d_mesh_census_add with the texel index as its key; the sums are resolved into one image in which two faces
 * share a cell of (R + 1) x R texels.  diff_recon_hip/mesh_texture.py builds atlas_layout, face_uvs, texel_index, TextureAtlas,
 * render_textured, bake_texture, evaluate_textured and save_glb_textured_mesh on it.
 *
 * A library of its own, the twelfth: the export lists of the other eleven are closed.  libts_atlas.so links no object of the others and
 * keeps its own error text.  The error codes are ts2d.h's.  The accumulator is NOT restated here: its Q16 rule, its mask rule and its
 * kernel are ts2d_mesh_census_add's (ts_mesh.h), called with `texel_idx` as the key image and F T as the row count.
 *
 * All pointers are device pointers, except `fill` (three host floats); everything is enqueued on `stream` (a hipStream_t); no call allocates
 * or synchronises with the host, so the calls can be captured in a graph; no call has a workspace.  Argument checks are decided before any HIP call: a negative V or F, an image
 * or atlas size below 1, R outside [1, 64], Cx < 1, Cx Cy < K, min_count < 1, a tangent that is NaN, infinite or not positive, or a null
 * required pointer return TS2D_ERR_INVALID with the text in the last-error call of this header.  F T > 2^31 - 1, Wa Ha > 2^31 - 1 or
 * W H > 2^31 - 1 is TS2D_ERR_CAPACITY.  F == 0 still writes `fill` or -1 everywhere.  The outputs overlap neither each other nor an input.
 * The unit is built with -ffp-contract=off.  Everything below that is not an integer is float64, computed from the fp32 inputs widened to
 * double, with every operation rounded.
 *
 * Texels per face.  R = the number of texels per face edge, 1 <= R <= 64, uniform over the mesh.  T = R (R + 1) / 2 texels per face.
 * Texel (f, i, j) exists for 0 <= j < R, 0 <= i < R - j; its compact index is n = f T + j R - j (j - 1) / 2 + i, a bijection onto [0, F T).
 *
 * Texel of a pixel (tsa_texel_index; one thread per pixel).  "Drawn", the view-space corners a, b, c, the ray r, the weights wa, wb, wc,
 * the sign flip, the clamp of negative or NaN weights, s' and (alpha, beta, gamma) are exactly tsc_interpolate's (ts_color.h,
 * "Interpolation of vertex attributes"), the 1.0 / 3.0 fallback included: both kernels are compiled from csrc/ts_mesh_bary.h.  Then
 *   i = (int) floor(beta R), clamped to R - 1;   j = (int) floor(gamma R), clamped to R - 1 - i.
 *   texel_idx[p] = n for a drawn pixel and -1 otherwise.
 * bary (optional, 3 H W floats, planar) is tsc_interpolate's: ((float)alpha, (float)beta, (float)gamma) on drawn pixels, 0 elsewhere.
 * Nothing is read out of bounds for any contents of face_idx or faces.
 *
 * Atlas.  K = ceil(F / 2) cells; cell k holds face 2 k as its lower triangle and face 2 k + 1 as its upper triangle.  Cx >= 1 cells per
 * row, Cy = max(1, ceil(K / Cx)) rows (tsa_texel_index derives Cy so; tsa_resolve takes any Cy with Cx Cy >= K).  Wa = Cx (R + 1),
 * Ha = Cy R.  The origin of cell k is X0 = (k % Cx)(R + 1), Y0 = (k / Cx) R.
 *   lower texel (i, j) sits at (X0 + i, Y0 + j);   upper texel (i, j) sits at (X0 + R - i, Y0 + R - 1 - j).
 * The two sets are disjoint and fill the cell: x + y - X0 - Y0 <= R - 1 for lower texels and >= R for upper ones.
 *   atlas_idx[p] (optional) = y Wa + x for a drawn pixel and -1 otherwise.
 *
 * UVs (computed by the caller; diff_recon_hip.mesh_texture.face_uvs).  uv is F x 3 x 2 fp32 in glTF's convention: origin top-left, image
 * row y is v Ha.  In texel units the corners (a, b, c) of a lower face are (X0, Y0), (X0 + R, Y0), (X0, Y0 + R), those of an upper face
 * (X0 + R + 1, Y0 + R), (X0 + 1, Y0 + R), (X0 + R + 1, Y0);  uv = ((float)((double)x / (double)Wa), (float)((double)y / (double)Ha)).
 * The atlas is exact under a NEAREST sampler only: floor(uv size) of an interior point of a face is the texel above.  There are no
 * gutters: a bilinear or mip-mapped sampler mixes the texels of neighbouring faces along every edge.
 *
 * Accumulator.  texels: F T rows of four unsigned 64-bit words {count, sum_r, sum_g, sum_b}, caller-cleared, accumulated by
 * ts2d_mesh_census_add.  At R == 1, texel_idx == face_idx on every drawn pixel.
 *
 * Face totals (tsa_face_totals).  face_totals: F x 4 unsigned 64-bit words, each the integer sum of the face's T rows.  A segmented
 * reduction without atomics: several faces to a wave at small T, one wave per face at large T.
 *
 * Resolve (tsa_resolve; one thread per atlas texel).  Every atlas texel (x, y) is written.  The placement is inverted: the cell from
 * x / (R + 1), y / R, then lx = x % (R + 1), ly = y % R; lx + ly <= R - 1 is the lower face with (i, j) = (lx, ly), anything else the
 * upper face with (i, j) = (R - lx, R - 1 - ly).  The first rule that applies:
 *   1  f >= F (the empty half of the last cell, or empty cells): fill, state 0.
 *   2  count[n] >= min_count (min_count >= 1): (float)((double)sum_c / ((double)count 65536)), state 3.
 *   3  the face's total count is >= 1: the same quotient on the face totals, state 2.
 *   4  face_fallback (F x 3 fp32, optional) is given: that row, state 1.
 *   5  otherwise: fill, state 0.
 * image: 3 Ha Wa fp32, planar.  state: Ha Wa bytes.  rgb8 (optional): Ha Wa 3 bytes, interleaved, each
 * (uint8) rint(min(max(c, 0), 1) 255) in double; a NaN gives 0.
 *
 * Render (tsa_render; one thread per pixel).  out[ch H W + p] = image[ch Ha Wa + atlas_idx[p]] where 0 <= atlas_idx[p] < Wa Ha, and
 * background[ch] (3 device floats) elsewhere.  Nothing is read out of bounds for any contents of atlas_idx.  Nothing is clamped.
 *
 * Purity (DESIGN.md "Purity of the entry points").  The outputs may hold anything on entry; texel_idx, atlas_idx, bary, face_totals,
 * image, state, rgb8 and out are overwritten in full; no byte outside an output's extent is written.
 */
#ifndef TS_ATLAS_H
#define TS_ATLAS_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSA_MAX_RES 64

/* The text of the calling thread's last error of this library. */
const char *tsa_last_error(void);

/* view: 16 floats; vertices: V*3 floats; faces: F*3 int32; face_idx: H*W int32; texel_idx: H*W int32; atlas_idx: H*W int32 or NULL;
 * bary: 3*H*W floats or NULL.  vertices may be NULL with V == 0, faces with F == 0. */
int tsa_texel_index(const float *view, float tan_fovx, float tan_fovy, int32_t W, int32_t H, int32_t V, const float *vertices, int32_t F,
                    const int32_t *faces, const int32_t *face_idx, int32_t R, int32_t Cx, int32_t *texel_idx, int32_t *atlas_idx, float *bary,
                    void *stream);

/* texels: F*T*4 64-bit words; face_totals: F*4 64-bit words.  F == 0 is a no-op that returns TS2D_OK. */
int tsa_face_totals(int32_t F, int32_t R, const unsigned long long *texels, unsigned long long *face_totals, void *stream);

/* texels, face_totals: as above, may be NULL with F == 0; face_fallback: F*3 floats or NULL; fill: 3 HOST floats;
 * image: 3*Ha*Wa floats; state: Ha*Wa bytes; rgb8: Ha*Wa*3 bytes or NULL, with Wa = Cx (R + 1), Ha = Cy R. */
int tsa_resolve(int32_t F, int32_t R, int32_t Cx, int32_t Cy, const unsigned long long *texels, const unsigned long long *face_totals,
                int32_t min_count, const float *face_fallback, const float *fill, float *image, uint8_t *state, uint8_t *rgb8, void *stream);

/* atlas_idx: H*W int32; image: 3*Ha*Wa floats; background: 3 floats; out: 3*H*W floats. */
int tsa_render(int32_t W, int32_t H, int32_t Wa, int32_t Ha, const int32_t *atlas_idx, const float *image, const float *background, float *out,
               void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_ATLAS_H */
