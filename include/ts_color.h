/*
 * ts_color.h -- C ABI of libts_color.so: colour fused beside the distances of a ts_volume.h grid (integer sums), the colour field, a
 * trilinear sampler of any channel-planar fp32 grid that skips samples without data, and the per-pixel interpolation of vertex attributes
 * over a face_idx image.  diff_recon_hip/color_volume.py builds ColorTSDFVolume, sample_grid, interpolate_vertex_attributes,
 * render_vertex_colors and fuse_colored_mesh on it.
 *
 * A library of its own, beside libts2d.so, libts_geom.so, libts_bvh.so, libts_ray.so and libts_volume.so: the export lists of all five are
 * closed.  libts_color.so links no object of the others and keeps its own error text.  The error codes are ts2d.h's.  Nothing is extracted
 * here: the surface comes from ts_volume.h, and colour is read off the grid at its vertices by a pure function of position.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a dimension below 1, a null required pointer, h or trunc (or a tangent) that is NaN,
 * infinite or not positive, an image size below 1, min_weight below 1, C outside [1, 8], a negative N, V or F return TS2D_ERR_INVALID with
 * the text in the last-error call of this header.  A grid of more than 2^27 samples, or an image of more than 2^31 - 1 pixels, is
 * TS2D_ERR_CAPACITY.  N == 0 is a no-op that returns TS2D_OK; tsc_interpolate with F == 0 still writes the background everywhere.
 *
 * The volume is ts_volume.h's: nx * ny * nz samples; sample (i, j, k) has the linear index n = (k ny + j) nx + i and sits at
 * p[a] = (double)o[a] + (double)h * idx[a], o = (ox, oy, oz).  The colour state is two arrays over n: csum (3 n int64, channels interleaved,
 * csum[3 n + c]) and cweight (n int32).  The units are built with -ffp-contract=off.  Everything below is float64, computed from the fp32
 * inputs widened to double, with every operation rounded.
 *
 * Integration of one view's colour.  One thread per sample, no atomics on the state.  M = the 16 floats of world_view_transform in the
 * row-vector convention (M[r][c] = view[4 r + c]).  Steps 1-3 are those of tsv_integrate, restated:
 *   1  v[c] = ((p0 M[0][c] + p1 M[1][c]) + p2 M[2][c]) + M[3][c], z = v[2]; skipped unless z is finite and > 0.
 *   2  u = (v0 / (z tan_fovx) + 1) (0.5 W), col = floor(u); row likewise from v1, tan_fovy, H: the inverse of the pixel-centre rays of
 *      diff_recon_hip.camera_rays.  Skipped unless 0 <= col < W and 0 <= row < H (a NaN fails the test).
 *   3  skipped if `mask` (H W bytes, optional) is 0 at the pixel.
 *   4  d = depth[row W + col].  Skipped unless d is finite and > 0: an uncovered pixel never colours anything; there is no carving flag.
 *   5  sd = d - z.  Skipped unless -trunc <= sd <= trunc: the band in which the distance is not clipped.
 *   6  x[c] = image[c H W + row W + col], c = 0, 1, 2 (planar, like MeshRenderer's render).  Skipped if any of the three is NaN or infinite.
 *   7  q[c] = (int64) rint(min(max(x[c], 0), 1) 65536): the Q16 rule of ts2d_mesh_census_add, in double.
 *   8  A sample whose cweight is INT32_MAX is skipped.  Otherwise csum[3 n + c] += q[c], cweight[n] += 1.
 *   9  `updated` (optional, one caller-cleared 64-bit word) gains the number of samples coloured.
 * The sums are integers: the state after any set of views is bit-identical in any order, and the states of two volumes can be added.
 * Only coloured samples are read and written back.
 *
 * Colour field.  field[c n_total + n] (channel-planar, 3 n_total floats) = cweight >= min_weight
 *   ? (float)((double)csum[3 n + c] / ((double)cweight 65536)) : NaN (0x7FC00000), in all three channels.
 *
 * Sampler.  grid: C nx ny nz floats, channel-planar (grid[c n_total + n]), 1 <= C <= 8; with C == 1 it is tsv_field's output as it is.
 * A sample HAS DATA iff all C of its values are finite.  One thread per point.  For point p (points: N * 3 floats), per axis a with n_a
 * samples: g = ((double)p[a] - (double)o[a]) / (double)h.  The point is OUTSIDE unless 0 <= g <= n_a - 1 on every axis (a NaN fails): then
 * valid = 0 and out = NaN.  Otherwise, per axis: base b = min((int)floor(g), n_a - 2) where n_a >= 2 (a point on the upper face uses the
 * last cell), b = 0 where n_a == 1; t = g - b; the factor of a corner is t where its bit of that axis is 1, else 1 - t; where n_a == 1
 * only the corners whose bit of that axis is 0 exist.  Corner k = bit0 x + bit1 y + bit2 z is the sample (bx + bit0, by + bit1, bz + bit2)
 * and has the weight w = (wx wy) wz.  Over the existing corners that have data, in ascending k:
 *   num[c] = sum of w value[c],  den = sum of w;  the first addend is assigned, not added to zero.
 * A corner without data is left out; a corner with data and weight 0 adds 0.  If den > 0: out[i C + c] = (float)(num[c] / den), valid[i] = 1;
 * otherwise out[i C + c] = NaN (0x7FC00000) and valid[i] = 0.  out: N * C floats, point-major; valid: N bytes.
 * The result is a function of the point's position and the grid alone: vertices that welding with eps = 0 merges get equal bits.
 *
 * Interpolation of vertex attributes.  One thread per pixel.  Pixel (col, row), p = row W + col, is DRAWN iff f = face_idx[p] lies in
 * [0, F) and the three indices (ia, ib, ic) = faces[3 f .. 3 f + 2] lie in [0, V); nothing is read out of bounds for any contents of
 * face_idx or faces.  For a drawn pixel, with P = vertices[3 i .. 3 i + 2] of i = ia, ib, ic in face order:
 *   a[k] = ((P0 M[0][k] + P1 M[1][k]) + P2 M[2][k]) + M[3][k], k = 0, 1, 2; b and c likewise: the view-space corners.
 *   r = (((col + 0.5) / (0.5 W) - 1) tan_fovx, ((row + 0.5) / (0.5 H) - 1) tan_fovy, 1): camera_rays' direction in view space.
 *   x cross y = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0);  r dot n = (r0 n0 + r1 n1) + n2.
 *   wa = r dot (b cross c), wb = r dot (c cross a), wc = r dot (a cross b);  s = (wa + wb) + wc.
 *   If s < 0 all three are negated.  Every weight that is then negative or NaN (not w >= 0) becomes 0.  s' = (wa + wb) + wc.
 *   If s' is finite and > 0: (alpha, beta, gamma) = (wa / s', wb / s', wc / s'); otherwise each is 1.0 / 3.0.
 * These are the perspective-correct barycentrics of the ray / plane hit, held inside the face: a silhouette pixel that the fp32 coverage
 * test of the renderer took still gets a convex combination.
 *   out[ch H W + p] = (float)((alpha A[ia C + ch] + beta A[ib C + ch]) + gamma A[ic C + ch]), A = attributes (V * C floats), 1 <= C <= 8.
 * A pixel that is not drawn gets background[ch] (C device floats).  bary (optional, 3 H W floats, planar) = ((float)alpha, (float)beta,
 * (float)gamma) on drawn pixels and 0 elsewhere.  Nothing is clamped.
 *
 * Purity (DESIGN.md "Purity of the entry points").  The outputs may hold anything on entry; field, out, valid and bary are overwritten in
 * full; csum, cweight and updated are caller-owned accumulators; no byte outside an output's extent is written.  No call has a workspace.
 */
#ifndef TS_COLOR_H
#define TS_COLOR_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSC_MAX_SAMPLES (1 << 27)
#define TSC_MAX_CHANNELS 8

/* The text of the calling thread's last error of this library. */
const char *tsc_last_error(void);

/* view: 16 floats; depth: H*W floats; mask: H*W bytes or NULL; image: 3*H*W floats; csum: 3*nx*ny*nz int64; cweight: nx*ny*nz int32;
 * updated: one 64-bit device word that the caller cleared, or NULL. */
int tsc_integrate(int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz, float h, float trunc, const float *view, float tan_fovx,
                  float tan_fovy, int32_t W, int32_t H, const float *depth, const uint8_t *mask, const float *image, int64_t *csum,
                  int32_t *cweight, unsigned long long *updated, void *stream);

/* field: 3*nx*ny*nz floats, channel-planar. */
int tsc_color_field(int32_t nx, int32_t ny, int32_t nz, const int64_t *csum, const int32_t *cweight, int32_t min_weight, float *field,
                    void *stream);

/* grid: C*nx*ny*nz floats, channel-planar; points: N*3 floats; out: N*C floats; valid: N bytes. */
int tsc_sample(int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz, float h, int32_t C, const float *grid, int32_t N,
               const float *points, float *out, uint8_t *valid, void *stream);

/* view: 16 floats; vertices: V*3 floats; faces: F*3 int32; face_idx: H*W int32; attributes: V*C floats; background: C floats;
 * out: C*H*W floats; bary: 3*H*W floats or NULL.  vertices and attributes may be NULL with V == 0, faces with F == 0. */
int tsc_interpolate(const float *view, float tan_fovx, float tan_fovy, int32_t W, int32_t H, int32_t V, const float *vertices, int32_t F,
                    const int32_t *faces, const int32_t *face_idx, int32_t C, const float *attributes, const float *background, float *out,
                    float *bary, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_COLOR_H */
