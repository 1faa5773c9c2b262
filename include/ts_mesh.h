/*
 * ts_mesh.h -- C ABI of the opaque triangle-mesh renderer of libts2d.so: a per-pixel depth-tested (z-buffer) rasterizer for the
 * meshes the reference exports with saveGLB and looks at through src/diff_recon/renderer/kaolin_renderer.py (Kaolin's CUDA-only
 * `nvdiffrast_fwd` backend).  Forward only, like that backend.
 *
 * Semantics ("Opaque mesh renderer"):
 *   view space   p_view = [p, 1] @ viewmatrix (row-vector convention, ts2d.h); depth = p_view.z
 *   validity     a face is drawn iff its three indices lie in [0, V) and its three vertices have depth > znear
 *                (kaolin_renderer.py:51); no clipping, no back-face culling
 *   screen       x = (x_v / (z_v tan_fovx) + 1) W / 2,  y = (y_v / (z_v tan_fovy) + 1) H / 2; the centre of pixel (i, j) is (i + .5, j + .5)
 *   coverage     the pixel centre lies inside or on the projected triangle
 *   depth        ray / plane intersection in view space, d = (n . a) / (n . r), r = (x_ndc tan_fovx, y_ndc tan_fovy, 1), kept inside the
 *                depth range of the face's own vertices
 *   winner       the smallest d; ties go to the smaller face index: the images are a pure function of the inputs
 *   vertex order a face's record is built from its vertices in ascending index order, so two faces that name the same three vertices --
 *                a front face and its reversed back twin -- have the same coverage and depth bit for bit: the twin never wins a pixel
 *
 * The two render calls (ts2d_mesh_bin, ts2d_mesh_render) share the three opaque state buffers of ts2d.h (ts2d_state,
 * ts2d_binning_state_bytes, ts2d_image_state_bytes) and the rasterizer's ordering chain; like ts2d_forward_bin / ts2d_forward_render they
 * are split where the caller sizes the binning buffer.  A third call, ts2d_mesh_census_add, consumes the `face_idx` image: a per-face
 * reduction (pixels won, fixed-point colour sums of a target image) that accumulates over views in integers.
 * All pointers except `cam`, `state` and `num_rendered` are device pointers; everything is enqueued on `stream` (a hipStream_t).
 * Return value and ts2d_last_error() as in ts2d.h.
 * Purity (DESIGN.md "Purity of the entry points"): the images are functions of the documented inputs only, whatever the state buffers and
 * the outputs held on entry; every element of every non-NULL output of the render calls is overwritten; `census` and `wave_visits` are
 * caller-cleared accumulators (inputs); no byte outside the state sizes or an output's extent is written.
 */
#ifndef TS_MESH_H
#define TS_MESH_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the geometry state for F faces (the rasterizer's for F triangles). */
size_t ts2d_mesh_geometry_state_bytes(int32_t F);

/* Per-face setup (gather through `faces`, view transform, validity, tile rectangle, nearest-vertex depth as the sort key), depth order and
 * prefix sum.  Uses cam->width / height / tan_fovx / tan_fovy / viewmatrix only (projmatrix and campos may be NULL).  znear >= 0.
 * vertices: V*3 floats; faces: F*3 int32.  Returns the number of (tile, face) instances like ts2d_forward_bin; the host waits for that
 * count only, never for the whole stream.  F must be below 2^28 (TS2D_ERR_CAPACITY). */
int ts2d_mesh_bin(const ts2d_camera *cam, float znear, int32_t V, const float *vertices, int32_t F, const int32_t *faces,
                  const ts2d_state *state, int64_t *num_rendered, void *stream);

/* Instance emission, (tile, depth) sort, tile ranges and the per-pixel depth test.  Fully asynchronous.
 * faces_color: F*3 floats; background: 3 floats.  Every element of every non-NULL output is written:
 *   render   3*H*W  the winner's colour, else the background, clamped to [0, 1] (kaolin_renderer.py:63-64)
 *   mask     H*W    1.0 where a face was drawn, else 0.0
 *   depth    H*W    the winner's depth, 0 where uncovered            (may be NULL)
 *   face_idx H*W    the winner's index, -1 where uncovered           (may be NULL) */
int ts2d_mesh_render(const ts2d_camera *cam, int32_t F, const float *faces_color, const float *background, int64_t num_rendered,
                     const ts2d_state *state, float *render, float *mask, float *depth, int32_t *face_idx, void *stream);

/* The same render; `wave_visits` (one 64-bit device word that the caller cleared, or NULL) additionally receives how many (wavefront, face)
 * pairs the depth test walked.  A tile's list is walked by four wavefronts, each of which stops at the first face that lies wholly behind
 * everything it has kept, so 4 * num_rendered minus this count is what the early stop saved (tools/bench_mesh.py). */
int ts2d_mesh_render_counted(const ts2d_camera *cam, int32_t F, const float *faces_color, const float *background, int64_t num_rendered,
                             const ts2d_state *state, float *render, float *mask, float *depth, int32_t *face_idx,
                             unsigned long long *wave_visits, void *stream);

/* Census of one view: adds, for every counted pixel, one row update to `census`.
 * census: F rows of 4 unsigned 64-bit words {pixels, sum_r, sum_g, sum_b}, device memory, cleared by the caller before the first view.
 * face_idx: H*W int32 (ts2d_mesh_render's output).  target: 3*H*W floats (planar, like `render`) or NULL.  pixel_mask: H*W floats or NULL.
 *   counted    pixel p is counted iff 0 <= face_idx[p] < F and (pixel_mask == NULL or pixel_mask[p] > 0); every other index, -1
 *              included, is skipped, and so is a NaN mask value.  Nothing is read or written out of bounds for any face_idx contents.
 *   pixels     a counted pixel adds 1 to word 0 of row face_idx[p]
 *   colour     with a target it also adds q(c) = (uint64) rintf(fminf(fmaxf(c, 0), 1) * 65536.0f) per channel to words 1..3: Q16 fixed
 *              point, rounding to nearest even, a NaN target adds 0.  c * 65536 is exact in fp32, so q is a pure function of c.
 *              With target == NULL only word 0 changes.
 *   exactness  all sums are integers: the result does not depend on the order of pixels, wavefronts or views, and the same calls always
 *              leave the same bits.  A word cannot overflow in any realistic sweep (2^63 / 2^16 / 2 Mpx: 3e7 views).
 * width, height >= 1 with at most 2^31 - 1 pixels, F >= 0, face_idx non-NULL, census non-NULL unless F == 0: otherwise TS2D_ERR_INVALID,
 * decided before any HIP call.  F == 0 is a no-op that returns TS2D_OK.  Fully asynchronous. */
int ts2d_mesh_census_add(int32_t width, int32_t height, int32_t F, const int32_t *face_idx, const float *target,
                         const float *pixel_mask, unsigned long long *census, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_MESH_H */
