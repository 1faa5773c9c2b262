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
 *
 * The two calls share the three opaque state buffers of ts2d.h (ts2d_state, ts2d_binning_state_bytes, ts2d_image_state_bytes) and the
 * rasterizer's ordering chain; like ts2d_forward_bin / ts2d_forward_render they are split where the caller sizes the binning buffer.
 * All pointers except `cam`, `state` and `num_rendered` are device pointers; everything is enqueued on `stream` (a hipStream_t).
 * Return value and ts2d_last_error() as in ts2d.h.
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

#ifdef __cplusplus
}
#endif
#endif /* TS_MESH_H */
