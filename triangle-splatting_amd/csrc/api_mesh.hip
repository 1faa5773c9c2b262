// api_mesh.hip -- the C ABI of include/ts_mesh.h (the opaque z-buffer mesh renderer and its census) and include/ts_weld.h (welding).
// The renderer runs the rasterizer's ordering chain (ts2d_api.h) between its own per-face and per-pixel kernels.
#pragma GCC visibility push(default)
#include "../../include/ts_mesh.h"
#include "../../include/ts_weld.h"
#pragma GCC visibility pop
#include "ts2d_api.h"
#include "ts_weld_launch.h"
#include <cfloat>

#define TS_WELD_MAX_FACES 715827882 /* 3 F edge slots are addressed with 31 bits */

namespace
{
int validate_mesh_camera(const ts2d_camera *cam)
{
    if (!cam) return ts_fail(TS2D_ERR_INVALID, "null camera");
    if (cam->width <= 0 || cam->height <= 0) return ts_fail(TS2D_ERR_INVALID, "image size must be positive");
    if (cam->width > 65535 * TS_TILE || cam->height > 65535 * TS_TILE) return ts_fail(TS2D_ERR_INVALID, "image too large");
    if (!(cam->tan_fovx > 0.0f) || !(cam->tan_fovy > 0.0f)) return ts_fail(TS2D_ERR_INVALID, "tan_fovx / tan_fovy must be positive");
    return TS2D_OK;
}
int validate_mesh_faces(int32_t F)
{
    if (F < 0) return ts_fail(TS2D_ERR_INVALID, "F must be >= 0");
    if (F > (int)TS_ID_MASK) return ts_fail(TS2D_ERR_CAPACITY, "more than 2^28 - 1 faces: the instance values keep four bits of each face index");
    return TS2D_OK;
}
MeshArgs make_mesh(const ts2d_camera *cam, float znear, int32_t V, const float *vertices, int32_t F, const int32_t *faces)
{
    MeshArgs a;
    a.W = cam->width; a.H = cam->height; a.V = V; a.F = F;
    a.grid_x = (cam->width + TS_TILE - 1) / TS_TILE; a.grid_y = (cam->height + TS_TILE - 1) / TS_TILE;
    a.tan_fovx = cam->tan_fovx; a.tan_fovy = cam->tan_fovy; a.znear = znear;
    a.viewmatrix = cam->viewmatrix; a.vertices = vertices; a.faces = faces;
    return a;
}
int weld_counts_ok(int32_t V, int32_t F)
{
    if (V < 0) return ts_fail(TS2D_ERR_INVALID, "V must be >= 0");
    if (F < 0) return ts_fail(TS2D_ERR_INVALID, "F must be >= 0");
    if (F > TS_WELD_MAX_FACES) return ts_fail(TS2D_ERR_INVALID, "F must be at most %d", TS_WELD_MAX_FACES);
    return TS2D_OK;
}
int weld_workspace_ok(int32_t V, int32_t F, const void *workspace, size_t workspace_bytes)
{
    if (!workspace) return ts_fail(TS2D_ERR_INVALID, "workspace is null");
    if (workspace_bytes < ts_weld_workspace_bytes(V, F)) return ts_fail(TS2D_ERR_INVALID, "weld workspace too small");
    return TS2D_OK;
}
} // namespace

extern "C" {
// ---- include/ts_mesh.h ------------------------------------------------------------------------------------------------
size_t ts2d_mesh_geometry_state_bytes(int32_t F) { return ts2d_geometry_state_bytes(F); }

int ts2d_mesh_bin(const ts2d_camera *cam, float znear, int32_t V, const float *vertices, int32_t F, const int32_t *faces,
                  const ts2d_state *state, int64_t *num_rendered, void *stream)
{
    if (int rc = validate_mesh_camera(cam)) return rc;
    if (int rc = validate_mesh_faces(F)) return rc;
    if (!cam->viewmatrix) return ts_fail(TS2D_ERR_INVALID, "viewmatrix is null");
    if (!(znear >= 0.0f)) return ts_fail(TS2D_ERR_INVALID, "znear must be >= 0"); // the depth keys are ordered by their bit patterns
    if (V < 0) return ts_fail(TS2D_ERR_INVALID, "V must be >= 0");
    if (!state || !num_rendered) return ts_fail(TS2D_ERR_INVALID, "null state/num_rendered");
    *num_rendered = 0;
    if (F == 0) return TS2D_OK;
    if (!faces || (V > 0 && !vertices)) return ts_fail(TS2D_ERR_INVALID, "vertices/faces is null");
    if (!state->geometry || state->geometry_bytes < ts2d_geometry_state_bytes(F))
        return ts_fail(TS2D_ERR_CAPACITY, "geometry state buffer too small: %zu < %zu", state->geometry_bytes, ts2d_geometry_state_bytes(F));
    hipStream_t s = (hipStream_t)stream;
    GeometryStateView g;
    ts_carve_geometry((char *)state->geometry, F, g);
    const MeshArgs a = make_mesh(cam, znear, V, vertices, F, faces);
    EarlyCount early;
    const bool have_early = acquire_early_count(early);
    { ProfScope ps("mesh_preprocess", s); ts_launch_mesh_preprocess(a, g, s); }
    TS_CHECK(0u, s, "mesh_preprocess");
    if (int rc = ts_order_triangles(0u, g, F, have_early ? &early : nullptr, s)) return rc;
    return wait_instance_count(F, state, have_early ? &early : nullptr, s, num_rendered);
}

int ts2d_mesh_render_counted(const ts2d_camera *cam, int32_t F, const float *faces_color, const float *background, int64_t N,
                             const ts2d_state *state, float *render, float *mask, float *depth, int32_t *face_idx,
                             unsigned long long *wave_visits, void *stream)
{
    if (int rc = validate_mesh_camera(cam)) return rc;
    if (int rc = validate_mesh_faces(F)) return rc;
    if (!background || (F > 0 && !faces_color)) return ts_fail(TS2D_ERR_INVALID, "faces_color/background is null");
    if (!state || !render || !mask) return ts_fail(TS2D_ERR_INVALID, "null state/output");
    if (N < 0) return ts_fail(TS2D_ERR_INVALID, "num_rendered < 0");
    if (N > 0x7fffffffll) return ts_fail(TS2D_ERR_CAPACITY, "the instance list addresses at most 2^31 - 1 instances");
    const int W = cam->width, H = cam->height;
    if (F == 0 && N > 0) return ts_fail(TS2D_ERR_INVALID, "num_rendered > 0 without faces");
    if (!state->image || state->image_bytes < ts2d_image_state_bytes(W, H)) return ts_fail(TS2D_ERR_CAPACITY, "image state buffer too small");
    if (N > 0 && (!state->binning || ts_binning_capacity(state->binning_bytes, W, H) < N))
        return ts_fail(TS2D_ERR_CAPACITY, "binning state buffer too small");
    if (F > 0 && (!state->geometry || state->geometry_bytes < ts2d_geometry_state_bytes(F)))
        return ts_fail(TS2D_ERR_CAPACITY, "geometry state buffer too small");
    hipStream_t s = (hipStream_t)stream;
    GeometryStateView g{};
    BinningStateView b{};
    ImageStateView im{};
    if (F > 0) ts_carve_geometry((char *)state->geometry, F, g);
    if (N > 0)
    {
        ts_carve_binning((char *)state->binning, ts_binning_capacity(state->binning_bytes, W, H), W, H, b);
        ts_binning_set_count(b, N);
    }
    ts_carve_image((char *)state->image, W, H, im);
    const MeshArgs a = make_mesh(cam, 0.0f, 0, nullptr, F, nullptr);
    const int ntiles = a.grid_x * a.grid_y;
    // variant 0: every instance reaches every quadrant -- the depth test walks whole tiles and ignores the values' mask bits
    const QuadMaskArgs quad{0, 0.0f, cam->tan_fovx, cam->tan_fovy, W, H, 1.0f / (float)W, 1.0f / (float)H};
    if (int rc = ts_order_instances(0u, F, a.grid_x, ntiles, g, b, im, nullptr, nullptr, N, nullptr, quad, s)) return rc;
    { ProfScope ps("mesh_resolve", s); ts_launch_mesh_resolve(a, g, b, im, faces_color, background, render, mask, depth, face_idx, wave_visits, s); }
    TS_CHECK(0u, s, "mesh_resolve");
    return TS2D_OK;
}

int ts2d_mesh_render(const ts2d_camera *cam, int32_t F, const float *faces_color, const float *background, int64_t N,
                     const ts2d_state *state, float *render, float *mask, float *depth, int32_t *face_idx, void *stream)
{
    return ts2d_mesh_render_counted(cam, F, faces_color, background, N, state, render, mask, depth, face_idx, nullptr, stream);
}

int ts2d_mesh_census_add(int32_t width, int32_t height, int32_t F, const int32_t *face_idx, const float *target, const float *pixel_mask,
                         unsigned long long *census, void *stream)
{
    if (width < 1 || height < 1) return ts_fail(TS2D_ERR_INVALID, "image size must be positive");
    if ((int64_t)width * height > 0x7fffffffll) return ts_fail(TS2D_ERR_INVALID, "image too large: the census sweeps at most 2^31 - 1 pixels");
    if (F < 0) return ts_fail(TS2D_ERR_INVALID, "F must be >= 0");
    if (!face_idx) return ts_fail(TS2D_ERR_INVALID, "face_idx is null");
    if (F == 0) return TS2D_OK; // no row to add to
    if (!census) return ts_fail(TS2D_ERR_INVALID, "census is null");
    hipStream_t s = (hipStream_t)stream;
    { ProfScope ps("mesh_census", s); ts_launch_mesh_census(width, height, F, face_idx, target, pixel_mask, census, s); }
    TS_CHECK(0u, s, "mesh_census");
    return TS2D_OK;
}

// ---- include/ts_weld.h ------------------------------------------------------------------------------------------------

size_t ts2d_weld_workspace_bytes(int32_t V, int32_t F) { return ts_weld_workspace_bytes(V, F); }


int ts2d_weld_labels_counted(int32_t V, const float *vertices, float eps, int32_t *label, unsigned long long *box_visits, void *workspace,
                             size_t workspace_bytes, void *stream)
{
    if (int rc = weld_counts_ok(V, 0)) return rc;
    if (!(eps >= 0.0f) || !(eps <= FLT_MAX)) return ts_fail(TS2D_ERR_INVALID, "eps must be finite and >= 0");
    if (V == 0) return TS2D_OK;
    if (!vertices || !label) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (int rc = weld_workspace_ok(V, 0, workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("weld_labels", s);
    TS_HIP(ts_weld_labels(V, vertices, eps, (uint32_t *)label, box_visits, workspace, s));
    return TS2D_OK;
}

int ts2d_weld_labels(int32_t V, const float *vertices, float eps, int32_t *label, void *workspace, size_t workspace_bytes, void *stream)
{
    return ts2d_weld_labels_counted(V, vertices, eps, label, nullptr, workspace, workspace_bytes, stream);
}

int ts2d_weld_face_components(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep, int32_t *label, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes; // the union-find works in `label` itself
    if (int rc = weld_counts_ok(V, F)) return rc;
    if (V == 0) return TS2D_OK;
    if (!label || (F > 0 && !faces)) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("weld_face_components", s);
    TS_HIP(ts_weld_face_components(V, F, faces, keep, (uint32_t *)label, s));
    return TS2D_OK;
}

int ts2d_weld_compact(int32_t V, const int32_t *label, const float *vertices, int32_t mode, int32_t *remap, float *out_vertices,
                      int32_t *count, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = weld_counts_ok(V, 0)) return rc;
    if (mode != TS2D_WELD_FIRST && mode != TS2D_WELD_MEAN) return ts_fail(TS2D_ERR_INVALID, "mode must be TS2D_WELD_FIRST or TS2D_WELD_MEAN");
    if (V == 0) return TS2D_OK;
    if (!label || !vertices || !remap || !out_vertices || !count) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (int rc = weld_workspace_ok(V, 0, workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("weld_compact", s);
    TS_HIP(ts_weld_compact(V, (const uint32_t *)label, vertices, mode, remap, out_vertices, count, workspace, s));
    return TS2D_OK;
}

int ts2d_weld_remap_faces(int32_t V, int32_t F, const int32_t *faces, const int32_t *remap, int32_t *out_faces, uint8_t *keep, void *stream)
{
    if (int rc = weld_counts_ok(V, F)) return rc;
    if (F == 0) return TS2D_OK;
    if (!faces || !out_faces || !keep || (V > 0 && !remap)) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("weld_remap_faces", s);
    TS_HIP(ts_weld_remap_faces(V, F, faces, remap, out_faces, keep, s));
    return TS2D_OK;
}

int ts2d_weld_edge_census(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep, unsigned long long *counts, void *workspace,
                          size_t workspace_bytes, void *stream)
{
    if (int rc = weld_counts_ok(V, F)) return rc;
    if (F == 0) return TS2D_OK;
    if (!faces || !counts) return ts_fail(TS2D_ERR_INVALID, "null pointer");
    if (int rc = weld_workspace_ok(V, F, workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("weld_edge_census", s);
    TS_HIP(ts_weld_edge_census(V, F, faces, keep, counts, workspace, s));
    return TS2D_OK;
}
} // extern "C"
