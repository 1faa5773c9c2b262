// mesh_preprocess.hip -- per-face setup of the opaque mesh renderer (include/ts_mesh.h).
//
// One lane per face: gather the three vertices through `faces`, transform them to view space, decide validity (every index inside
// [0, V), every vertex at depth > znear: src/diff_recon/renderer/kaolin_renderer.py:51 of the reference; no clipping, no back-face
// culling), project to pixels, and leave behind what the ordering chain and mesh_resolve.hip read: the tile rectangle of the pixel
// centres inside the bounding box, tiles_touched, the face record (ts2d_common.h) and the NEAREST vertex depth as the sort key.
// That key, not the centroid's depth, is what makes the resolve kernel's early stop exact: no point of a face is nearer than its
// nearest vertex, so once a wavefront's pixels all hold something nearer than the next key, nothing later in the list can win.
// Built with -ffp-contract=off like the other preprocess units: the expressions evaluate as written.
#include "ts2d_common.h"
#include "ts2d_math.h"
#include "ts2d_preprocess_launch.h"

using namespace ts;

namespace
{
// A pixel centre this close outside the bounding box still counts as inside it: far above the rounding of a projected coordinate
// (2^-13 px at x = 2000), far below anything that changes which pixel centres a face can cover.
constexpr float BOX_MARGIN = 2e-3f;

__global__ void __launch_bounds__(256) mesh_preprocess_kernel(MeshArgs a, GeometryStateView g)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    clear_tickets(g, f, a.F); // the step's first launch zeroes what the ordering chain counts in (ts2d_preprocess_launch.h)
    if (f >= a.F) return;
    uint32_t out_tiles = 0;
    uint2 out_rect = {0u, 0u};
    float out_key = 0.0f;
    float rec[TS_REC_FLOATS];
#pragma unroll
    for (int i = 0; i < TS_REC_FLOATS; i++) rec[i] = 0.0f;

    // The record is built from the face's vertices in ASCENDING INDEX order, whatever order `faces` names them in: neither coverage nor depth
    // depends on the winding (no back-face culling; mesh_resolve.hip orients the edges itself), and a reversed twin -- the back face saveGLB
    // appends with the same three indices -- then gets its front face's record bit for bit.  Same coverage, same depth on every pixel: the
    // tie goes to the smaller index and a twin never wins a pixel (include/ts_mesh.h).  A face that already names its vertices in ascending
    // order, as every front face of an un-shared soup does, is untouched.
    int32_t i1 = a.faces[3 * (size_t)f], i2 = a.faces[3 * (size_t)f + 1], i3 = a.faces[3 * (size_t)f + 2];
    if (i1 > i2) { const int32_t t = i1; i1 = i2; i2 = t; }
    if (i2 > i3) { const int32_t t = i2; i2 = i3; i3 = t; }
    if (i1 > i2) { const int32_t t = i1; i1 = i2; i2 = t; }
    do
    {
        if ((uint32_t)i1 >= (uint32_t)a.V || (uint32_t)i2 >= (uint32_t)a.V || (uint32_t)i3 >= (uint32_t)a.V) break; // never read out of bounds
        const float *p1 = a.vertices + 3 * (size_t)i1, *p2 = a.vertices + 3 * (size_t)i2, *p3 = a.vertices + 3 * (size_t)i3;
        const f3 v1 = xform_point_4x3({p1[0], p1[1], p1[2]}, a.viewmatrix), v2 = xform_point_4x3({p2[0], p2[1], p2[2]}, a.viewmatrix),
                 v3 = xform_point_4x3({p3[0], p3[1], p3[2]}, a.viewmatrix);
        if (!(v1.z > a.znear && v2.z > a.znear && v3.z > a.znear)) break; // also refuses NaN

        const float hw = (float)a.W * 0.5f, hh = (float)a.H * 0.5f;
        const f2 s1 = {(v1.x / (v1.z * a.tan_fovx) + 1.0f) * hw, (v1.y / (v1.z * a.tan_fovy) + 1.0f) * hh};
        const f2 s2 = {(v2.x / (v2.z * a.tan_fovx) + 1.0f) * hw, (v2.y / (v2.z * a.tan_fovy) + 1.0f) * hh};
        const f2 s3 = {(v3.x / (v3.z * a.tan_fovx) + 1.0f) * hw, (v3.y / (v3.z * a.tan_fovy) + 1.0f) * hh};
        const float area2 = cross(sub(s2, s1), sub(s3, s1));
        if (!(fabsf(area2) > 0.0f)) break; // edge-on or collapsed on the screen: covers no pixel centre

        const float xmin = fminf(fminf(s1.x, s2.x), s3.x), xmax = fmaxf(fmaxf(s1.x, s2.x), s3.x);
        const float ymin = fminf(fminf(s1.y, s2.y), s3.y), ymax = fmaxf(fmaxf(s1.y, s2.y), s3.y);
        if (!(xmax >= 0.0f && xmin <= (float)a.W && ymax >= 0.0f && ymin <= (float)a.H)) break; // wholly outside the image (or not finite)
        // pixel columns / rows whose centre i + 0.5 lies in the box; the operands are clamped to the image first, so the conversions are small
        const int px0 = max(0, f2i(ceilf(fmaxf(xmin, 0.0f) - 0.5f - BOX_MARGIN))), px1 = min(a.W - 1, f2i(floorf(fminf(xmax, (float)a.W) - 0.5f + BOX_MARGIN)));
        const int py0 = max(0, f2i(ceilf(fmaxf(ymin, 0.0f) - 0.5f - BOX_MARGIN))), py1 = min(a.H - 1, f2i(floorf(fminf(ymax, (float)a.H) - 0.5f + BOX_MARGIN)));
        if (px1 < px0 || py1 < py0) break; // a sliver between pixel centres
        const int rminx = px0 / TS_TILE, rminy = py0 / TS_TILE, rmaxx = px1 / TS_TILE + 1, rmaxy = py1 / TS_TILE + 1; // <= grid_x, grid_y

        const f3 n = cross(sub(v2, v1), sub(v3, v1));
        rec[0] = s1.x; rec[1] = s1.y; rec[2] = s2.x; rec[3] = s2.y; rec[4] = s3.x; rec[5] = s3.y;
        rec[6] = n.x; rec[7] = n.y; rec[8] = n.z;
        rec[9] = dot(n, v1);
        rec[10] = fminf(fminf(v1.z, v2.z), v3.z);
        rec[11] = fmaxf(fmaxf(v1.z, v2.z), v3.z);
        out_key = rec[10];
        out_tiles = (uint32_t)(rmaxx - rminx) * (uint32_t)(rmaxy - rminy);
        out_rect = {(uint32_t)rminx | ((uint32_t)rminy << 16), (uint32_t)rmaxx | ((uint32_t)rmaxy << 16)};
    } while (false);

    g.tiles_touched[f] = out_tiles;
    g.rect[f] = out_rect;
    g.depth[f] = out_key;
    float4 *r = g.rec + 4 * (size_t)f;
    r[0] = make_float4(rec[0], rec[1], rec[2], rec[3]);
    r[1] = make_float4(rec[4], rec[5], rec[6], rec[7]);
    r[2] = make_float4(rec[8], rec[9], rec[10], rec[11]);
    r[3] = make_float4(rec[12], rec[13], rec[14], rec[15]);
}
} // namespace

void ts_launch_mesh_preprocess(const MeshArgs &a, const GeometryStateView &g, hipStream_t s)
{
    if (a.F <= 0) return;
    hipLaunchKernelGGL(mesh_preprocess_kernel, dim3((unsigned)((a.F + 255) / 256)), dim3(256), 0, s, a, g);
}
