/*
 * ts_weld.h -- C ABI of vertex welding and edge topology in libts2d.so: turns the triangle soup that mesh_from_triangles and
 * RawTriangle.saveGLB produce (three private vertices per triangle) into an indexed mesh with shared vertices, and says what
 * surface the result is.  The counterpart of the reference's saveGLB(..., process=True) (src/diff_recon/models/raw_triangle.py:183-207,
 * trimesh's vertex merging), defined here so that the result is a pure function of the input.
 *
 * Semantics.  All distance arithmetic is fp32 with every operation rounded (the unit is built with -ffp-contract=off).
 *   adjacent     vertices i != j are adjacent iff all six coordinates are finite and, with dx = xi - xj, dy = yi - yj, dz = zi - zj,
 *                (dx*dx + dy*dy) + dz*dz <= eps*eps.  The expression is symmetric bit for bit.  eps == 0 merges exactly equal positions
 *                (+0 and -0 are equal).  A vertex with a NaN or infinite coordinate is adjacent to nothing and does not shape the search grid.
 *   clusters     the connected components of that relation (single linkage: a row of points each 0.75 eps from the next is ONE cluster);
 *                label[i] = the smallest index in i's cluster.  Defined by the mathematics, not by thread order.
 *   numbering    clusters are ranked by ascending label; remap[i] = the rank of label[i]; V' = the number of clusters.  Vertices that no
 *                face names are kept.
 *   position     TS2D_WELD_FIRST: the position of vertex `label`, copied bit for bit.  TS2D_WELD_MEAN: the float64 sum of the members in
 *                ascending index order (starting from the first member), divided by the count in float64, rounded to fp32.
 *   faces        new[f][k] = remap[old[f][k]]; keep[f] = 0 iff an index lies outside [0, V) (the new row is then -1 -1 -1) or two of the new
 *                indices are equal.  Nothing is read out of bounds for any face contents.  Duplicate faces are NOT removed.
 *   topology     every kept face whose indices lie in [0, V) contributes three undirected edges (min, max); the census counts the distinct
 *                edges and how many of them are used by exactly one face (boundary), exactly two (manifold), three or more (non-manifold).
 *                A mesh with reversed back twins doubles every edge: pass front faces only.
 *
 * Cost.  The radius search is knn.hip's box search: Morton-sorted points in boxes of 1024, one workgroup per box, about 1024 x 1024 / 2
 * pair tests per box it visits.  It visits the boxes whose box-to-box bound is within eps, so an input in which most vertices lie within
 * eps of each other makes every box visit every other box: QUADRATIC in V.  The weld is built for eps far below the mesh's extent.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so
 * the calls can be captured in a graph.  Argument checks are decided before any HIP call: a negative count, a non-finite or negative eps,
 * a null required pointer or a workspace below ts2d_weld_workspace_bytes(V, F) return TS2D_ERR_INVALID with the text in ts2d_last_error().
 * V == 0 (F == 0 for the two calls that sweep faces) is a no-op that returns TS2D_OK.  `keep` arrays hold one byte per face (0 / 1).
 * The entry points carry the library's ts2d_ prefix like ts_mesh.h's.
 *
 * Purity (DESIGN.md "Purity of the entry points"): one workspace serves the whole chain in any order and may hold anything on entry;
 * label, remap, all V rows of out_vertices (rows V' .. V-1 zero), count, out_faces, keep and counts are overwritten whatever they held;
 * `box_visits` is a caller-cleared accumulator; no byte outside ts2d_weld_workspace_bytes(V, F) or an output's extent is written.
 */
#ifndef TS_WELD_H
#define TS_WELD_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS2D_WELD_FIRST 0
#define TS2D_WELD_MEAN 1

/* Bytes of device workspace that serve every call below for V vertices and F faces.  Monotonic in V and in F. */
size_t ts2d_weld_workspace_bytes(int32_t V, int32_t F);

/* label[i] = the smallest index of i's cluster.  vertices: V*3 floats; label: V int32. */
int ts2d_weld_labels(int32_t V, const float *vertices, float eps, int32_t *label, void *workspace, size_t workspace_bytes, void *stream);

/* The same; `box_visits` (one 64-bit device word that the caller cleared, or NULL) additionally receives the number of (workgroup, box)
 * visits of the search, own boxes included (tools/bench_mesh_weld.py). */
int ts2d_weld_labels_counted(int32_t V, const float *vertices, float eps, int32_t *label, unsigned long long *box_visits, void *workspace,
                             size_t workspace_bytes, void *stream);

/* The same union-find fed by face edges: label[i] = the smallest vertex index that i is joined to along the edges of the kept faces
 * (keep == NULL: all faces) whose indices lie in [0, V).  A vertex that no such face names is its own label.  The workspace is not used. */
int ts2d_weld_face_components(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep, int32_t *label, void *workspace,
                              size_t workspace_bytes, void *stream);

/* Numbering and welded positions from labels.  remap: V int32; out_vertices: V*3 floats of which rows 0 .. V'-1 are the welded positions and
 * the rest 0; count: one device int32 that receives V'.  mode: TS2D_WELD_FIRST or TS2D_WELD_MEAN. */
int ts2d_weld_compact(int32_t V, const int32_t *label, const float *vertices, int32_t mode, int32_t *remap, float *out_vertices,
                      int32_t *count, void *workspace, size_t workspace_bytes, void *stream);

/* Face remap and keep mask.  faces, out_faces: F*3 int32; keep: F bytes. */
int ts2d_weld_remap_faces(int32_t V, int32_t F, const int32_t *faces, const int32_t *remap, int32_t *out_faces, uint8_t *keep, void *stream);

/* counts: four 64-bit device words {edges, boundary, manifold, nonmanifold}, overwritten.  keep may be NULL (all faces).
 * F is at most 715827882 (3 F edge slots). */
int ts2d_weld_edge_census(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep, unsigned long long *counts, void *workspace,
                          size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_WELD_H */
