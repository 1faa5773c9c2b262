/*
 * ts_simplify.h -- C ABI of libts_simplify.so: an indexed triangle mesh made smaller by vertex clustering on a uniform grid with quadric
 * error placement (Lindstrom), and the sweep that removes the duplicate faces clustering leaves behind.
 * diff_recon_hip/mesh_simplify.py builds cluster_labels, place_clusters, unique_faces, simplify_mesh and drop_small_pieces on it
 * (DESIGN.md 16i).  The numbering and the face remap between the calls are ts_weld.h's (ts2d_weld_compact, ts2d_weld_remap_faces).
 *
 * A library of its own, beside libts2d.so, libts_geom.so, libts_bvh.so, libts_ray.so, libts_volume.so and libts_color.so: the export lists
 * of all six are closed.  It links the product's radix sort object and keeps its own error text.  The error codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, a cell that is zero, negative, NaN or infinite, an origin that is NaN
 * or infinite, a lambda that is negative, NaN or infinite, a mode other than the two below, attributes with C outside 1 .. 8 (C is ignored
 * when attributes is NULL), a null required pointer, a workspace below tsq_workspace_bytes(V, F) return TS2D_ERR_INVALID with the text
 * in tsq_last_error(); more than 715827882 faces (3 F sort slots) is TS2D_ERR_CAPACITY.  V == 0 (F == 0 for tsq_unique_faces) is a no-op
 * that returns TS2D_OK, except that counts is still overwritten.
 *
 * The result is a pure function of the input: one pass over the data, no priority queue, no floating-point atomics, no dependence on
 * thread order.  All arithmetic is float64 on the fp32 inputs widened, every operation rounded (the unit is built with
 * -ffp-contract=off), written operation by operation in tests/ref_mesh_simplify.py.  There is no square root anywhere.
 *
 * Cells.  Per axis g = ((double)x - (double)o) / (double)cell and c = floor(g).  A vertex is VALID iff its three coordinates are finite
 * and 0 <= c < 2^21 on every axis; its key is cz << 42 | cy << 21 | cx.
 * Clusters (tsq_cluster_labels).  Valid vertices with equal keys form a cluster; label[i] = the smallest index in i's cluster.  An invalid
 * vertex is its own cluster (label[i] = i).  Numbering is ts2d_weld_compact's: clusters ranked by ascending label, remap[i] = the rank of
 * label[i], V' = the number of clusters.
 *
 * Placement (tsq_place).  `remap` may come from any source that numbers the clusters as above (the labels themselves are not needed: a
 * cluster is the set of vertices with one remap value, its members taken in ascending index order, its head the first of them, which is
 * its label).  The head decides the cluster's cell c and whether the cluster is valid; an invalid cluster's row is its head's position
 * bit for bit.  For a valid cluster:
 *   frame     cc = (double)o + (double)cell ((double)c + 0.5) per axis.
 *   mean      m = the float64 sum of (v - cc) over the members in ascending index order (starting from 0), divided by (double)count.
 *   quadric   a face contributes iff its three indices lie in [0, V) and its nine coordinates are finite; it contributes ONCE to each
 *             distinct cluster among its VALID vertices, faces in ascending face index.  In the cluster's frame, p_k = v_k - cc,
 *             e1 = p1 - p0, e2 = p2 - p0: nx = e1y e2z - e1z e2y, ny = e1z e2x - e1x e2z, nz = e1x e2y - e1y e2x,
 *             d = -((nx p0x + ny p0y) + nz p0z); the nine accumulators a00 a01 a02 a11 a12 a22 b0 b1 b2 (from 0) gain nx nx, nx ny, nx nz,
 *             ny ny, ny nz, nz nz, nx d, ny d, nz d.  The normal is unnormalised (area^2 weights).
 *   TSQ_PLACE_MEAN     x = m.
 *   TSQ_PLACE_QUADRIC  tr = (a00 + a11) + a22.  If tr is finite and > 0: mu = (double)lambda tr is added to a00, a11, a22; r = mu m - b;
 *             c00 = a11 a22 - a12 a12, c01 = a02 a12 - a01 a22, c02 = a01 a12 - a02 a11, c11 = a00 a22 - a02 a02, c12 = a01 a02 - a00 a12,
 *             c22 = a00 a11 - a01 a01; det = (a00 c00 + a01 c01) + a02 c02.  If det is finite and > 0, x_i = ((c_i0 r0 + c_i1 r1) + c_i2 r2)
 *             / det (c symmetric); if all three x_i are finite that is x.  Any failed test gives x = m.
 *   clamp     each axis to [-0.5 cell, 0.5 cell] in float64 (min(max(x, -half), half)); the row is (float)(cc + x).
 * A vertex therefore never leaves its cell: that is the bound on displacement, and what keeps an ill-conditioned solve harmless.
 *   attributes  per cluster (valid or not) and channel: the float64 sum (from 0) of the widened values of the members with attr_valid != 0
 *             (all members when attr_valid is NULL) in ascending index order, divided by their count, rounded to fp32; out_valid = 1 iff
 *             the count is positive, otherwise the row is 0 and out_valid 0.  NaNs propagate.
 *   member_count[r] = the number of members of cluster r.
 * All outputs of tsq_place have V rows; rows V' .. V - 1 are zero, as ts2d_weld_compact leaves them.
 *
 * Duplicate faces (tsq_unique_faces).  `faces` are remapped faces on V vertices (any bound on the new indices will do; the sort uses only
 * the bits V needs).  A face TAKES PART iff keep_in[f] != 0, its three indices lie in [0, V) and are pairwise distinct.  Each such face is
 * rotated so that its smallest index comes first, keeping its orientation; among the faces with equal rotated triples only the smallest
 * face index survives: keep_out[f] = 1 for it, 0 for every other face.  Opposite-oriented twins are both kept (the two sides of a
 * collapsed sheet).  counts = {duplicates, flaps}: the faces that took part and did not survive, and the survivors whose reversed triple
 * also survives.  keep_out may not alias keep_in.
 *
 * Cost.  Every sum above is sequential by definition, so a cluster is ONE thread's work in tsq_place: the cost of the call is linear in
 * the largest cluster (members plus incident faces), and a grid with one cell over the whole mesh is a serial walk of it.  `cell` is
 * meant to be far below the mesh's extent.  The sorts are the product's stable LSD radix sort: 8 passes over V pairs for the labels
 * (the key's 63 bits and the invalid flag), the bits of V for the placement's two sorts (V and 3 F pairs) and three times that over F
 * pairs for the duplicate sweep.
 *
 * Purity (DESIGN.md "Purity of the entry points").  One workspace serves all three calls in any order and may hold anything on entry;
 * label, all V rows of out_vertices, out_attributes, out_valid and member_count, keep_out and counts are overwritten whatever they held;
 * no byte outside tsq_workspace_bytes(V, F) or an output's extent is written.
 */
#ifndef TS_SIMPLIFY_H
#define TS_SIMPLIFY_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSQ_PLACE_MEAN 0
#define TSQ_PLACE_QUADRIC 1
#define TSQ_MAX_CHANNELS 8
#define TSQ_CELL_BITS 21 /* cell indices per axis: 0 .. 2^21 - 1 */

/* The text of the calling thread's last error of this library. */
const char *tsq_last_error(void);

/* Bytes of device workspace that serve every call below for V vertices and F faces.  Monotonic in V and in F. */
size_t tsq_workspace_bytes(int32_t V, int32_t F);

/* vertices: V*3 floats; label: V int32. */
int tsq_cluster_labels(int32_t V, const float *vertices, float ox, float oy, float oz, float cell, int32_t *label, void *workspace,
                       size_t workspace_bytes, void *stream);

/* vertices: V*3 floats; faces: F*3 int32 (NULL with F == 0); remap: V int32; attributes: V*C floats or NULL; attr_valid: V bytes or
 * NULL; out_vertices: V*3 floats; out_attributes: V*C floats and out_valid: V bytes (both required with attributes, ignored without);
 * member_count: V int32.  F is at most 715827882 (3 F incidence slots). */
int tsq_place(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const int32_t *remap, float ox, float oy,
              float oz, float cell, float lambda, int32_t mode, const float *attributes, const uint8_t *attr_valid, int32_t C,
              float *out_vertices, float *out_attributes, uint8_t *out_valid, int32_t *member_count, void *workspace,
              size_t workspace_bytes, void *stream);

/* faces: F*3 int32; keep_in, keep_out: F bytes; counts: two 64-bit device words {duplicates, flaps}, overwritten. */
int tsq_unique_faces(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep_in, uint8_t *keep_out, unsigned long long *counts,
                     void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_SIMPLIFY_H */
