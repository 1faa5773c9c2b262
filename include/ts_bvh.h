/*
 * ts_bvh.h -- C ABI of libts_bvh.so: a bounding-volume hierarchy over the TRIANGLES of a mesh and the exact closest-point query on it.
 * diff_recon_hip/mesh_surface.py builds the sample-to-SURFACE scores of an exported mesh on it; the point-to-point scores of
 * ts_geom.h carry the sampling spacing, these do not.
 *
 * A library of its own, beside libts2d.so and libts_geom.so: the export lists of both are closed.  libts_bvh.so links the same radix sort
 * (csrc/radix_sort.hip) and the same front half of the box searches (csrc/ts_knn_front.h) and keeps its own error text.  The error codes are
 * ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, a null required pointer, a workspace or an index buffer below its size
 * query return TS2D_ERR_INVALID with the text in the last-error call of this header.  Counts are int32_t, at most 2^31 - 1025.
 *
 * Build.  Writes the index of the mesh (vertices: V*3 floats, faces: F*3 int32, keep: F bytes or NULL) into `bvh`: a copy of the eligible
 * faces' fp32 coordinates in Morton order of their centroids, in leaves of 8, and the boxes of an implicit 8-ary tree above the leaves.  The
 * index is a pure function of (V, F, vertices, faces, keep) and is only meaningful to the closest call with the same F.  F == 0 is the
 * no-op (nothing is written, bvh may be NULL).
 *
 * Closest point.  A pure function of its input; the unit is built with -ffp-contract=off.  Everything below is float64, computed from the
 * fp32 coordinates widened to double, with every operation rounded.
 *   eligible     a face is eligible iff its keep byte is non-zero (or keep is NULL), its three indices lie in [0, V) and its nine
 *                coordinates are finite.  Zero-area faces ARE eligible: they are segments or points and the formula handles them.
 *   dot          u.v = (ux*vx + uy*vy) + uz*vz;  cross u x v = (uy*vz - uz*vy, uz*vx - ux*vz, ux*vy - uy*vx);  clamp01(x) = x < 0 ? 0 : (x > 1 ? 1 : x).
 *   segment      seg(p0, p1): d = p1 - p0, w = q - p0, den = d.d, t = den == 0 ? 0 : clamp01((w.d) / den), r = w - t*d per component,
 *                value r.r, point p0 + t*d per component.
 *   interior     e1 = b - a, e2 = c - a, n = e1 x e2, nn = n.n, s = (q - a).n.  It counts only when nn > 0 and the three side tests
 *                ((b - a) x (q - a)).n, ((c - b) x (q - b)).n, ((a - c) x (q - c)).n are all >= 0.  Value (s*s)/nn, point q - (s/nn)*n per component.
 *   distance     D(q, T) of q to the face T = (a, b, c) is the minimum of the four candidates seg(a, b), seg(b, c), seg(c, a), interior, taken in
 *                this order, the first smallest winning.  D is finite for all finite fp32 inputs (the largest intermediate is s*s, below 1e236).
 *   box bound    L(q, box) = (ex*ex + ey*ey) + ez*ez with, per axis, e = lo - q when that is > 0, else q - hi when that is > 0, else 0.
 *   reported     D'(q, T) = D(q, T) when D(q, T) > L(q, AABB(T)), else L(q, AABB(T)): the larger of the two.  AABB(T) is the per-axis
 *                minimum and maximum of the three fp32 vertices.  Mathematically D' = D: a distance is never below the distance to the box.
 *                Numerically it is what makes the pruned search EQUAL to brute force: L is monotone under box inclusion, rounding included, so
 *                L(q, B) <= D'(q, T) for every node box B that contains AABB(T), and a traversal that skips a node only when L(q, B) > best
 *                (strict) returns the brute-force argmin, ties included.
 *   selection    face[i] = the eligible face with the smallest D', ties to the SMALLEST FACE INDEX; dist2[i] = that D', bit for bit;
 *                point[3i .. 3i+2] = the winning candidate's point rounded to fp32.
 *   no face      no eligible face (F == 0 included): face[i] = -1, dist2[i] = +inf, point = NaN.
 *   bad query    a query with a NaN or infinite coordinate: face[i] = -1, dist2[i] = NaN, point = NaN.
 *   Q == 0 is the no-op.
 *   `vertices` and `faces` are the arrays the index was built from; the query reads the index's own copy of the coordinates.
 *
 * Cost.  The queries are Morton-sorted; one wave owns 64 consecutive sorted queries and walks the tree once for all of them, entering a node
 * when some lane's bound does not exceed that lane's best.  `leaf_visits` gains the number of (wave, leaf) visits.
 *
 * Purity (DESIGN.md "Purity of the entry points").  `bvh`, both workspaces and all outputs may hold anything on entry; face, dist2 and point
 * are overwritten in full; `leaf_visits` is a caller-cleared accumulator; no byte outside the size queries or an output's extent is written;
 * the build writes every slot of `bvh` that a query reads, padding slots included.
 */
#ifndef TS_BVH_H
#define TS_BVH_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The text of the calling thread's last error of this library. */
const char *tsb_last_error(void);

/* Bytes of the index of a mesh of F faces.  Monotonic. */
size_t tsb_bvh_bytes(int32_t F);

/* Bytes of device workspace of a build over F faces.  Monotonic. */
size_t tsb_build_workspace_bytes(int32_t F);

/* vertices: V*3 floats; faces: F*3 int32; keep: F bytes or NULL (all faces); bvh: at least the index size of F.  F == 0 is the no-op. */
int tsb_build(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, void *bvh, size_t bvh_bytes,
              void *workspace, size_t workspace_bytes, void *stream);

/* Bytes of device workspace of a query of Q points.  Monotonic. */
size_t tsb_closest_workspace_bytes(int32_t Q);

/* queries: Q*3 floats; bvh: what the build wrote for (V, F, vertices, faces); face: Q int32; dist2: Q doubles; point: Q*3 floats or NULL.
 * leaf_visits: one 64-bit device word that the caller cleared, or NULL. */
int tsb_closest(int32_t Q, const float *queries, int32_t V, int32_t F, const float *vertices, const int32_t *faces, const void *bvh,
                size_t bvh_bytes, int32_t *face, double *dist2, float *point, unsigned long long *leaf_visits, void *workspace,
                size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_BVH_H */
