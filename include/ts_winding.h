/*
 * ts_winding.h -- C ABI of libts_winding.so: the GENERALISED WINDING NUMBER of a triangle mesh at a point (Jacobson, Kavan and
 * Sorkine-Hornung 2013), summed on the index that the build call of ts_bvh.h wrote with one far-field term per node (Barill, Dickson,
 * Schmidt, Levin and Jacobson 2018, first order), and the signed distance that follows from it and the unsigned distance of ts_bvh.h's
 * closest-point call.  diff_recon_hip/mesh_winding.py builds the inside test of OPEN meshes on it: where the crossing
 * counts of ts_inside.h need a closed surface, w(q) = sum over the faces T of Omega_T(q) / 4 pi, Omega_T the signed solid angle of T seen
 * from q, is an integer away from a closed surface and degrades smoothly at a hole; w >= 1/2 is a robust "inside".
 *
 * A library of its own, the fourteenth: the export lists of the other thirteen are closed.  libts_winding.so links the same radix sort
 * (csrc/radix_sort.hip) and the same front half of the box searches (csrc/ts_knn_front.h), reads the index through the layout header it
 * shares with the build (csrc/ts_bvh_layout.h) and keeps its own error text.  The error codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, a null required pointer, an index buffer below the index size of F (the
 * size query of ts_bvh.h; computed here from the layout header), a moments or leaf-face buffer or a workspace below its size query, beta NaN
 * or below 1 return TS2D_ERR_INVALID with the text in the last-error call of this header.  Counts are int32_t, at most 2^31 - 1025;
 * F > 2^24 - 1 returns TS2D_ERR_CAPACITY (the overflow bound below).
 *
 * Arithmetic.  Pure functions of their input; the unit is built with -ffp-contract=off.  Everything is float64 on the fp32 coordinates
 * widened to double, every operation rounded; dot, cross, min2 and max2 are those of ts_bvh.h and ts_ray.h (u.v = (ux*vx + uy*vy) + uz*vz;
 * of two equal values the first stays), PI is the double nearest pi (0x400921FB54442D18).  Eligible faces are ts_bvh.h's: the index holds no
 * other.  Every sum over faces or nodes is a 64-BIT INTEGER SUM OF QUANTISED TERMS, in units of 2^-38 turns: the result does not depend on
 * the order of the walk or on which queries share a wave.
 *
 * Face term.  For the query q and the face (A, B, C): a = A - q, b = B - q, c = C - q; la = sqrt(a.a), lb, lc likewise; det = a.(b x c);
 *   den = ((la*lb)*lc + (a.b)*lc) + ((b.c)*la + (c.a)*lb);  theta = det == 0 ? 0 : atan2(det, den);  term = llrint((theta / PI) * 2^37),
 * round half to even (theta is HALF the solid angle: van Oosterom and Strackee).  det == 0, a query in the plane of the face, counts 0: the
 * mean of the two sides.  A point inside an outward-facing closed mesh has w = +1, the sign of ts_inside.h's w.
 *
 * Node moments (the moments call).  One record of 8 doubles per node of every level, numbered like the boxes of the index (level 0, the
 * leaves, first): [Nx, Ny, Nz, px, py, pz, R2, S].  A leaf node sums over its slots j = 0..7 in slot order, those with id >= 0:
 * n = 0.5 * ((B - A) x (C - A)) per component, ar = sqrt(n.n), g = ((A + B) + C) / 3 per component; N += n, S += ar, M += ar*g per
 * component, each sum starting from +0.  An inner node sums N, S and M of its children in index order; a child without an eligible face
 * holds zeros.  Then p = S > 0 ? M / S : 0 per component, and R2 = S > 0 ? (ex*ex + ey*ey) + ez*ez : +inf with e = max2(p - lo, hi - p)
 * per axis, lo and hi the node's box: every face of the node lies within sqrt(R2) of p.  `leaf_faces`, when not NULL, receives the face id
 * of every leaf slot, ceil(F / 8) * 8 int32, -1 for padding: with it a reference restates the tree, whose boxes are the exact fp32 minima
 * and maxima of the slots' vertices.
 *
 * Query (the winding call).  beta2 = beta*beta, rounded once, on the host.  Per query, depth first from the root: a node with the empty
 * box is skipped.  With r = p - q and d2 = r.r the node is ACCEPTED iff S > 0 and d2 > beta2 * R2; it then contributes
 *   llrint((((N.r) / (d2 * sqrt(d2))) / (4*PI)) * 2^38)
 * and is not descended.  A leaf node that is not accepted contributes the face terms of its slots with id >= 0.  Any other node is
 * replaced by its children.  wq[i] is the int64 sum; terms[2i], terms[2i+1] (terms may be NULL) are the faces evaluated and the nodes
 * accepted.  beta = +inf accepts nothing: the exact sum, equal to brute force over the eligible faces whatever the tree.  A query with a NaN
 * or infinite coordinate gets wq = INT64_MIN and terms = -1, -1.  F == 0 (bvh and moments may be NULL) or no eligible face: zeros.  Q == 0
 * is the no-op.
 *
 * Finite.  For finite fp32 input every intermediate is finite: the largest are (la*lb)*lc and det, below 2e117, the moment sums, below
 * 2^24 * 1e117, and n.n, below 1e157.  An accepted node has R2 > 0 and d2 > beta2 * R2 > 0: nothing is divided by zero.  The only infinities
 * are R2 of a node without area, which is never accepted, and beta2 of the exact form, likewise.
 *
 * Overflow.  A face term is at most 2^37 units in magnitude (|theta| <= pi).  An accepted node that holds m faces, each within sqrt(R2)
 * of p and hence of area at most 2 R2, has |N| <= 2 m R2 and contributes below 2 m R2 / (4 pi d2) < m / (2 pi beta^2) turns, with
 * beta >= 1 below 2^36 m units.  A face is counted once, by itself or within one accepted node: the magnitudes sum below 2^37 F < 2^61
 * for F <= 2^24 - 1, and the int64 sum cannot wrap, whatever the order.
 *
 * Cost.  The queries are Morton-sorted, one wave owns 64 consecutive sorted queries and walks the tree once for all of them: a node is
 * entered when some lane of the wave has accepted none of its ancestors; a lane that accepted one sits out below it.
 *
 * Signed distance (the sign-distance call).  One thread per point, on dist2 (what tsb_closest wrote for the point), wq (what the winding
 * call wrote for it) and a threshold in units:
 *   dist2 == 0                               out = +0, decided = 1, whatever wq says
 *   dist2 NaN or +inf, or wq == INT64_MIN    out = NaN (0x7FC00000), decided = 0
 *   otherwise                                out = (float)sqrt(dist2), negated iff wq >= threshold, decided = 1
 * sqrt is the correctly rounded float64 one.  Negative inside is ts_inside.h's and TSDFVolume's convention.
 *
 * Purity (DESIGN.md "Purity of the entry points").  The workspace, the moments, leaf_faces and all outputs may hold anything on entry;
 * moments, leaf_faces, wq, terms, out and decided are overwritten in full; no byte outside a size query or an output's extent is written.
 */
#ifndef TS_WINDING_H
#define TS_WINDING_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The text of the calling thread's last error of this library. */
const char *tsn_last_error(void);

/* Bytes of the node moments of a mesh of F faces: 64 per node of the index.  Monotonic. */
size_t tsn_moments_bytes(int32_t F);

/* Bytes of the leaf-face table of a mesh of F faces: 4 * 8 * ceil(F / 8).  Monotonic. */
size_t tsn_leaf_faces_bytes(int32_t F);

/* bvh: the index of the F faces; moments: at least the moments size of F; leaf_faces: at least the leaf-face size of F, or NULL.  F == 0
 * is the no-op. */
int tsn_moments(int32_t F, const void *bvh, size_t bvh_bytes, double *moments, size_t moments_bytes, int32_t *leaf_faces,
                size_t leaf_faces_bytes, void *stream);

/* Bytes of device workspace of a winding-number query of Q points.  Monotonic. */
size_t tsn_winding_workspace_bytes(int32_t Q);

/* points: Q*3 floats; beta: >= 1, +inf for the exact sum; bvh, moments: the index of the F faces and what the moments call wrote for it;
 * wq: Q int64; terms: Q*2 int32 or NULL. */
int tsn_winding(int32_t Q, const float *points, double beta, int32_t F, const void *bvh, size_t bvh_bytes, const double *moments,
                size_t moments_bytes, int64_t *wq, int32_t *terms, void *workspace, size_t workspace_bytes, void *stream);

/* dist2: Q doubles; wq: Q int64; threshold: in units of 2^-38 turns; out: Q floats; decided: Q bytes. */
int tsn_sign_distance(int32_t Q, const double *dist2, const int64_t *wq, int64_t threshold, float *out, uint8_t *decided, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_WINDING_H */
