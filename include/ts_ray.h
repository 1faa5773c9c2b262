/*
 * ts_ray.h -- C ABI of libts_ray.so: the exact FIRST HIT of a ray on the triangles of a mesh, found on the index that the build call of
 * ts_bvh.h wrote.  diff_recon_hip/mesh_ray.py builds ray casting, pixel-centre camera rays, point visibility and the visibility-aware
 * surface scores on it.
 *
 * A library of its own, beside libts2d.so, libts_geom.so and libts_bvh.so: the export lists of all three are closed.  libts_ray.so links the
 * same radix sort (csrc/radix_sort.hip) and the same front half of the box searches (csrc/ts_knn_front.h), reads the index through the
 * layout header it shares with the build (csrc/ts_bvh_layout.h) and keeps its own error text.  The error codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, a null required pointer, an index buffer below the index size of F (the
 * size query of ts_bvh.h; computed here from the layout header), a workspace below its size query, tmin or tmax NaN, tmin > tmax, cull_back
 * other than 0 or 1 return TS2D_ERR_INVALID with the text in the last-error call of this header.  Counts are int32_t, at most 2^31 - 1025.
 *
 * `bvh` is what tsb_build (ts_bvh.h) of the same tree wrote for (V, F, vertices, faces, keep); the cast reads the index's own copy of the
 * coordinates and needs neither array again.  Q == 0 is the no-op.  F == 0: nobody hits anything (bvh may be NULL).
 *
 * First hit.  A pure function of its input; the unit is built with -ffp-contract=off.  Everything below is float64, computed from the fp32
 * inputs widened to double, with every operation rounded.  min(x, y) is y < x ? y : x and max(x, y) is y > x ? y : x: of a +0 and a -0 the
 * first stays.  Ray i has origin o = origins[3i..], direction d = directions[3i..] (any length: t counts in units of d) and the upper limit
 * hi = t_limit ? min(tmax, (double)t_limit[i]) : tmax.
 *   bad ray      any component of o or d is NaN or infinite, d == (0, 0, 0), or t_limit[i] is NaN: face = -1, t = NaN, bary = NaN, side = 0.
 *   triangle     the watertight test of Woop, Benthin and Wald ("Watertight Ray/Triangle Intersection", JCGT 2013).  kz = the index of the
 *                largest |d[k]|, ties to the smallest index; kx = (kz + 1) % 3, ky = (kx + 1) % 3, the two swapped when d[kz] < 0;
 *                Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].  Per vertex p of (a, b, c): P = p - o per component,
 *                Px = P[kx] - Sx * P[kz], Py = P[ky] - Sy * P[kz], Pz = Sz * P[kz] (A, B, C for a, b, c).
 *                U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax, det = (U + V) + W.
 *                The face is a CANDIDATE iff det != 0 and not (one of U, V, W is < 0 and one is > 0); with cull_back also det > 0.
 *                tt = ((U * Az + V * Bz) + W * Cz) / det.
 *                The two faces of a shared edge compute the same two products, subtracted the other way round: the same value with the other
 *                sign, so a ray never slips between them.  An edge value of exactly 0 counts for both faces; the smaller index wins.
 *   slab         of a box (lo, hi): per axis k with d[k] != 0, ta = (lo - o) / d, tb = (hi - o) / d, near = min(ta, tb), far = max(ta, tb),
 *                padded near' = near - |near| * 2^-40, far' = far + |far| * 2^-40.  An axis with d[k] == 0 PASSES iff lo <= o <= hi and
 *                contributes (-inf, +inf).  tn = max(max(near'x, near'y), near'z), tf = min(min(far'x, far'y), far'z).  The box is CROSSED
 *                iff every zero-direction axis passes, tn <= tf, tf >= tmin and tn <= hi.  No intermediate is NaN or infinite otherwise:
 *                |lo - o| < 7e38 and |d| >= 1.4e-45, the quotients stay below 5e83.
 *   reported     the face T is HIT iff it is eligible in the build's sense (ts_bvh.h), a candidate, AABB(T) is crossed and
 *                t' = max(tt, tn(AABB(T))) lies in [tmin, hi].  AABB(T) is the per-axis minimum and maximum of the three fp32 vertices.
 *                face[i] = the hit face with the smallest t', ties to the SMALLEST FACE INDEX; t[i] = that t', bit for bit;
 *                bary[3i .. 3i+2] = (U / det, V / det, W / det) rounded to fp32: the weights of a, b and c; side[i] = +1 when det > 0, else -1.
 *                Mathematically t' = tt: a hit is never nearer than where the ray enters the face's box.  Numerically it is what makes the
 *                pruned search EQUAL to brute force.  Every operation of the slab interval is monotone, rounding included: for a node box
 *                B that contains AABB(T) = A, tn(B) <= tn(A) <= t' and tf(B) >= tf(A), so a crossed A implies a crossed B, and a traversal
 *                that skips a node only when it is not crossed or when tn(B) > best (strict) returns the brute-force result, ties included.
 *                The 2^-40 padding is 2^12 times the rounding of the two operations behind near and far: it keeps a true hit from being
 *                refused by its own box.  Zero-area faces are never hit (det == 0).
 *   side         det > 0 is a hit on the FRONT: ((b - a) x (c - a)) . d < 0, the ray runs against the normal of the counter-clockwise face.
 *   no hit       (F == 0 and no eligible face included): face = -1, t = +inf, bary = NaN, side = 0.
 *
 * Cost.  The rays are Morton-sorted by their ORIGINS (the key is the origin alone: the rays of one camera share it and stay in pixel order,
 * which is coherent already; the result does not depend on the key).  One wave owns 64 consecutive sorted rays and walks the tree once for
 * all of them, entering a node when some lane crosses it with tn <= that lane's best.  `leaf_visits` gains the number of (wave, leaf) visits.
 *
 * Purity (DESIGN.md "Purity of the entry points").  The workspace and all outputs may hold anything on entry; face, t, bary and side are
 * overwritten in full; `leaf_visits` is a caller-cleared accumulator; no byte outside the size query or an output's extent is written.
 */
#ifndef TS_RAY_H
#define TS_RAY_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The text of the calling thread's last error of this library. */
const char *tsr_last_error(void);

/* Bytes of device workspace of a cast of Q rays.  Monotonic. */
size_t tsr_cast_workspace_bytes(int32_t Q);

/* origins, directions: Q*3 floats; t_limit: Q floats or NULL; cull_back: 0 or 1; bvh: the index of the F faces; face: Q int32; t: Q doubles;
 * bary: Q*3 floats or NULL; side: Q bytes or NULL; leaf_visits: one 64-bit device word that the caller cleared, or NULL. */
int tsr_cast(int32_t Q, const float *origins, const float *directions, const float *t_limit, double tmin, double tmax, int32_t cull_back,
             int32_t F, const void *bvh, size_t bvh_bytes, int32_t *face, double *t, float *bary, int8_t *side,
             unsigned long long *leaf_visits, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_RAY_H */
