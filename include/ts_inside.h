/*
 * ts_inside.h -- C ABI of libts_inside.so: ALL hits of a ray on the triangles of a mesh, counted in half crossings on the index that the
 * build call of ts_bvh.h wrote, and the signed distance that follows from such a count and the unsigned distance of ts_bvh.h's closest-point
 * call.  diff_recon_hip/mesh_inside.py builds the inside test, the winding number, the signed distance, the distance volume of a mesh,
 * remeshing and the volumetric IoU of two meshes on it.
 *
 * A library of its own, the thirteenth: the export lists of the other twelve are closed.  libts_inside.so links the same radix sort
 * (csrc/radix_sort.hip) and the same front half of the box searches (csrc/ts_knn_front.h), reads the index through the layout header it
 * shares with the build (csrc/ts_bvh_layout.h), evaluates a ray with the very text that libts_ray.so evaluates it with
 * (csrc/ts_ray_tests.h) and keeps its own error text.  The error codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, a null required pointer, an index buffer below the index size of F (the
 * size query of ts_bvh.h; computed here from the layout header), a workspace below its size query, tmin or tmax NaN, tmin > tmax,
 * shared_direction, rule or only_undecided out of range return TS2D_ERR_INVALID with the text in the last-error call of this header.  Counts
 * are int32_t, at most 2^31 - 1025; F > 2^30 - 1 returns TS2D_ERR_CAPACITY (2 F must fit the int32 sum of half crossings).
 *
 * Crossings.  A pure function of its input; the unit is built with -ffp-contract=off.  `bvh` is what tsb_build (ts_bvh.h) wrote for the F
 * faces.  Ray i has origin o = origins[3i..] and direction d = directions[3i..], or with shared_direction == 1 d = directions[0..2] for every
 * ray (the inside test's case: dominant axis and shear are then the same for a whole wave).  Bad ray, hi, eligibility, the triangle test
 * (U, V, W, det, tt), the slab test, AABB(T) and t' = max(tt, tn) are those of ts_ray.h with cull_back = 0, to the letter, and a face is HIT
 * iff it is hit in that header's sense.  Per ray, over ALL hit faces, with z = the number of U, V, W that equal 0 and s = +1 when det > 0
 * (the front), else -1:
 *   hits       the number of hit faces
 *   winding2   the sum of 2 s over the hits with z = 0, plus the sum of s over the hits with z = 1: HALF crossings
 *   touches    the number of hits with z >= 2: the ray goes through a vertex of the face
 * A bad ray gets hits = -1, winding2 = 0, touches = 0.  F == 0 (bvh may be NULL) or no eligible face: zeros.  Q == 0 is the no-op.
 *
 * Why half crossings.  The two faces of a shared edge compute the same two products, subtracted the other way round (ts_ray.h): the edge value
 * is exactly 0 for both faces or for neither.  A ray that crosses the surface through an edge gets s + s with equal sides: one crossing.  A
 * ray that only grazes a fold gets +1 - 1 = 0.  A boundary edge leaves winding2 odd, which the caller can see.  Through a vertex any number of
 * faces meet and no fixed weight is right: the ray is reported (touches) and the caller casts another.  Integer sums do not depend on the order
 * of the faces or of the walk.
 *
 * Equal to brute force.  The walk skips a node only when its box B is not crossed, tf(B) < tmin or tn(B) > hi.  Every operation of the slab
 * interval is monotone, rounding included (ts_ray.h): for a node box B that contains AABB(T) = A, tn(B) <= tn(A) and tf(B) >= tf(A), and
 * a zero-direction axis that passes A passes B.  A hit face has A crossed, tf(A) >= tmin and tn(A) <= t' <= hi, so every node above it is
 * crossed with tf(B) >= tmin and tn(B) <= hi and is never skipped: the walk evaluates every hit face exactly once (a face lies in one leaf)
 * and the counts are the brute-force counts bit for bit.  There is no nearest hit to prune on: the walk visits every leaf whose box some ray
 * of the wave crosses within its range.
 *
 * Cost.  The rays are Morton-sorted by their origins, one wave owns 64 consecutive sorted rays and walks the tree once for all of them.
 * `leaf_visits` gains the number of (wave, leaf) visits.
 *
 * Signed distance.  One thread per point, on dist2 (what tsb_closest wrote for the point) and hits, winding2, touches (what tsi_crossings
 * wrote for a ray from the point).  The ray is CLEAN iff hits >= 0, touches == 0 and winding2 is even.  w = -winding2 / 2: a point inside an
 * outward-facing closed mesh has w = +1.  INSIDE by rule: 0 (nonzero) w != 0; 1 (odd) w is odd; 2 (positive) w > 0.
 *   dist2 == 0               out = +0, decided = 1, whatever the ray says
 *   dist2 NaN or +inf        out = NaN (0x7FC00000), decided = 0
 *   the ray is not clean     out = +(float)sqrt(dist2), decided = 0
 *   otherwise                out = (float)sqrt(dist2), negated when inside, decided = 1
 * sqrt is the correctly rounded float64 one.  Negative inside is TSDFVolume's convention (ts_volume.h; the extraction's inside is f < iso).
 * only_undecided == 1: a point whose decided byte is not 0 on entry keeps out and decided as they are (`out` and `decided` are then inputs as
 * well); the caller retries along another direction.  With 0 both are overwritten in full.
 *
 * The inside test's three directions, fp32, in this order; the result of every function of mesh_inside.py is that of the FIRST whose ray is
 * clean:  (0.7548777, 0.5698403, 0.3247180)  (-0.4301597, 0.6823278, -0.5905000)  (0.2360680, -0.4142136, 0.8793852).
 *
 * Purity (DESIGN.md "Purity of the entry points").  The workspace and all outputs may hold anything on entry; hits, winding2 and touches are
 * overwritten in full, out and decided as said above; `leaf_visits` is a caller-cleared accumulator; no byte outside the size query or an
 * output's extent is written.
 */
#ifndef TS_INSIDE_H
#define TS_INSIDE_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The text of the calling thread's last error of this library. */
const char *tsi_last_error(void);

/* Bytes of device workspace of a crossing count of Q rays.  Monotonic. */
size_t tsi_crossings_workspace_bytes(int32_t Q);

/* origins: Q*3 floats; directions: Q*3 floats, or 3 with shared_direction == 1; t_limit: Q floats or NULL; bvh: the index of the F faces;
 * hits, winding2, touches: Q int32 each; leaf_visits: one 64-bit device word that the caller cleared, or NULL. */
int tsi_crossings(int32_t Q, const float *origins, const float *directions, int32_t shared_direction, const float *t_limit, double tmin,
                  double tmax, int32_t F, const void *bvh, size_t bvh_bytes, int32_t *hits, int32_t *winding2, int32_t *touches,
                  unsigned long long *leaf_visits, void *workspace, size_t workspace_bytes, void *stream);

/* dist2: Q doubles; winding2, touches, hits: Q int32 each; rule: 0, 1 or 2; only_undecided: 0 or 1; out: Q floats; decided: Q bytes. */
int tsi_signed_distance(int32_t Q, const double *dist2, const int32_t *winding2, const int32_t *touches, const int32_t *hits, int32_t rule,
                        int32_t only_undecided, float *out, uint8_t *decided, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_INSIDE_H */
