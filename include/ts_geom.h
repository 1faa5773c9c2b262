/*
 * ts_geom.h -- C ABI of libts_geom.so: the geometric scores of an exported mesh.  An exact nearest-neighbour search between two
 * DIFFERENT point sets, and a deterministic area-weighted surface sampler; diff_recon_hip/mesh_distance.py builds accuracy /
 * completeness / Chamfer / precision / recall / F-score on the two, and RawTriangle's set difference on the first.
 *
 * A library of its own, beside libts2d.so: the entry points of libts2d.so are a closed list.  libts_geom.so links
 * the same radix sort (csrc/radix_sort.hip) and the same front half of the box searches (csrc/ts_knn_front.h) and keeps its own error text.
 * The error codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, a null required pointer or a workspace below the size query return
 * TS2D_ERR_INVALID with the text in the last-error call of this header.  Counts are int32_t, so at most 2^31 - 1.  Zero counts are no-ops
 * that return TS2D_OK (see each call for what "zero" covers).
 *
 * Nearest search.  A pure function of its input; the unit is built with -ffp-contract=off.
 *   distance     d(q, r) = (dx*dx + dy*dy) + dz*dz in fp32 with every operation rounded, dx = qx - rx, dy = qy - ry, dz = qz - rz.
 *   eligible     a ref is eligible iff its three coordinates are finite.
 *   selection    nearest[i] = the eligible ref with the smallest d, ties to the SMALLEST REF INDEX; dist2[i] = that d, bit for bit.  When every
 *                eligible ref is at d = +inf (fp32 overflow), the smallest eligible index still wins.
 *   no ref       no eligible ref (R == 0 included): nearest[i] = -1, dist2[i] = +inf.
 *   bad query    a query with a NaN or infinite coordinate: nearest[i] = -1, dist2[i] = NaN.
 *   Q == 0 is the no-op.
 *
 * Cost of the search.  Both sets are Morton-sorted into boxes of 1024 points; one 256-lane workgroup owns 1024 sorted queries.  It first
 * scans the ref box that is nearest to its query box, then every ref box whose box-to-box bound does not exceed the workgroup's worst
 * current distance, about 1024 x 1024 distance evaluations per box it visits.  Queries that lie among the refs visit a handful of boxes.
 * Queries FAR FROM ALL REFS see every ref box within their (large) radius: a query cluster away from the refs visits every box, and the
 * search goes QUADRATIC, Q x R distance evaluations.  `box_visits` reports it.
 *
 * Face areas.  area[f] = 0 for an invalid face: its keep byte is 0, an index lies outside [0, V), or a coordinate is non-finite.  A
 * valid face is computed in float64 with every operation rounded: e1 = v1 - v0, e2 = v2 - v0 from the fp32 coordinates widened to double,
 * c = e1 x e2 with each component a*b - c*d, area = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz).
 *
 * Surface sampler.  A pure function of (area, vertices, faces, N, seed).
 *   weights      amax = max area; amax == 0 (F == 0 included): every face[s] = -1 and every point is 0.  Otherwise
 *                w[f] = (uint64) floor(area[f] / amax * 4294967296.0) in float64, C = the inclusive 64-bit prefix sum of w, W = C[F-1] >= 2^32 > N.
 *   random words sample s draws r0, r1 = splitmix64 of the counters k = 2s, 2s+1: z = seed + (k+1)*0x9E3779B97F4A7C15;
 *                z = (z ^ z>>30)*0xBF58476D1CE4E5B9; z = (z ^ z>>27)*0x94D049BB133111EB; r = z ^ z>>31 (mod 2^64).
 *   face         stratified: qn = W / N, rem = W % N; stratum s starts at b = s*qn + min(s, rem) and has length L = qn + (s < rem);
 *                t = b + r0 % L; face[s] = the smallest f with C[f] > t.  `face` is non-decreasing in s.
 *   point        iu = r1 >> 40, iv = (r1 >> 16) & 0xFFFFFF; if iu + iv > 2^24 both are replaced by 2^24 - iu, 2^24 - iv; u = iu * 2^-24,
 *                v = iv * 2^-24 (exact); the point is (v0 + u*(v1 - v0)) + v*(v2 - v0) per coordinate in fp32, every operation rounded.
 *   `area` is meant to be what the face-area call wrote for the same mesh.  A face drawn from a foreign `area` whose indices lie outside
 *   [0, V) is never read: its point is 0.  Areas are non-negative and not NaN.
 *   N == 0 is the no-op.
 *
 * Purity (DESIGN.md "Purity of the entry points").  The workspaces may hold anything on entry; nearest, dist2, area, points and face are
 * overwritten in full whatever they held; `box_visits` is a caller-cleared accumulator; no byte outside the workspace sizes or an output's
 * extent is written.
 */
#ifndef TS_GEOM_H
#define TS_GEOM_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The text of the calling thread's last error of this library. */
const char *tsg_last_error(void);

/* Bytes of device workspace of a nearest search of Q queries among R refs.  Monotonic in both. */
size_t tsg_cross_workspace_bytes(int32_t Q, int32_t R);

/* queries: Q*3 floats; refs: R*3 floats; nearest: Q int32; dist2: Q floats.  box_visits: one 64-bit device word that the caller cleared,
 * or NULL; it gains the number of (workgroup, ref box) visits. */
int tsg_nearest_cross(int32_t Q, const float *queries, int32_t R, const float *refs, int32_t *nearest, float *dist2,
                      unsigned long long *box_visits, void *workspace, size_t workspace_bytes, void *stream);

/* Bytes of device workspace of the sampler for F faces.  Monotonic. */
size_t tsg_sample_workspace_bytes(int32_t F);

/* vertices: V*3 floats; faces: F*3 int32; keep: F bytes or NULL (all faces); area: F doubles.  F == 0 is the no-op. */
int tsg_face_areas(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, double *area, void *stream);

/* points: N*3 floats; face: N int32. */
int tsg_sample_surface(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const double *area, int32_t N, uint64_t seed,
                       float *points, int32_t *face, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_GEOM_H */
