/*
 * ts_overlap.h -- C ABI of libts_overlap.so: the OVERLAP query of the triangle index that the build call of ts_bvh.h wrote.  Which faces of
 * the index does this triangle meet?  Asked for every face of one mesh against its own index it lists the SELF-INTERSECTIONS of the mesh;
 * asked for the faces of mesh A against the index of mesh B it lists the face pairs in which the two meshes meet.
 * diff_recon_hip/mesh_overlap.py builds self_intersections, mesh_intersections and drop_intersecting_faces on it.
 *
 * A library of its own, the fifteenth: the export lists of the other fourteen are closed.  libts_overlap.so links the same radix sort
 * (csrc/radix_sort.hip), reads the index through the layout header it shares with the build (csrc/ts_bvh_layout.h), walks it with
 * csrc/ts_bvh_walk.h and keeps its own error text.  The error codes are ts2d.h's.  The prefix is tsx_: tso_ is ts_optim.h's, whose functions
 * libts2d.so exports.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count or capacity, a null required pointer, an index buffer below the index
 * size of its F (the size query of ts_bvh.h; computed here from the layout header), a capacity > 0 without both lists, a workspace below
 * its size query, a bit count outside [1, 31] return TS2D_ERR_INVALID with the text in the last-error call of this header.  Counts are
 * int32_t, at most 2^31 - 1025.
 *
 * Arithmetic.  A pure function of its input; the unit is built with -ffp-contract=off.  Everything below is float64 on the fp32
 * coordinates of the index widened to double, every operation rounded; dot and cross are those of ts_bvh.h (u.v = (ux*vx + uy*vy) + uz*vz;
 * u x v = (uy*vz - uz*vy, uz*vx - ux*vz, ux*vy - uy*vx)).  The query is equal to its float64 reference, bit for bit; it is no proof about
 * the geometry of the real numbers.
 *   orient       orient(a, b, c, d) = (b - a) . ((c - a) x (d - a)).
 *   takes part   a face takes part iff it is eligible in ts_bvh.h's sense (it sits in the index with a slot id >= 0) and, in self mode,
 *                its three vertex indices are pairwise different.  A face that does not take part is nobody's partner and is counted in
 *                stats[5] (degenerate): of the one mesh in self mode, of both meshes in cross mode.
 *   box filter   AABB(T) is the per-axis fp32 minimum and maximum of the three vertices.  Two boxes overlap iff on every axis
 *                mnA <= mxB && mnB <= mxA: fp32, closed.  A pair whose boxes do not overlap has kind 0 BY DEFINITION.  That is what makes
 *                the walk equal to brute force: the boxes of the index are plain fp32 min / max unions (mesh_bvh.hip's leaf and union
 *                kernels), so a node's box contains AABB(T) of every eligible face below it, and an interval that meets a part meets the
 *                whole: a walk that enters a node whenever the query's box overlaps the node's reaches every box-overlapping pair.
 *   self mode    (`faces` given, one mesh and its own index.)  Pairs are unordered, lo < hi by face index, both faces take part; A is face
 *                lo, B is face hi.  shared = the number of distinct vertex indices the two faces have in common:
 *                  3   kind 3 (DUPLICATE), nothing is computed;
 *                  2   the pair is ADJACENT: kind 0, counted in stats[1] only (a fold over a shared edge is the flap count of
 *                      ts_simplify.h's duplicate sweep, not this query's);
 *                  1, 0   decided as below.
 *   cross mode   (`faces` NULL: the faces of the query index A against the index B.)  Every pair (face of A, face of B) is considered
 *                with shared = 0; indices are not compared.
 *   plane values pB[k] = orient(a0, a1, a2, bk), pA[k] = orient(b0, b1, b2, ak), k = 0, 1, 2.  With shared == 1 the value of the shared
 *                vertex is 0 by definition and not computed (it would not round to 0 for a vertex other than a0); "the values of a face"
 *                below are those of its NON-SHARED vertices, three or two of them.
 *   apart        kind 0: the values pB are all > 0 or all < 0, or the values pA are.  Tested first: a face of zero normal beside a
 *                proper one is apart, not coplanar.
 *   kind 2       COPLANAR: not apart, and the values pB are all == 0 or the values pA are all == 0.  A face of zero normal makes every
 *                value of the other face 0.  Such pairs are reported as candidates: whether they overlap within their plane is not resolved.
 *   segment      seg(p, q, sp, sq; t0, t1, t2), the segment p q against the face (t0, t1, t2), sp and sq the plane values of p and q on
 *                that face: false when sp and sq are both > 0, both < 0 or both == 0; otherwise e0 = orient(p, q, t0, t1),
 *                e1 = orient(p, q, t1, t2), e2 = orient(p, q, t2, t0), true iff all three are >= 0 or all three are <= 0.  Closed: a touch
 *                is a hit.
 *   kind 1       CROSSING: neither apart nor coplanar, and at least one segment test is true:
 *                  shared == 0   the edges a0 a1, a1 a2, a2 a0 against B, then b0 b1, b1 b2, b2 b0 against A;
 *                  shared == 1   only A's edge opposite the shared vertex against B (a1 a2, a2 a0 or a0 a1 for a0, a1 or a2 shared: the
 *                                edge keeps its direction), and B's edge opposite it against A.  The other four edges meet the other
 *                                face's plane in the shared vertex alone.
 *                Any other pair has kind 0.
 *   finite       for finite fp32 input every intermediate is finite (an orient is below 3e117 in magnitude): no NaN is compared.
 *
 * Outputs of the overlap call.
 *   count_a      FA int32: for every face of the query mesh the number of its partners of kind 1; 0 for a face that does not take part.
 *                In self mode this is the one array, and both faces of a pair gain 1.
 *   count_b      cross mode: FB int32 or NULL, the same for the faces of B.  Self mode: must be NULL.
 *   stats        8 uint64, overwritten in full: [0] candidates (box-overlapping pairs of faces that take part, each pair once; adjacent and
 *                duplicate pairs included), [1] adjacent, [2] crossing, [3] coplanar, [4] duplicate, [5] degenerate, [6] stored, [7] 0.
 *   pairs, kind  2 * capacity int32 and capacity bytes.  Every pair of kind != 0 is appended once through an integer cursor while
 *                cursor < capacity: (lo, hi), in cross mode (face of A, face of B), and its kind.  stats[6] = min(total, capacity) with
 *                total = stats[2] + stats[3] + stats[4].  The ORDER of the list is unspecified (the sort call orders it).  When the total
 *                exceeds the capacity the list holds `capacity` valid pairs, which ones is unspecified, and the caller calls again with
 *                the total; counts and stats are exact either way.  capacity == 0 with NULL lists is allowed.
 *   leaf_visits  one 64-bit device word that the caller cleared, or NULL: gains the number of (wave, leaf) visits.
 *   FA == 0 or FB == 0: zeros and an empty list (the index pointers may be NULL for an F of 0).
 * All sums are integer atomics: the result does not depend on the order of the walk or on which faces share a wave.
 *
 * Sorting the list (the sort call).  Orders a complete list of P pairs ascending by (first, second), the kinds along with them: two stable
 * passes of the product's radix sort, by the low bits_second bits of the second entry, then by the low bits_first bits of the first.  P is
 * known to the host after it has read stats; every entry must lie below 2^bits of its column.  A list without repeated pairs, which the
 * overlap call writes, has one sorted form.
 *
 * Cost.  The queries are the leaves of the query index themselves, Morton-sorted by the build: one wave owns 64 consecutive leaf slots
 * (8 leaves) and walks the tree once for all of them, entering a node when some lane's box overlaps the node's.  Nothing is sorted and the
 * overlap call has no workspace.
 *
 * Purity (DESIGN.md "Purity of the entry points").  The sort's workspace and all outputs may hold anything on entry; count_a, count_b
 * and stats are cleared and overwritten in full; of pairs and kind the first stats[6] entries are written; leaf_visits is a caller-cleared
 * accumulator; no byte outside the size query or an output's extent is written.
 */
#ifndef TS_OVERLAP_H
#define TS_OVERLAP_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSX_KIND_CROSSING 1
#define TSX_KIND_COPLANAR 2
#define TSX_KIND_DUPLICATE 3

/* The text of the calling thread's last error of this library. */
const char *tsx_last_error(void);

/* bvh_a: the index of the FA query faces.  faces: FA*3 int32, the array the index was built from: SELF mode, bvh_b must be NULL and FB 0,
 * count_b NULL.  faces NULL: CROSS mode against bvh_b, the index of the FB faces of the other mesh.  count_a: FA int32; count_b: FB int32
 * or NULL; stats: 8 uint64; pairs: 2*capacity int32 and kind: capacity bytes, both NULL when capacity == 0; leaf_visits: one cleared
 * 64-bit device word or NULL. */
int tsx_overlap(int32_t FA, const void *bvh_a, size_t bvh_a_bytes, const int32_t *faces, int32_t FB, const void *bvh_b, size_t bvh_b_bytes,
                int32_t *count_a, int32_t *count_b, uint64_t *stats, int32_t capacity, int32_t *pairs, uint8_t *kind,
                unsigned long long *leaf_visits, void *stream);

/* Bytes of device workspace of a sort of P pairs.  Monotonic. */
size_t tsx_sort_workspace_bytes(int32_t P);

/* pairs: P*2 int32, every first entry in [0, 2^bits_first), every second in [0, 2^bits_second); kind: P bytes; both reordered in place.
 * P == 0 is the no-op. */
int tsx_sort_pairs(int32_t P, int32_t bits_first, int32_t bits_second, int32_t *pairs, uint8_t *kind, void *workspace, size_t workspace_bytes,
                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_OVERLAP_H */
