/*
 * ts_flip.h -- C ABI of libts_flip.so: one round of edge flips toward the Delaunay condition on an indexed triangle mesh.  A flip moves no
 * vertex and keeps the numbers of vertices, edges and faces; only the connectivity changes.  diff_recon_hip/mesh_flip.py builds flip_edges,
 * delaunay_flips, nondelaunay_edges and flip_fused on it.
 *
 * A library of its own, the seventeenth: the export lists of the other sixteen are closed.  It links the product's radix_sort object and no
 * other product object, and keeps its own error text.  The error codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, a min_cos outside [-1, 1] (NaN included), a null required pointer,
 * out_faces given without face_flipped or the reverse, a workspace below tse_workspace_bytes(V, F) return TS2D_ERR_INVALID with the text in
 * tse_last_error(); TS2D_ERR_CAPACITY where 3 F, 4 F or V + 3 F does not fit the int32 indices (F above 536870911, or V + 3 F above
 * 2147483647): the capacities of ts_subdivide.h, so that every mesh that can be split can be flipped.
 *
 * The result is a pure function of the input: the only atomics are integer adds of counters, nothing depends on thread or launch order.
 * The arithmetic is float64 on the fp32 inputs widened, every operation rounded (the unit is built with -ffp-contract=off), written
 * operation by operation in tests/ref_mesh_flip.py.  Below, for points p, q: p - q is taken per axis; dot(s, t) = (s.x t.x + s.y t.y) +
 * s.z t.z; cross(s, t) = (s.y t.z - s.z t.y, s.z t.x - s.x t.z, s.x t.y - s.y t.x).
 *
 * Taking part.  A face TAKES PART by ts_subdivide.h's rule: keep[f] != 0 (a NULL keep means all faces), its three indices lie in [0, V) and
 * are pairwise distinct.  Half-edge h = 3 f + k runs from faces[f][k] to faces[f][(k + 1) % 3]; the vertex OPPOSITE to it is
 * faces[f][(k + 2) % 3].
 *
 * Edges.  The undirected edges (lo, hi), lo < hi, of the faces that take part are numbered 0 .. E-1 in ascending (lo, hi); `use` is the
 * number of half-edges on the edge.
 *
 * Eligible.  An edge is ELIGIBLE iff use == 2, its two half-edges run in opposite directions -- one runs lo -> hi in face f0 with opposite
 * vertex c, the other hi -> lo in face f1 with opposite vertex d -- c != d, and the twelve coordinates of a = lo, b = hi, c, d are finite.
 *
 * The criterion W(p, q; r, s) of an edge p-q with opposite vertices r and s, without a square root or a division:
 *   u = p - r, v = q - r, A = dot(u, v), w = cross(u, v), P = dot(w, w);    u' = p - s, v' = q - s, B = dot(u', v'), w' = cross(u', v'),
 *   Q = dot(w', w').  The two opposite angles sum to more than pi iff A sqrt(Q) + B sqrt(P) < 0, decided by cases:
 *     A < 0 and B < 0:    W iff P > 0 or Q > 0
 *     A < 0 and B >= 0:   W iff (A A) Q > (B B) P
 *     B < 0 and A >= 0:   W iff (B B) P > (A A) Q
 *     otherwise (A >= 0 and B >= 0, or a NaN):  not W
 *   Overflow and NaN behave as the arithmetic gives; a comparison with NaN is false.  An eligible edge is NON-DELAUNAY iff
 *   W(p_a, p_b; p_c, p_d).  A cocircular quad (a square) is not flipped.  A zero-area face whose apex lies on its long edge is a cap: P = 0
 *   and A < 0, so its long edge is non-Delaunay and the cap is flipped away.
 *
 * Candidate.  A non-Delaunay edge is a CANDIDATE iff all four guards pass; otherwise it is GUARDED.
 *   (i)   (min(c, d), max(c, d)) is not an edge of this round's table (binary search over the sorted (lo, hi) columns): a flip never creates
 *         an edge of use 3, nor two faces on the same three vertices.
 *   (ii)  W(p_c, p_d; p_a, p_b) is false: the edge just created does not want to flip back (always so in exact arithmetic).
 *   (iii) flatness.  n0 = cross(p_b - p_a, p_c - p_a), n1 = cross(p_a - p_b, p_d - p_b), D = dot(n0, n1), L = dot(n0, n0) dot(n1, n1),
 *         m = (double)min_cos, M = m m.  With min_cos >= 0 the guard passes iff D >= 0 && D D >= M L; with min_cos < 0 iff D >= 0 ||
 *         D D <= M L.  A crease (the edges of a cube) is left alone; a degenerate face passes, 0 >= 0.
 *   (iv)  no fold.  S = n0 + n1 per axis; m0 = cross(p_d - p_a, p_c - p_a), m1 = cross(p_b - p_d, p_c - p_d), the normals of the new faces:
 *         the guard passes iff dot(m0, S) > 0 && dot(m1, S) > 0.
 *
 * Selection.  Every candidate carries a 32-bit priority, in uint32 arithmetic (wrapping):
 *     h = seed * 0x9E3779B1 + lo;  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h += hi;  h *= 0xC2B2AE35;  h ^= h >> 16.
 *   A candidate WINS iff no other candidate among the four other edges of f0 and f1 has a greater priority, or an equal priority and a
 *   smaller edge id; the others have LOST and wait for the next round.  Winners share no face.  Two winners with disjoint faces can still
 *   propose the same new edge (two quads over one vertex pair c, d): of the winners with equal (min(c, d), max(c, d)) only the one with the
 *   smallest edge id FLIPS, the others are DUPLICATES.
 *
 * The flip.  With f0 = (a, b, c) and f1 = (b, a, d) up to rotation, slot f0 becomes (a, d, c) and slot f1 becomes (d, b, c), in this order
 * of the indices: the orientation is kept.  Every other face is copied bit for bit, a face that does not take part included.
 *
 * tse_flip runs one round and writes every element of its outputs, to their capacity of F faces and 3 F edges:
 *   out_faces      F x 3 int32, face_flipped F bytes (1 where the slot was rewritten).  Both NULL: the call classifies only; the selection
 *                  is still made and reported in edge_state and totals.
 *   edge_vertices  3 F x 2 int32: (lo, hi) of edge e; -1 past E.
 *   edge_state     3 F bytes: TSE_NOT_ELIGIBLE, TSE_DELAUNAY, TSE_GUARDED, TSE_LOST, TSE_DUPLICATE or TSE_FLIPPED; TSE_NO_EDGE past E.
 *   edge_opposite  3 F x 2 int32: (c, d) of an eligible edge, -1 otherwise and past E.
 *   totals         four 64-bit words {edges, nondelaunay, candidates, flipped}; nondelaunay counts the guarded edges too.
 * V == 0 or F == 0 is a valid call that writes the empty result: with F == 0 only totals (zeros); with V == 0 nothing takes part, every
 * face is copied and every other entry holds its fill value.
 *
 * Cost.  The front is ts_subdivide.h's: one thread per face writes the half-edge records; two stable radix sorts order them by (lo, hi)
 * (csrc/ts_mesh_edges.h); run heads become edge ids by one prefix sum in block-sum form (csrc/ts_mesh_scan.h: nobody waits for anybody).
 * One thread per edge gathers the four vertex rows and decides state, opposite vertices and priority; one scatter hands the edge ids to
 * the half-edges; one thread per edge compares itself with its four neighbours; a second prefix sum compacts the winners, at most F / 2,
 * whose new edges two stable radix sorts of that length order; the heads of the runs flip; one thread per face gathers its new indices.
 *
 * Purity (DESIGN.md "Purity of the entry points").  The workspace may hold anything on entry; every output above is overwritten whatever
 * it held; no byte outside tse_workspace_bytes(V, F) or an output's extent is written.
 */
#ifndef TS_FLIP_H
#define TS_FLIP_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSE_NO_EDGE 0
#define TSE_NOT_ELIGIBLE 1
#define TSE_DELAUNAY 2
#define TSE_GUARDED 3
#define TSE_LOST 4
#define TSE_DUPLICATE 5
#define TSE_FLIPPED 6

/* The text of the calling thread's last error of this library. */
const char *tse_last_error(void);

/* Bytes of device workspace that serve the call below for V vertices and F faces.  Monotonic in V and in F. */
size_t tse_workspace_bytes(int32_t V, int32_t F);

/* vertices: V*3 floats; faces: F*3 int32; keep: F bytes or NULL; min_cos in [-1, 1]: the cosine of the largest dihedral angle across a
 * flipped edge, formed by the caller once in float64 and rounded to fp32; seed: mixed into the priorities; out_faces: F*3 int32 and face_flipped: F bytes, or both NULL; edge_vertices, edge_opposite:
 * 3*F*2 int32; edge_state: 3*F bytes; totals: four 64-bit device words, overwritten.  The workspace is needed with F > 0.  F is at most
 * 536870911 and V + 3*F at most 2147483647. */
int tse_flip(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, float min_cos, uint32_t seed,
             int32_t *out_faces, uint8_t *face_flipped, int32_t *edge_vertices, uint8_t *edge_state, int32_t *edge_opposite,
             unsigned long long *totals, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_FLIP_H */
