/*
 * ts_orient.h -- C ABI of libts_orient.so: every orientable piece of an indexed triangle mesh made to wind one way, the pieces that cannot
 * be oriented (Moebius-like) reported, and the way each piece faces chosen by a stated rule, on the device.
 * diff_recon_hip/mesh_orient.py builds orient_faces and orient_fused on it.
 *
 * A library of its own, beside libts2d.so, libts_geom.so, libts_bvh.so, libts_ray.so, libts_volume.so, libts_color.so, libts_simplify.so,
 * libts_smooth.so, libts_holes.so and libts_manifold.so: the export lists of all ten are closed.  It links the product's radix_sort object
 * and no other, and keeps its own error text.  The error codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, a mode outside 0..2, mode 2 without vertices (with V > 0), a null
 * required pointer, a workspace below tsw_workspace_bytes(V, F) return TS2D_ERR_INVALID with the text in tsw_last_error(); more than
 * 715827882 faces (3 F half-edges in an int32; the sort's layout asks for no less) is TS2D_ERR_CAPACITY.
 *
 * The result is a pure function of the input: the only atomics are integer (compare-exchange, minimum, maximum, add), nothing depends on
 * thread order.  The floating-point arithmetic of mode 2 is float64 on widened fp32 and every operation rounds (the unit is built with
 * -ffp-contract=off); its sums are 64-bit integers.  The contract is written operation by operation in tests/ref_mesh_orient.py.
 *
 * Participation, half-edges, edge use.  Exactly ts_manifold.h's: a face TAKES PART iff keep[f] != 0 (a NULL keep means all faces), its
 * three indices lie in [0, V) and are pairwise distinct; face f, slot k, is half-edge 3 f + k from faces[f][k] (its tail) to
 * faces[f][(k + 1) % 3] (its head); the use count of the undirected edge {a, b} is the number of participating half-edges between a and b
 * in either direction.
 *
 * Links.  An edge used EXACTLY TWICE links its two faces f and g.  The link is EVEN when the two half-edges run in opposite directions
 * (the two faces wind consistently) and ODD when they run in the same direction (an orientation conflict).  Edges used once, or three
 * times and more, link nothing: run after tsf_split, where no such edge is left, to orient across every shared edge.
 *
 * Pieces and flips, by the DOUBLED GRAPH.  There are 2 F nodes: node 2 f is "f as given", node 2 f + 1 is "f reversed".  An even link
 * unites (2 f, 2 g) and (2 f + 1, 2 g + 1); an odd link unites (2 f, 2 g + 1) and (2 f + 1, 2 g), in the lock-free union-find of
 * csrc/ts_union_find.h, whose roots are the smallest index whatever the order of the unions.  With r0 = root(2 f) and r1 = root(2 f + 1):
 *   face_piece[f] = min(r0, r1) >> 1, the smallest face of f's PIECE (a connected component of the links), the piece's ANCHOR; -1 for a
 *                   face that does not take part;
 *   the piece is NON-ORIENTABLE iff r0 == r1: no choice of flips makes it consistent, and its faces get flip 0;
 *   otherwise the CONSISTENCY FLIP of f is r0 & 1, so the anchor keeps its direction.
 * face_piece does not depend on the winding of the input.
 *
 * Outward rule.  `mode` chooses, for every orientable piece, whether ALL its flips are inverted on top:
 *   0 ANCHOR    never.
 *   1 MAJORITY  iff more than half of the piece's faces carry a consistency flip (2 c_p > n_p); a tie keeps the anchor.  This changes the
 *               fewest faces.
 *   2 VOLUME    iff the piece's quantised signed volume S_p is negative; S_p == 0 changes nothing.
 * S_p.  o is the vertex in slot 0 of the anchor face.  For a face (a, b, c) of the piece each of the nine differences d = x - o (float64
 * of the widened fp32 coordinates) takes one rounding; t = a . (b x c), the cross product formed component by component as p1 - p2
 * (by cz - bz cy, bz cx - bx cz, bx cy - by cx), the dot product left to right ((ax X + ay Y) + az Z), every product and sum rounded.
 * m_p is the largest |d| over the piece's faces whose nine differences are all finite (64-bit integer maximum on the bits of |d|); e_p is 0
 * if m_p == 0, else the frexp exponent of m_p (m_p = x 2^e_p with 0.5 <= x < 1); n_p is the piece's face count;
 * k_p = 56 - bitlength(n_p) - 3 e_p, which makes n_p |q| < 2^59; q_f = llrint(ldexp(t, k_p)), round half to even, and q_f = 0 when t or any
 * of the nine differences is non-finite: such a face is counted in counts[9], over all participating faces.  S_p is the sum of +q_f over
 * the piece's faces without and -q_f over those with a consistency flip (64-bit integer adds).  The per-piece scale keeps a small piece far
 * from the origin as well resolved as a large one at it.  A reversed row (a, c, b) has exactly the term -t, so a second call sees |S_p|.
 *
 * tsw_orient writes every element of its outputs:
 *   face_piece  F int32, above.
 *   face_flip   F bytes: 1 where the face is reversed, else 0 (faces that do not take part included).
 *   out_faces   3 F int32: a reversed face (a, b, c) becomes (a, c, b) -- slot 0 stays, so the anchor vertex of a piece does not move --
 *               and every other row is copied bit for bit.
 *   counts      ten 64-bit words {participating faces, pieces, non-orientable pieces, faces in non-orientable pieces, linking edges,
 *               same-direction edges before, same-direction edges after, faces flipped, pieces inverted by the outward rule, faces with
 *               a non-finite volume term (0 unless mode 2)}.
 * V == 0 or F == 0: nothing takes part; face_piece is -1, face_flip 0, out_faces is faces, and the counters are 0.
 *
 * Promises (the reference checks them on every fixture; the device on its own output by a second call).  counts[6] of a call equals
 * counts[5] of a second call on its output; every conflict that remains lies in a non-orientable piece, so counts[6] is 0 when counts[2]
 * is 0; a second call in the same mode flips nothing and returns the faces bit for bit; a mesh that is already consistent and
 * non-negative by the mode's rule comes back bit for bit; the faces of a non-orientable piece come back bit for bit.
 *
 * Cost.  Two stable LSD sorts of the 3 F half-edge records (tsf_fans' key: the larger, then the smaller end, on the bits of V), two
 * gathers, one pass over the sorted runs with two unions per linking edge, one flatten per face, for mode 2 a maximum and a term pass, one
 * pass that decides and writes, one pass over the sorted runs for counts[6].  The per-piece sums are integers: equal labels are reduced
 * within the wave before the global atomic, so a mesh that is ONE piece does not send F adds to one word.
 *
 * Purity (DESIGN.md "Purity of the entry points").  The workspace may hold anything on entry; every output above is overwritten whatever
 * it held; no byte outside tsw_workspace_bytes(V, F) or an output's extent is written.  The outputs overlap neither each other nor an
 * input: out_faces is not faces (the recount of counts[6] reads faces after out_faces is written).
 */
#ifndef TS_ORIENT_H
#define TS_ORIENT_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The text of the calling thread's last error of this library. */
const char *tsw_last_error(void);

/* Bytes of device workspace that serve tsw_orient for V vertices and F faces.  Monotonic in V and in F. */
size_t tsw_workspace_bytes(int32_t V, int32_t F);

/* vertices: V*3 fp32, read in mode 2 only (may be NULL otherwise); faces, out_faces: F*3 int32; keep: F bytes or NULL; mode: 0 anchor,
 * 1 majority, 2 volume; face_piece: F int32; face_flip: F bytes; counts: ten 64-bit device words, overwritten.  F is at most 715827882. */
int tsw_orient(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, int32_t mode, int32_t *face_piece,
               uint8_t *face_flip, int32_t *out_faces, unsigned long long *counts, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_ORIENT_H */
