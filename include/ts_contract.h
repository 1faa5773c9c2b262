/*
 * ts_contract.h -- C ABI of libts_contract.so: decimation of an indexed triangle mesh to a face budget or an error bound by EDGE
 * CONTRACTION (Garland and Heckbert's pair contraction), one round per call.  A contraction of the edge {r, k} replaces r by k in every
 * face around r, deletes the two faces on the edge, and MOVES the survivor k to the minimum of the summed quadrics of both ends, pulled
 * towards the midpoint of the edge and rounded to fp32.  ts_decimate.h's half-edge collapse keeps the survivor where it was; on a coarse
 * mesh of a curved surface every input vertex lies on one side of the best-fitting faces, and this operator is the one that leaves it.
 * diff_recon_hip/mesh_contract.py builds contract_round, placed_edges, contract_mesh and contract_fused on it.
 *
 * A library of its own, the twentieth: the export lists of the other nineteen are closed.  It links the product's radix_sort object and
 * no other product object, and keeps its own error text.  The error codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so
 * the calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, max_collapses < 0, a max_cost that is not >= 0 (NaN included; +inf is
 * allowed), a max_edge that is not > 0 (NaN included), a min_cos outside [0, 1] (NaN included), a lambda or a reach that is not finite
 * and >= 0, a null required pointer, a pointer to float64 values (quadrics, out_quadrics, vertex_blend, edge_cost) that is not 8-byte
 * aligned, out_faces, out_keep, vertex_target, out_vertices, out_quadrics and vertex_blend not given together, a workspace below
 * tsu_workspace_bytes(V, F) return TS2D_ERR_INVALID with the text in tsu_last_error(); TS2D_ERR_CAPACITY at ts_collapse.h's capacities
 * (F above 536870911, or V + 3 F above 2147483647).
 *
 * The result is a pure function of the input: the only atomics are integer adds of counters, nothing depends on thread or launch order.
 * The arithmetic is float64 on the fp32 inputs widened, every operation rounded (the unit is built with -ffp-contract=off), written
 * operation by operation in tests/ref_mesh_contract.py.  p - q, dot, cross and length2 are ts_collapse.h's.
 *
 * Taken from ts_collapse.h word for word, and not redefined here: which faces TAKE PART, half-edges and opposite vertices, the numbering
 * of the edges 0 .. E-1 in ascending (lo, hi), length2, CLEAN edges, RINGS, the vertex classes FREE and HELD with the ring bound
 * TSU_MAX_RING = 64, ELIGIBLE edges (c and d are the vertices opposite to the edge), the LINK guard, and the 32-bit priority of
 * (lo, hi, seed).  The guard bits and the edge states carry that header's values.  Quadrics are ts_decimate.h's: ten float64 values per
 * vertex, a00 a01 a02 a11 a12 a22 b0 b1 b2 c, in that vertex's OWN FRAME, Q_v(x) = y^T A y + 2 b . y + c with y = x - p_v; the caller
 * obtains the initial ones from that header's vertex quadrics.
 *
 * One decision per eligible EDGE (ts_decimate.h decides per direction).
 *
 * Ends.  Both ends FREE: k = lo, r = hi, and the survivor is PLACED.  Exactly one end FREE: r is the free end, k the held one, and the
 * survivor STAYS at p_k: that is ts_decimate.h's half-edge collapse for that direction, with its cost (cost_r + c_k), its three guards over
 * the ring of r and its TSU_GUARD_HELD bit for the direction that is not walked, word for word.  With p* = p_k the rest of this text holds
 * for it unchanged.
 *
 * Edge quadric, in the frame of k.  d = p_k - p_r.  A_r d is formed per row i as (a_i0 dx + a_i1 dy) + a_i2 dz from the quadric of r, and
 * cost_r = (dot(d, A_r d) + (dot(b_r, d) + dot(b_r, d))) + c_r, as in ts_decimate.h.  Then, entry by entry and axis by axis,
 *     A = A_k + A_r,      b = b_k + (A_r d + b_r),      c = c_k + cost_r.
 *
 * Placement (both ends FREE).  ts_simplify.h's quadric placement operation for operation, towards the midpoint m = -0.5 d per axis (exact):
 * tr = (a00 + a11) + a22.  If tr is finite and > 0: mu = (double)lambda tr is added to a00, a11, a22; the right-hand side is
 * r_i = mu m_i - b_i; c00 = a11 a22 - a12 a12, c01 = a02 a12 - a01 a22, c02 = a01 a12 - a02 a11, c11 = a00 a22 - a02 a02,
 * c12 = a01 a02 - a00 a12, c22 = a00 a11 - a01 a01; det = (a00 c00 + a01 c01) + a02 c02.  If det is finite and > 0,
 * y_i = ((c_i0 r0 + c_i1 r1) + c_i2 r2) / det (c symmetric); if all three y_i are finite that is y.  Any failed test gives y = m.
 * The regularised diagonal is used in the solve alone: the A of the edge quadric, of the cost and of the merge is the sum above.
 *
 * Reach.  h = (double)reach max(|dx|, |dy|, |dz|); no square root.  Per axis t_i = y_i - m_i; if t_i > h then y_i = m_i + h; if
 * t_i < -h then y_i = m_i - h; otherwise y_i stays.  If h is 0, y = m: reach = 0 is midpoint placement bit for bit.
 *
 * Rounding first.  p* = (float)((double)p_k + y) per axis, and everything below uses y' = (double)p* - (double)p_k: the cost and the
 * guards are those of the fp32 mesh that is written, not of the unrounded solve.
 *
 * Cost.  A y' per row as above, cost = (dot(y', A y') + (dot(b, y') + dot(b, y'))) + c.  If it is not finite the edge HAS NO COST.
 * Otherwise a negative cost, or -0, becomes +0: the bit pattern of a cost is then monotone as an unsigned 64-bit integer.
 *
 * Guards of a placed edge, each over the whole ring, without early exit; every guard that fails adds its bit:
 *   TSU_GUARD_LINK    ts_collapse.h's, for the direction r -> k over the ring of r.
 *   TSU_GUARD_LONG    length2(p*, p_x) <= (double)max_edge (double)max_edge for every ring neighbour x of r and of k other than r and k
 *                     (d = p_x - p* per axis, (dx dx + dy dy) + dz dz; a comparison with NaN is false).
 *   TSU_GUARD_NORMAL  ts_collapse.h's inequality, Q1 > 0 && (Q0 == 0 || (D > 0 && D D >= (M Q0) Q1)), with n0 from the face as it is and
 *                     n1 with p* in the moved corner's place: for a ring face (v, x, y) of v = r or v = k,
 *                     n0 = cross(p_x - p_v, p_y - p_v), n1 = cross(p_x - p*, p_y - p*).  It is evaluated for every SURVIVING ring face of
 *                     r AND of k: a face that does not contain both ends.
 * The ring of k is bounded because k is FREE.  The edge PASSES iff no guard fails, it has a cost, and cost <= (double)max_cost; it is
 * then a CANDIDATE with r = hi and that cost.  If no guard fails but it does not pass it is TSU_TOO_COSTLY and reports its cost, +inf if
 * it has none.  Otherwise it is TSU_GUARDED.
 *
 * Budget, ranking, selection: ts_decimate.h's.  The call takes max_collapses >= 0.  The candidates are ranked 0, 1, 2, ... in the total
 * order (cost ascending as float64, priority descending, edge id ascending); a candidate with rank >= max_collapses is TSU_DEFERRED and
 * takes no part in the selection; the selection is ts_collapse.h's best / best2 / winners over the others, on the unique ranks.  A round
 * never contracts more than max_collapses edges, and when a candidate is in budget the first one in the order always wins.
 * The round stays independent although k now moves: no winner has an end inside the closed ring of another winner's ends, so every face
 * whose guard was evaluated for a winner has exactly one moving corner, and every new edge was measured from the only end of it that
 * moves.  The round equals its winners applied one after another in any order.
 *
 * What follows a winner.  vertex_target, out_faces and out_keep are exactly ts_collapse.h's.
 *   out_vertices   the row of k becomes p*; every other row, the row of r included, is copied bit for bit.
 *   out_quadrics   the row of k, in the NEW own frame of k: A' = A, b' = b + A y' per axis, c' = the cost before the clamp.  For a
 *                  survivor that stays it is ts_decimate.h's row: A, b, c.  Every other row is copied bit for bit.
 *   vertex_blend   for a placed survivor t = dot(y', -d) / dot(d, d), with -d negated per axis; if t is not > 0 (NaN and -0 included)
 *                  t = +0; if t > 1, t = 1; dot(d, d) == 0 gives t = 0.  It is 0 for every other vertex.  It is how far the survivor went
 *                  from p_k towards p_r: the caller blends attributes as (1 - t) attr_k + t attr_r.
 *
 * tsu_contract runs one round and writes every element of its outputs, to their capacity of F faces, V vertices and 3 F edges:
 *   out_faces      F x 3 int32, out_keep F bytes, vertex_target V int32, out_vertices V x 3 fp32, out_quadrics V x 10 float64,
 *                  vertex_blend V float64.  All six NULL: the call classifies only; the selection is still made and reported.
 *   edge_vertices  3 F x 2 int32: (lo, hi) of edge e; -1 past E.
 *   edge_state     3 F bytes: TSU_NOT_ELIGIBLE, TSU_TOO_COSTLY, TSU_GUARDED, TSU_LOST, TSU_COLLAPSED or TSU_DEFERRED; TSU_NO_EDGE past E.
 *   edge_removed   3 F int32: r of a candidate (lost, collapsed or deferred), -1 otherwise and past E.
 *   edge_guard     3 F bytes: the guard mask of an eligible edge, 0 otherwise and past E.
 *   edge_cost      3 F float64: the cost of a candidate, the reported cost of a TSU_TOO_COSTLY edge, +inf otherwise and past E.
 *   edge_position  3 F x 3 fp32: p* of a candidate; NaN (0x7FC00000) otherwise and past E.
 *   totals         five 64-bit words {edges, candidates, in_budget, collapsed, too_costly}; candidates counts the deferred ones too.
 * V == 0 or F == 0 is a valid call that writes the empty result: with F == 0 only totals (zeros), vertex_target (the identity),
 * out_vertices and out_quadrics (copies) and vertex_blend (zeros); with V == 0 nothing takes part, every face is copied and every other
 * entry holds its fill value.
 *
 * Cost.  The front, the ranking (three stable 32-bit radix sorts over the 3 F edge slots) and the selection are ts_decimate.h's
 * (csrc/ts_collapse_round.h holds what the units share).  One thread per edge slot classifies: an eligible edge with two FREE ends loads
 * two quadrics, solves once and walks two rings.
 *
 * Purity (DESIGN.md "Purity of the entry points").  The workspace may hold anything on entry; every output above is overwritten whatever
 * it held; no byte outside tsu_workspace_bytes(V, F) or an output's extent is written.
 */
#ifndef TS_CONTRACT_H
#define TS_CONTRACT_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSU_NO_EDGE 0
#define TSU_NOT_ELIGIBLE 1
#define TSU_TOO_COSTLY 2
#define TSU_GUARDED 3
#define TSU_LOST 4
#define TSU_COLLAPSED 5
#define TSU_DEFERRED 6

#define TSU_GUARD_LINK 1
#define TSU_GUARD_LONG 2
#define TSU_GUARD_NORMAL 4
#define TSU_GUARD_HELD 8

#define TSU_MAX_RING 64

/* The text of the calling thread's last error of this library. */
const char *tsu_last_error(void);

/* Bytes of device workspace that serve the call below for V vertices and F faces.  Monotonic in V and in F. */
size_t tsu_workspace_bytes(int32_t V, int32_t F);

/* vertices: V*3 floats; faces: F*3 int32; keep: F bytes or NULL; pinned: V bytes or NULL; quadrics: V*10 float64; max_cost >= 0, +inf for
 * none; max_collapses >= 0; max_edge > 0, +inf for none; min_cos in [0, 1], formed by the caller as for ts_collapse.h; lambda >= 0: the
 * pull towards the midpoint, as a share of the trace; reach >= 0: how far from the midpoint the survivor may go, in units of the edge's
 * largest axis extent; seed: mixed into the priorities; out_faces: F*3 int32, out_keep: F bytes, vertex_target: V int32, out_vertices: V*3
 * floats, out_quadrics: V*10 float64 and vertex_blend: V float64, or all six NULL; edge_vertices: 3*F*2 int32; edge_state, edge_guard: 3*F
 * bytes; edge_removed: 3*F int32; edge_cost: 3*F float64; edge_position: 3*F*3 floats; totals: five 64-bit device words, overwritten.
 * The workspace is needed with F > 0.  F is at most 536870911 and V + 3*F at most 2147483647. */
int tsu_contract(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, const uint8_t *pinned,
                 const double *quadrics, float max_cost, int32_t max_collapses, float max_edge, float min_cos, float lambda, float reach,
                 uint32_t seed, int32_t *out_faces, uint8_t *out_keep, int32_t *vertex_target, float *out_vertices, double *out_quadrics,
                 double *vertex_blend, int32_t *edge_vertices, uint8_t *edge_state, int32_t *edge_removed, uint8_t *edge_guard,
                 double *edge_cost, float *edge_position, unsigned long long *totals, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_CONTRACT_H */
