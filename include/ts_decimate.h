/*
 * ts_decimate.h -- C ABI of libts_decimate.so: decimation of an indexed triangle mesh to a face budget or an error bound, one round of
 * half-edge collapses ordered by quadric error (Garland and Heckbert) per call.  A collapse r -> k is ts_collapse.h's: r is replaced by k
 * in every face around r, the two faces on the edge are deleted, no vertex moves.  What is new is the order -- the cheapest collapse
 * first, by the quadric of the removed vertex evaluated at the surviving one -- a budget of collapses per round, and the quadrics that
 * follow the collapses.  diff_recon_hip/mesh_decimate.py builds vertex_quadrics, decimate_round, cheapest_edges, decimate_mesh and
 * decimate_fused on it.
 *
 * A library of its own, the nineteenth: the export lists of the other eighteen are closed.  It links the product's radix_sort object and
 * no other product object, and keeps its own error text.  The error codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so
 * the calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, max_collapses < 0, a max_cost that is not >= 0 (NaN included; +inf is
 * allowed), a max_edge that is not > 0 (NaN included), a min_cos outside [0, 1] (NaN included), a null required pointer, a pointer to
 * float64 values (quadrics, out_quadrics, edge_cost) that is not 8-byte aligned, out_faces, out_keep, vertex_target and out_quadrics not
 * given together, a workspace below tsz_workspace_bytes(V, F) return TS2D_ERR_INVALID with the text in tsz_last_error(); TS2D_ERR_CAPACITY
 * at ts_collapse.h's capacities (F above 536870911, or V + 3 F above 2147483647).
 *
 * The result is a pure function of the input: the only atomics are integer adds of counters, nothing depends on thread or launch order.
 * The arithmetic is float64 on the fp32 inputs widened, every operation rounded (the unit is built with -ffp-contract=off), written
 * operation by operation in tests/ref_mesh_decimate.py.  p - q, dot, cross and length2 are ts_collapse.h's.
 *
 * Taken from ts_collapse.h word for word, and not redefined here: which faces TAKE PART, half-edges and opposite vertices, the numbering
 * of the edges 0 .. E-1 in ascending (lo, hi), length2, CLEAN edges, RINGS, the vertex classes FREE and HELD with the ring bound
 * TSZ_MAX_RING = 64, ELIGIBLE edges, the three guards LINK, LONG and NORMAL and the HELD bit -- each guard evaluated over the whole ring
 * of r without early exit -- and the 32-bit priority of (lo, hi, seed).  The guard bits carry that header's values.
 *
 * Vertex quadrics.  A quadric is ten float64 values per vertex, a00 a01 a02 a11 a12 a22 b0 b1 b2 c, in that vertex's OWN FRAME:
 *     Q_v(x) = y^T A y + 2 b . y + c   with y = x - p_v.
 * tsz_vertex_quadrics computes the initial quadrics.  For vertex v the ring faces (v, x, y) are taken in ascending corner index (the
 * stable sort of the corners by vertex gives that order).  A ring face contributes iff its nine coordinates are finite (it takes part: it
 * is in the ring).  For such a face e1 = p_x - p_v, e2 = p_y - p_v, n = cross(e1, e2), and the six accumulators of A, which start at 0,
 * gain nx nx, nx ny, nx nz, ny ny, ny nz, nz nz (one product, one sum each).  b and c are 0.  The normal is unnormalised: area^2
 * weights, ts_simplify.h's convention, no square root and no division.  A vertex that is not finite or has no ring face gets ten zeros.
 * There is no ring cap here: rings are walked, at any valence.
 *
 * Cost of a direction r -> k, both ends of an eligible edge.  d = p_k - p_r.  A d is formed per row i as (a_i0 dx + a_i1 dy) + a_i2 dz
 * from the quadric of r (A is symmetric: a_10 = a_01 and so on).
 *     cost_r = (dot(d, A_r d) + (dot(b_r, d) + dot(b_r, d))) + c_r,      cost = cost_r + c_k.
 * If cost is not finite the direction HAS NO COST.  Otherwise a negative cost, or -0, becomes +0: the bit pattern of a cost is then
 * monotone as an unsigned 64-bit integer.
 *
 * Direction.  Every direction whose r is FREE is walked: both where both ends are FREE, unlike ts_collapse.h.  A direction whose r is
 * HELD is not walked and adds TSZ_GUARD_HELD.  A walked direction PASSES iff its three guards pass, it has a cost, and
 * cost <= (double)max_cost.  Of two passing directions the smaller cost wins; a tie goes to r = hi.  The edge is then a CANDIDATE with that
 * r and that cost.  If no direction passes but some direction passed its guards, the edge is TSZ_TOO_COSTLY and reports the smaller cost
 * among those directions, +inf if none of them has a cost.  If no direction passed its guards the edge is TSZ_GUARDED.  The guard mask of
 * every eligible edge is the OR over all its directions: the failing guards of the walked ones and TSZ_GUARD_HELD of the others.
 *
 * Budget.  The call takes max_collapses >= 0.  The candidates of the round are ranked 0, 1, 2, ... in the total order (cost ascending as
 * float64, priority descending, edge id ascending).  A candidate with rank >= max_collapses is TSZ_DEFERRED and takes no part in the
 * selection.  The selection is ts_collapse.h's best / best2 / winners over the remaining candidates in the same order -- an independent
 * set at distance two, so the round equals its winners applied one after another in any order.  The implementation compares the unique
 * ranks instead of the key triples, which is the same order.  Two consequences:
 *   - a round never collapses more than max_collapses edges;
 *   - when at least one candidate is in budget, the first candidate in the order always wins: a round makes progress.
 *
 * The collapse.  vertex_target, out_faces and out_keep are exactly ts_collapse.h's.  The quadrics follow: for a winner r -> k, with d and
 * cost_r as above (cost_r unclamped),
 *     A_k' = A_k + A_r entry by entry,   b_k' = b_k + (A_r d + b_r) per axis,   c_k' = c_k + cost_r.
 * Every other row of out_quadrics, the row of r included, is copied bit for bit.  At distance two no vertex is the k of two winners, so
 * this is free of any order.
 *
 * tsz_decimate runs one round and writes every element of its outputs, to their capacity of F faces, V vertices and 3 F edges:
 *   out_faces      F x 3 int32, out_keep F bytes, vertex_target V int32, out_quadrics V x 10 float64.  All four NULL: the call classifies
 *                  only; the selection is still made and reported in edge_state and totals.
 *   edge_vertices  3 F x 2 int32: (lo, hi) of edge e; -1 past E.
 *   edge_state     3 F bytes: TSZ_NOT_ELIGIBLE, TSZ_TOO_COSTLY, TSZ_GUARDED, TSZ_LOST, TSZ_COLLAPSED or TSZ_DEFERRED; TSZ_NO_EDGE past E.
 *   edge_removed   3 F int32: r of a candidate (lost, collapsed or deferred), -1 otherwise and past E.
 *   edge_guard     3 F bytes: the guard mask of an eligible edge, 0 otherwise and past E.
 *   edge_cost      3 F float64: the cost of a candidate, the reported cost of a TSZ_TOO_COSTLY edge, +inf otherwise and past E.
 *   totals         five 64-bit words {edges, candidates, in_budget, collapsed, too_costly}; candidates counts the deferred ones too.
 * V == 0 or F == 0 is a valid call that writes the empty result, as in ts_collapse.h: with F == 0 only totals (zeros), vertex_target (the
 * identity) and out_quadrics (a copy); with V == 0 nothing takes part, every face is copied and every other entry holds its fill value.
 *
 * Cost.  The front is ts_collapse.h's (csrc/ts_collapse_round.h holds what the two units share).  The ranking is three stable 32-bit
 * radix sorts over the 3 F edge slots, least significant key first: the inverted priority, the low word of the cost, the high word of the
 * cost (all ones for a slot that holds no candidate, which therefore sorts behind every candidate); the slots start in edge order, so the
 * position of a candidate in the result is its rank.
 *
 * Purity (DESIGN.md "Purity of the entry points").  The workspace may hold anything on entry; every output above is overwritten whatever
 * it held; no byte outside tsz_workspace_bytes(V, F) or an output's extent is written.
 */
#ifndef TS_DECIMATE_H
#define TS_DECIMATE_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSZ_NO_EDGE 0
#define TSZ_NOT_ELIGIBLE 1
#define TSZ_TOO_COSTLY 2
#define TSZ_GUARDED 3
#define TSZ_LOST 4
#define TSZ_COLLAPSED 5
#define TSZ_DEFERRED 6

#define TSZ_GUARD_LINK 1
#define TSZ_GUARD_LONG 2
#define TSZ_GUARD_NORMAL 4
#define TSZ_GUARD_HELD 8

#define TSZ_MAX_RING 64

/* The text of the calling thread's last error of this library. */
const char *tsz_last_error(void);

/* Bytes of device workspace that serve either call below for V vertices and F faces.  Monotonic in V and in F. */
size_t tsz_workspace_bytes(int32_t V, int32_t F);

/* vertices: V*3 floats; faces: F*3 int32; keep: F bytes or NULL; out_quadrics: V*10 float64, 8-byte aligned, overwritten.  The workspace
 * is needed with F > 0 and V > 0. */
int tsz_vertex_quadrics(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, double *out_quadrics,
                        void *workspace, size_t workspace_bytes, void *stream);

/* vertices: V*3 floats; faces: F*3 int32; keep: F bytes or NULL; pinned: V bytes or NULL; quadrics: V*10 float64; max_cost >= 0, +inf for
 * none; max_collapses >= 0; max_edge > 0, +inf for none; min_cos in [0, 1], formed by the caller as for ts_collapse.h; seed: mixed into the
 * priorities; out_faces: F*3 int32, out_keep: F bytes, vertex_target: V int32 and out_quadrics: V*10 float64, or all four NULL;
 * edge_vertices: 3*F*2 int32; edge_state, edge_guard: 3*F bytes; edge_removed: 3*F int32; edge_cost: 3*F float64; totals: five 64-bit
 * device words, overwritten.  The workspace is needed with F > 0.  F is at most 536870911 and V + 3*F at most 2147483647. */
int tsz_decimate(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, const uint8_t *pinned,
                 const double *quadrics, float max_cost, int32_t max_collapses, float max_edge, float min_cos, uint32_t seed,
                 int32_t *out_faces, uint8_t *out_keep, int32_t *vertex_target, double *out_quadrics, int32_t *edge_vertices,
                 uint8_t *edge_state, int32_t *edge_removed, uint8_t *edge_guard, double *edge_cost, unsigned long long *totals,
                 void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_DECIMATE_H */
