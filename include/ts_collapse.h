/*
 * ts_collapse.h -- C ABI of libts_collapse.so: one round of half-edge collapses of the short edges of an indexed triangle mesh.  A collapse
 * r -> k along an edge {r, k} replaces r by k in every face around r and deletes the two faces on the edge.  No vertex moves: the output's
 * vertices are a subset of the input's, so vertex attributes need no interpolation, and float64 arithmetic appears only in the decisions.
 * diff_recon_hip/mesh_collapse.py builds collapse_edges, short_edges, collapse_short_edges, collapse_fused and isotropic_remesh on it
 * (DESIGN.md 16v).
 *
 * A library of its own, the eighteenth: the export lists of the other seventeen are closed.  It links the product's radix_sort object and no
 * other product object, and keeps its own error text.  The error codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, a min_cos outside [0, 1] (NaN included), a min_edge that is not >= 0
 * (NaN included) in TSP_MARK_SHORTER, a max_edge that is not > 0 (NaN included), an unknown mode, a null required pointer, out_faces,
 * out_keep and vertex_target not given together, a workspace below tsp_workspace_bytes(V, F) return TS2D_ERR_INVALID with the text in
 * tsp_last_error(); TS2D_ERR_CAPACITY where 3 F, 4 F or V + 3 F does not fit the int32 indices (F above 536870911, or V + 3 F above
 * 2147483647): the capacities of ts_flip.h, so that every mesh that can be split and flipped can be collapsed.
 *
 * The result is a pure function of the input: the only atomics are integer adds of counters, nothing depends on thread or launch order.
 * The arithmetic is float64 on the fp32 inputs widened, every operation rounded (the unit is built with -ffp-contract=off), written
 * operation by operation in tests/ref_mesh_collapse.py.  Below, for points p, q: p - q is taken per axis; dot(s, t) = (s.x t.x + s.y t.y) +
 * s.z t.z; cross(s, t) = (s.y t.z - s.z t.y, s.z t.x - s.x t.z, s.x t.y - s.y t.x); length2(i, j) of two vertices is taken from the
 * smaller index to the larger, d = p_max - p_min per axis, length2 = (dx dx + dy dy) + dz dz: ts_subdivide.h's length2 of a finite edge.
 *
 * Taking part.  A face TAKES PART by ts_subdivide.h's rule: keep[f] != 0 (a NULL keep means all faces), its three indices lie in [0, V) and
 * are pairwise distinct.  Half-edge h = 3 f + k runs from faces[f][k] to faces[f][(k + 1) % 3]; the vertex OPPOSITE to it is
 * faces[f][(k + 2) % 3].
 *
 * Edges.  The undirected edges (lo, hi), lo < hi, of the faces that take part are numbered 0 .. E-1 in ascending (lo, hi); `use` is the
 * number of half-edges on the edge.  An edge is CLEAN iff use == 2 and its two half-edges run in opposite directions.
 *
 * Rings.  The RING of a vertex v is the list of the corners of participating faces at v; a ring face is written (v, x, y), rotated so that
 * v comes first, in the face's own order.  x is a RING NEIGHBOUR of v.  Around a vertex all of whose edges are clean every vertex adjacent
 * to v occurs exactly once as x.
 *
 * Vertex classes.  A vertex is FREE iff it is named by a face that takes part, its three coordinates are finite, pinned[v] == 0 (a NULL
 * pinned pins nothing), every edge at it is clean, and its ring has at most TSP_MAX_RING = 64 corners.  Every other vertex is HELD:
 * boundary vertices, vertices on non-manifold edges and pinned vertices are held, so boundaries and caller-chosen features keep their
 * shape exactly.
 *
 * Eligible.  An edge is ELIGIBLE iff it is clean -- one half-edge runs lo -> hi in face f0 with opposite vertex c, the other hi -> lo in
 * face f1 with opposite vertex d -- c != d, the twelve coordinates of lo, hi, c, d are finite (ts_flip.h's rule so far), and at least one
 * of lo, hi is FREE.
 *
 * Short.  An eligible edge is SHORT by the mode, with l2 = length2(lo, hi):
 *   TSP_MARK_SHORTER       l2 < L L with L = (double)min_edge.
 *   TSP_MARK_VERTEX_LIMIT  vertex_limit holds V fp32 values.  If limit[lo] or limit[hi] is NaN the edge is not short; otherwise with
 *                          m = limit[hi] < limit[lo] ? limit[hi] : limit[lo] and L = (double)m it is short iff l2 < L L.
 * A zero-length edge is short under every positive limit.  An eligible edge that is not short is TSP_LONG_ENOUGH.
 *
 * Direction.  A short edge first tries r = hi, k = lo.  If hi is HELD, or a guard fails, it tries r = lo, k = hi.  A direction whose r is
 * HELD is not walked: it adds TSP_GUARD_HELD to the edge's guard mask (the ring guard: a FREE r bounds every walk by TSP_MAX_RING
 * corners).  A direction with a FREE r passes iff the three guards below pass.  Each guard is evaluated over the whole ring of r, without
 * early exit, and every guard that fails adds its bit: the mask of an edge, the OR over the directions tried up to and without the one that
 * passed, is a function of the input alone.
 *   TSP_GUARD_LINK    no ring neighbour x of r other than k, c, d is adjacent to k: (min(x, k), max(x, k)) is not an edge of this round's
 *                     table (binary search over the sorted (lo, hi) columns, as ts_flip.h's guard (i)).  And no ring face (r, x, y) with
 *                     x != k and y != k -- a SURVIVING face -- has {x, y} = {c, d}: the tetrahedron, which would leave two faces on one
 *                     vertex triple.
 *   TSP_GUARD_LONG    for every ring neighbour x != k: length2(k, x) <= (double)max_edge (double)max_edge, by plain arithmetic (for finite
 *                     ends it equals what ts_subdivide.h's edge table reports afterwards bit for bit; a comparison with NaN is false).  max_edge = +inf
 *                     passes every finite edge.  Without this guard split and collapse undo each other.
 *   TSP_GUARD_NORMAL  for every surviving ring face (r, x, y): n0 = cross(p_x - p_r, p_y - p_r), n1 = cross(p_x - p_k, p_y - p_k),
 *                     Q0 = dot(n0, n0), Q1 = dot(n1, n1), D = dot(n0, n1), m = (double)min_cos, M = m m.  The guard passes iff
 *                     Q1 > 0 && (Q0 == 0 || (D > 0 && D D >= (M Q0) Q1)).  No square root, no division; a comparison with NaN is false.
 *                     A face never folds and never degenerates; a face that was degenerate may turn any way; a crease survives because a
 *                     collapse across it turns normals.
 * A short edge with a passing direction is a CANDIDATE and remembers r; a short edge without one is TSP_GUARDED.
 *
 * Selection: an independent set at distance two.  The candidates are ordered by (l2 ascending, priority descending, edge id ascending);
 * l2 is compared as float64; the priority is ts_flip.h's 32-bit mix of (lo, hi, seed), in uint32 arithmetic (wrapping):
 *     h = seed * 0x9E3779B1 + lo;  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h += hi;  h *= 0xC2B2AE35;  h ^= h >> 16.
 * Shortest first; the hash breaks the ties of regular grids, where the edge id alone would let one wavefront win per round.
 *   1. best[v]  is the first candidate in that order among the edges at v (none if there is none).
 *   2. best2[v] is the first among best[u] over u = v and the vertices adjacent to v.
 *   3. a candidate e = {a, b} WINS iff best2[a] == best2[b] == e; it is TSP_COLLAPSED.  The other candidates are TSP_LOST and wait for
 *      the next round.
 * Both steps are gathers over the vertex rings.  No winner has an end inside the closed ring of another winner's end, so the winners' rings
 * share no face, no guard of one reads a vertex, an edge or a face that another changes, and no two winners create the same edge: the
 * round equals the winners applied one after another in any order.
 *
 * The collapse.  vertex_target[v] is k for the r of a winner and v otherwise.  Every participating face maps its three indices through
 * vertex_target: at most one index changes.  A face in which two indices become equal is deleted: out_keep = 0 and the row is copied
 * bit for bit.  Every other participating face keeps its slot and the order of its indices -- its orientation -- with out_keep = 1.  A
 * face that does not take part is copied bit for bit; its out_keep is 1 iff keep was NULL or keep[f] != 0.
 *
 * tsp_collapse runs one round and writes every element of its outputs, to their capacity of F faces, V vertices and 3 F edges:
 *   out_faces      F x 3 int32, out_keep F bytes, vertex_target V int32.  All three NULL: the call classifies only; the selection is still
 *                  made and reported in edge_state and totals.
 *   edge_vertices  3 F x 2 int32: (lo, hi) of edge e; -1 past E.
 *   edge_state     3 F bytes: TSP_NOT_ELIGIBLE, TSP_LONG_ENOUGH, TSP_GUARDED, TSP_LOST or TSP_COLLAPSED; TSP_NO_EDGE past E.
 *   edge_removed   3 F int32: r of a candidate (lost or collapsed), -1 otherwise and past E.
 *   edge_guard     3 F bytes: the guard mask of a short edge, 0 otherwise and past E.
 *   totals         four 64-bit words {edges, short, candidates, collapsed}; short counts the guarded edges too.
 * V == 0 or F == 0 is a valid call that writes the empty result: with F == 0 only totals (zeros) and vertex_target (the identity); with
 * V == 0 nothing takes part, every face is copied and every other entry holds its fill value.
 *
 * Cost.  The front is ts_subdivide.h's: one thread per face writes the half-edge records and the corner records; two stable radix sorts
 * order the half-edges by (lo, hi) (csrc/ts_mesh_edges.h); run heads become edge ids by one prefix sum in block-sum form
 * (csrc/ts_mesh_scan.h: nobody waits for anybody; csrc/ts_mesh_edge_ids.h); one more stable radix sort orders the corners by vertex.  Rings
 * are walked, never stored: one thread per edge flags the clean edges, one per vertex finds its ring bounds and its class, one per edge
 * slot classifies -- only a short eligible edge walks a ring, at most two, each corner a 12-byte row gather or two and one binary
 * search -- one per vertex takes best, one per vertex best2, one per edge decides the winners, one per face gathers its new indices.
 *
 * Purity (DESIGN.md "Purity of the entry points").  The workspace may hold anything on entry; every output above is overwritten whatever
 * it held; no byte outside tsp_workspace_bytes(V, F) or an output's extent is written.
 */
#ifndef TS_COLLAPSE_H
#define TS_COLLAPSE_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSP_NO_EDGE 0
#define TSP_NOT_ELIGIBLE 1
#define TSP_LONG_ENOUGH 2
#define TSP_GUARDED 3
#define TSP_LOST 4
#define TSP_COLLAPSED 5

#define TSP_MARK_SHORTER 1
#define TSP_MARK_VERTEX_LIMIT 2

#define TSP_GUARD_LINK 1
#define TSP_GUARD_LONG 2
#define TSP_GUARD_NORMAL 4
#define TSP_GUARD_HELD 8

#define TSP_MAX_RING 64

/* The text of the calling thread's last error of this library. */
const char *tsp_last_error(void);

/* Bytes of device workspace that serve the call below for V vertices and F faces.  Monotonic in V and in F. */
size_t tsp_workspace_bytes(int32_t V, int32_t F);

/* vertices: V*3 floats; faces: F*3 int32; keep: F bytes or NULL; pinned: V bytes or NULL; mode: TSP_MARK_*; min_edge: read in
 * TSP_MARK_SHORTER; vertex_limit: V floats, read in TSP_MARK_VERTEX_LIMIT; max_edge > 0, +inf for none; min_cos in [0, 1]: the cosine of the
 * largest turn of a face normal, formed by the caller once in float64 and rounded to fp32; seed: mixed into the priorities; out_faces: F*3
 * int32, out_keep: F bytes and vertex_target: V int32, or all three NULL; edge_vertices: 3*F*2 int32; edge_state, edge_guard: 3*F bytes;
 * edge_removed: 3*F int32; totals: four 64-bit device words, overwritten.  The workspace is needed with F > 0.  F is at most 536870911 and
 * V + 3*F at most 2147483647. */
int tsp_collapse(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, const uint8_t *pinned, int32_t mode,
                 float min_edge, const float *vertex_limit, float max_edge, float min_cos, uint32_t seed, int32_t *out_faces,
                 uint8_t *out_keep, int32_t *vertex_target, int32_t *edge_vertices, uint8_t *edge_state, int32_t *edge_removed,
                 uint8_t *edge_guard, unsigned long long *totals, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_COLLAPSE_H */
