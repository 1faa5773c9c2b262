/*
 * ts_holes.h -- C ABI of libts_holes.so: the boundary loops of an indexed triangle mesh, found, ordered and numbered on the device, and the
 * centroid fans that close the short ones.  diff_recon_hip/mesh_holes.py builds boundary_loops, loop_vertices, fill_holes and fill_fused on it
 * (DESIGN.md 16k).
 *
 * A library of its own, beside libts2d.so, libts_geom.so, libts_bvh.so, libts_ray.so, libts_volume.so, libts_color.so, libts_simplify.so and
 * libts_smooth.so: the export lists of all eight are closed.  It links no other product object and keeps its own error text.  The error
 * codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, a negative num_entries, a negative max_loop_edges, num_loops above F or
 * num_members above 3 F, a null required pointer, a workspace below tsh_workspace_bytes(V, F) return TS2D_ERR_INVALID with the text in
 * tsh_last_error(); more than 357913941 faces (3 F half-edges, and ts_smooth.h's table) is TS2D_ERR_CAPACITY.
 *
 * The result is a pure function of the input: the only atomics are integer adds and minima, nothing depends on thread order.  The
 * arithmetic of the fill is float64 on the fp32 inputs widened, every operation rounded (the unit is built with -ffp-contract=off), written
 * operation by operation in tests/ref_mesh_holes.py.
 *
 * Half-edges.  Face f, corner k, is half-edge h = 3 f + k; its TAIL is faces[f][k], its HEAD faces[f][(k + 1) % 3].  A face TAKES PART by
 * ts_smooth.h's rule: keep[f] != 0 (a NULL keep means all faces), its three indices lie in [0, V) and are pairwise distinct.
 * offsets, neighbors, edge_faces are tss_adjacency's table for the same faces and the same keep (or any table of that shape); num_entries is
 * the number of elements of neighbors and edge_faces that may be read.  The row of the tail is cut to [max(offsets[tail], 0),
 * min(offsets[tail + 1], num_entries)) and the head is looked up in it by a lower-bound binary search (lo = m + 1 while neighbors[m] < head,
 * m = lo + (hi - lo) / 2).  A pair that is not found is not boundary, so a foreign table stays in bounds.
 * A half-edge is BOUNDARY iff its face takes part and edge_faces of its entry is 1.
 *
 * Simple vertices and successors.  Over the boundary half-edges, a vertex is SIMPLE iff exactly one has it as tail and exactly one has it as
 * head.  The successor of a boundary half-edge is the boundary half-edge whose tail is its head, if that head is simple; otherwise it has
 * none.  Successors are injective, so the boundary half-edges form disjoint simple cycles and simple paths that end where a vertex is not
 * simple.
 *
 * Loops.  A LOOP is a cycle; its HEAD is its smallest half-edge; its members are listed from the head along the successors; loops are numbered
 * in ascending head.  The half-edges on paths are OPEN: they are counted and never filled.  A pinch or bow-tie vertex (two holes that meet in
 * one vertex) is not simple and opens both holes that meet there: this is stated, not fixed.  With tss_adjacency's own table no loop is
 * shorter than 3, and every face contributes to at most one loop, so there are at most F loops.
 *
 * tsh_loops writes every element of its outputs:
 *   half_edge_loop   3 F int32: the loop of every half-edge, or -1.
 *   loop_offsets     F + 1 int32: loop i is [loop_offsets[i], loop_offsets[i + 1]) of loop_half_edges; entries past the number of loops hold
 *                    the member total.
 *   loop_half_edges  3 F int32: the members, loop by loop; -1 past the member total.
 *   counts           four 64-bit words {boundary half-edges, half-edges on loops, loops, non-simple boundary vertices}; a non-simple boundary
 *                    vertex is one that some boundary half-edge names as tail or head and that is not simple.
 * V == 0 or F == 0: nothing takes part; the outputs say so (-1, 0, -1) and the counters are 0.
 *
 * Filling (tsh_fill).  loop_offsets (num_loops + 1) and loop_half_edges (num_members) are tsh_loops' (the host knows both counts from
 * `counts`), or any table of that shape: loop i is cut to [clamp(loop_offsets[i], 0, num_members), clamp(loop_offsets[i + 1], that,
 * num_members)).  Its length is L, its member tails are a_0 .. a_{L-1}.  Its status is the first rule that applies:
 *   TSH_TOO_LONG   L > max_loop_edges.  Its members and vertices are not read.
 *   TSH_LONE_FACE  L == 3 and the three members are one face's: the outline of a lone triangle, not a hole.
 *   TSH_DEAD       some a_i has a coordinate that is not finite (or, in a foreign table, L < 3, some member lies outside [0, 3 F) or some
 *                  tail outside [0, V)).
 *   TSH_FILLED     otherwise.
 * A filled loop with L == 3 gives the one face (a_0, a_2, a_1) and no vertex.  Any other filled loop gives one new vertex c: per axis
 * c = (float)(s / (double)L), s the float64 sum, from 0, of the widened coordinates in member order; and the L faces (a_{i+1}, a_i, c),
 * i = 0 .. L-1, a_L = a_0.  They run against the boundary, so the orientation of the mesh continues over the cap.  New vertices are numbered
 * V, V + 1, ... in ascending loop; new faces are in ascending loop, then i.
 * attributes (V x channels fp32, NULL with channels == 0) and attr_valid (V bytes, NULL: all valid): per channel the same sequential sum
 * over the members whose attribute is valid, n their number; n > 0 gives (float)(s / (double)n) and a valid byte 1, otherwise 0 and 0.
 *
 * tsh_fill writes every element of its outputs, to their capacity:
 *   loop_status      num_loops bytes.
 *   new_vertices     num_loops x 3 fp32: the new vertices in order, 0 past their number.
 *   new_attributes   num_loops x channels fp32, new_attr_valid num_loops bytes, likewise (not touched with channels == 0).
 *   new_faces        num_members x 3 int32: the new faces in order, -1 past their number.
 *   new_face_loop    num_members int32: the loop of every new face, -1 past their number.
 *   totals           three 64-bit words {filled loops, new vertices, new faces}.
 *
 * Cost.  tsh_loops is one lower-bound search per half-edge, a census with integer atomics, and two rounds of pointer doubling over all 3 F
 * half-edges -- the loop labels (jump, smallest label, open flag), then the ranks (Wyllie, the cycle cut in front of its head) -- of
 * ceil(log2(max(min(3 F, V + 1), 2))) launches each, every read from the previous round's buffer; then a prefix sum over head flags and loop
 * lengths in the block-sum form (every block adds the sums in front of it: nobody waits for anybody) and one scatter.  tsh_fill decides the
 * status and sums the vertices with ONE thread per loop, linear in L, as ts_smooth.h states for its hub: a loop of 10^5 edges is a serial
 * walk unless max_loop_edges turns it away; one thread per member writes the faces.
 *
 * Purity (DESIGN.md "Purity of the entry points").  One workspace serves both calls in any order and may hold anything on entry; every output
 * above is overwritten whatever it held; no byte outside tsh_workspace_bytes(V, F) or an output's extent is written.
 */
#ifndef TS_HOLES_H
#define TS_HOLES_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSH_FILLED 0
#define TSH_TOO_LONG 1
#define TSH_LONE_FACE 2
#define TSH_DEAD 3

/* The text of the calling thread's last error of this library. */
const char *tsh_last_error(void);

/* Bytes of device workspace that serve both calls below for V vertices and F faces.  Monotonic in V and in F. */
size_t tsh_workspace_bytes(int32_t V, int32_t F);

/* faces: F*3 int32; keep: F bytes or NULL; offsets: V+1 int32; neighbors, edge_faces: num_entries int32; half_edge_loop, loop_half_edges:
 * 3*F int32; loop_offsets: F+1 int32; counts: four 64-bit device words, overwritten.  F is at most 357913941. */
int tsh_loops(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep, const int32_t *offsets, const int32_t *neighbors,
              const int32_t *edge_faces, int32_t num_entries, int32_t *half_edge_loop, int32_t *loop_offsets, int32_t *loop_half_edges,
              unsigned long long *counts, void *workspace, size_t workspace_bytes, void *stream);

/* vertices: V*3 floats; faces: F*3 int32; loop_offsets: num_loops+1 int32; loop_half_edges: num_members int32; attributes: V*channels floats
 * or NULL with channels == 0; attr_valid: V bytes or NULL; loop_status, new_attr_valid: num_loops bytes; new_vertices: num_loops*3 floats;
 * new_attributes: num_loops*channels floats; new_faces: num_members*3 int32; new_face_loop: num_members int32; totals: three 64-bit device
 * words, overwritten.  num_loops is at most F, num_members at most 3*F. */
int tsh_fill(int32_t V, int32_t F, const float *vertices, const int32_t *faces, int32_t num_loops, const int32_t *loop_offsets,
             const int32_t *loop_half_edges, int32_t num_members, int32_t max_loop_edges, const float *attributes, const uint8_t *attr_valid,
             int32_t channels, uint8_t *loop_status, float *new_vertices, float *new_attributes, uint8_t *new_attr_valid, int32_t *new_faces,
             int32_t *new_face_loop, unsigned long long *totals, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_HOLES_H */
