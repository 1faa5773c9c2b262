/*
 * ts_subdivide.h -- C ABI of libts_subdivide.so: the unique undirected edges of an indexed triangle mesh with their use counts and lengths,
 * and the conforming 1-to-2/3/4 split of the faces at the midpoints of marked edges.  diff_recon_hip/mesh_subdivide.py builds mesh_edges,
 * split_edges, split_long_edges, subdivide_mesh and split_fused on it.
 *
 * A library of its own, the sixteenth: the export lists of the other fifteen are closed.  It links the product's radix_sort object and no
 * other product object, and keeps its own error text.  The error codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, a negative channels, an unknown mode, a max_edge that is not >= 0 (NaN
 * included) in TSD_MARK_LONGER, a null required pointer, a workspace below tsd_workspace_bytes(V, F) return TS2D_ERR_INVALID with the text
 * in tsd_last_error(); TS2D_ERR_CAPACITY where 3 F, 4 F or V + 3 F does not fit the int32 indices (F above 536870911, or V + 3 F above
 * 2147483647).
 *
 * The result is a pure function of the input: the only atomics are integer adds of counters, nothing depends on thread or launch order.
 * The arithmetic is float64 on the fp32 inputs widened, every operation rounded (the unit is built with -ffp-contract=off), written
 * operation by operation in tests/ref_mesh_subdivide.py.
 *
 * Taking part.  A face TAKES PART by ts_smooth.h's rule: keep[f] != 0 (a NULL keep means all faces), its three indices lie in [0, V) and
 * are pairwise distinct.  Half-edge h = 3 f + k runs from faces[f][k] to faces[f][(k + 1) % 3].
 *
 * Edges.  The undirected edges (lo, hi), lo < hi, of the faces that take part are numbered 0 .. E-1 in ascending (lo, hi).  Every half-edge
 * learns the id of its edge, -1 where its face does not take part.
 *   use      the number of half-edges on the edge: the number of participating faces on it.
 *   length2  in float64 on the widened coordinates: with d = p_hi - p_lo per axis, length2 = (dx dx + dy dy) + dz dz.  Always taken from lo
 *            to hi, once per edge: both neighbours see one value.  An edge is FINITE iff all six coordinates of its ends are; the length2
 *            of an edge that is not finite is the quiet NaN 0x7FF8000000000000 whatever the arithmetic would give.  A finite edge whose
 *            squares overflow has length2 = +inf.
 *
 * Marks.  In every mode an edge is marked only if it is finite.
 *   TSD_MARK_ALL           every finite edge is marked.
 *   TSD_MARK_LONGER        marked iff length2 > (double)max_edge (double)max_edge.  A zero-length edge is never marked.
 *   TSD_MARK_VERTEX_LIMIT  vertex_limit holds V fp32 values.  If limit[lo] or limit[hi] is NaN the edge is not marked; otherwise with
 *                          m = limit[hi] < limit[lo] ? limit[hi] : limit[lo] and L = (double)m it is marked iff length2 > L L.
 *
 * New vertices.  Every marked edge gets one new vertex, numbered V + r, r the rank of the edge among the marked edges in ascending edge id.
 * Its position per axis is (float)((p_lo + p_hi) 0.5) in float64.  attributes (V x channels fp32, NULL with channels == 0) and attr_valid
 * (V bytes, NULL: all valid): both ends valid gives (float)((a_lo + a_hi) 0.5) per channel in float64 and a valid byte 1; exactly one end
 * valid gives that end's values bit for bit and 1; neither gives 0 and 0.  new_vertex_edge records (lo, hi).
 *
 * Faces.  The output replaces the input's face list: output faces come in ascending parent face, the pieces of one parent in the order
 * below; out_face_parent names the parent of every output face.  A face that does not take part is copied bit for bit as one output face.
 * For a participating face (v0, v1, v2), m_k is the new vertex on half-edge k if that edge is marked:
 *   0 marked  the face is copied.
 *   1 marked  at corner k; a = v_k, b = v_{k+1}, c = v_{k+2}, m = m_k: (a, m, c), (m, b, c).
 *   2 marked  corner k the unmarked one; a = v_k, b = v_{k+1}, c = v_{k+2}, m1 on (b, c), m2 on (c, a): first (m1, c, m2); then the quad
 *             (a, b, m1, m2) is cut by its shorter diagonal.  The two lengths are float64 squared lengths formed as length2 above, from
 *             the fp32 positions of a and m1, and of b and m2, as written to the outputs.  Diagonal a-m1 wins if it is strictly shorter;
 *             on a tie (two +inf included) it wins iff a < b as indices.  a-m1 gives (a, b, m1), (a, m1, m2); b-m2 gives (a, b, m2),
 *             (b, m1, m2).
 *   3 marked  (v0, m0, m2), (m0, v1, m1), (m2, m1, v2), (m0, m1, m2).
 * Every piece keeps its parent's orientation.  Marks belong to edges, so the two faces of an edge agree about its midpoint, and no output
 * vertex lies inside an output edge of a participating face: the split is conforming.  A face masked out by keep (or one that does not
 * take part for another reason) next to a split edge KEEPS its long edge: the new vertex lies inside that edge, a T-junction the caller
 * asked for.
 *
 * tsd_edges writes every element of its outputs, to their capacity of 3 F edges:
 *   edge_vertices   3 F x 2 int32: (lo, hi) of edge e; -1 past E.
 *   edge_use        3 F int32; 0 past E.
 *   edge_length2    3 F float64, or NULL: then no length is formed and `vertices` is not read (it may be NULL); 0 past E.
 *   half_edge_edge  3 F int32: the edge of every half-edge, or -1.
 *   counts          four 64-bit words {edges, boundary (use == 1), manifold (use == 2), nonmanifold (use >= 3)}: half of tss_adjacency's
 *                   entry counts on the same faces.
 * tsd_split runs one round and writes every element of its outputs, to their capacity of 3 F new vertices and 4 F faces:
 *   new_vertices     3 F x 3 fp32: the new vertices in order, 0 past their number.
 *   new_attributes   3 F x channels fp32, new_attr_valid 3 F bytes, likewise (not touched with channels == 0).
 *   new_vertex_edge  3 F x 2 int32: -1 past the number of new vertices.
 *   out_faces        4 F x 3 int32: -1 past the number of output faces.
 *   out_face_parent  4 F int32: likewise.
 *   totals           four 64-bit words {edges, marked, out_faces, faces_split}; faces_split counts the parents with more than one piece.
 * V == 0 or F == 0 is a valid call that writes the empty result: with F == 0 only counts / totals (zeros); with V == 0 nothing takes part,
 * every face is copied and every other entry holds its fill value.
 *
 * Cost.  One thread per face writes the half-edge records; two stable radix sorts order them by (lo, hi) (csrc/ts_mesh_edges.h); run heads
 * become edge ids by one prefix sum in block-sum form (csrc/ts_mesh_scan.h: nobody waits for anybody); one thread per edge forms length2,
 * the mark and the use count; a second prefix sum over the marks numbers the new vertices and writes them in its apply pass; one scatter
 * hands edge and midpoint ids to the half-edges; a third prefix sum over the per-face piece counts (1 to 4) places the output faces, and
 * one thread per parent writes its pieces.
 *
 * Purity (DESIGN.md "Purity of the entry points").  One workspace serves both calls in any order and may hold anything on entry; every
 * output above is overwritten whatever it held; no byte outside tsd_workspace_bytes(V, F) or an output's extent is written.
 */
#ifndef TS_SUBDIVIDE_H
#define TS_SUBDIVIDE_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSD_MARK_ALL 0
#define TSD_MARK_LONGER 1
#define TSD_MARK_VERTEX_LIMIT 2

/* The text of the calling thread's last error of this library. */
const char *tsd_last_error(void);

/* Bytes of device workspace that serve both calls below for V vertices and F faces.  Monotonic in V and in F. */
size_t tsd_workspace_bytes(int32_t V, int32_t F);

/* vertices: V*3 floats, or NULL with edge_length2 NULL; faces: F*3 int32; keep: F bytes or NULL; edge_vertices: 3*F*2 int32; edge_use,
 * half_edge_edge: 3*F int32; edge_length2: 3*F doubles or NULL; counts: four 64-bit device words, overwritten.  The workspace is needed
 * with F > 0.  F is at most 536870911 and V + 3*F at most 2147483647. */
int tsd_edges(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, int32_t *edge_vertices,
              int32_t *edge_use, double *edge_length2, int32_t *half_edge_edge, unsigned long long *counts, void *workspace,
              size_t workspace_bytes, void *stream);

/* vertices: V*3 floats; faces: F*3 int32; keep: F bytes or NULL; mode: TSD_MARK_*; max_edge: read in TSD_MARK_LONGER; vertex_limit: V
 * floats, read in TSD_MARK_VERTEX_LIMIT; attributes: V*channels floats or NULL with channels == 0; attr_valid: V bytes or NULL;
 * new_vertices: 3*F*3 floats; new_attributes: 3*F*channels floats; new_attr_valid: 3*F bytes; new_vertex_edge: 3*F*2 int32; out_faces:
 * 4*F*3 int32; out_face_parent: 4*F int32; totals: four 64-bit device words, overwritten.  The workspace is needed with F > 0. */
int tsd_split(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, int32_t mode, float max_edge,
              const float *vertex_limit, const float *attributes, const uint8_t *attr_valid, int32_t channels, float *new_vertices,
              float *new_attributes, uint8_t *new_attr_valid, int32_t *new_vertex_edge, int32_t *out_faces, int32_t *out_face_parent,
              unsigned long long *totals, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_SUBDIVIDE_H */
