/*
 * ts_smooth.h -- C ABI of libts_smooth.so: the one-ring of every vertex of an indexed triangle mesh, Taubin lambda|mu smoothing over it, and
 * the unit normals of faces and vertices.  diff_recon_hip/mesh_smooth.py builds vertex_adjacency, smooth_mesh, face_normals, vertex_normals,
 * smooth_fused, mesh_normal_consistency and save_glb_shaded_mesh on it.
 *
 * A library of its own, beside libts2d.so, libts_geom.so, libts_bvh.so, libts_ray.so, libts_volume.so, libts_color.so and libts_simplify.so:
 * the export lists of all seven are closed.  It links the product's radix sort object and keeps its own error text.  The error codes are
 * ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, a lambda or mu that is NaN or infinite, a negative iteration count, a
 * max_move that is NaN or negative, a mode other than those below, a null required pointer, a workspace below tss_workspace_bytes(V, F)
 * return TS2D_ERR_INVALID with the text in tss_last_error(); more than 357913941 faces (6 F adjacency slots) is TS2D_ERR_CAPACITY.
 * V == 0 is a no-op that returns TS2D_OK, except that counts is still overwritten.
 *
 * The result is a pure function of the input: no floating-point atomics, no dependence on thread order.  All arithmetic is float64 on the
 * fp32 inputs widened, every operation rounded (the unit is built with -ffp-contract=off), written operation by operation in
 * tests/ref_mesh_smooth.py.
 *
 * Adjacency (tss_adjacency).  A face TAKES PART iff keep[f] != 0 (a NULL keep means all faces), its three indices lie in [0, V) and are
 * pairwise distinct.  Vertex coordinates are not read.  A participating face (a, b, c) contributes six directed records (src, dst):
 * (a,b) (b,a) (b,c) (c,b) (c,a) (a,c).
 *   offsets      V + 1 int32; row v is [offsets[v], offsets[v + 1]).
 *   neighbors    6 F int32; row v holds the distinct dst of the records with src == v, ascending.  Entries from offsets[V] on are -1.
 *   edge_faces   6 F int32, parallel to neighbors: the number of records equal to that (src, dst), which is the number of participating
 *                faces that use the undirected edge.  Entries from offsets[V] on are 0.  The table is symmetric by construction.
 *   vertex_class V bytes: TSS_ISOLATED an empty row; TSS_NONMANIFOLD some entry's count is 3 or more; TSS_BOUNDARY some count is 1 and none is
 *                3 or more; TSS_INTERIOR every count is 2.  A vertex where two closed fans touch is INTERIOR by this rule: the class looks at
 *                edges, not at the fan around the vertex.
 *   counts       four 64-bit words {entries, boundary, manifold, nonmanifold}, counted over entries: each is exactly twice the matching
 *                count of ts2d_weld_edge_census on the same faces whenever no participating face repeats an index (the census does not
 *                apply the distinctness rule).
 * With F == 0 every row is empty and every class TSS_ISOLATED.
 *
 * Smoothing (tss_smooth), gather form.  offsets, neighbors, edge_faces and vertex_class are tss_adjacency's (or any table of that shape);
 * num_entries is the number of elements of neighbors and of edge_faces that may be read: a row is cut at it, and an entry outside [0, V)
 * is skipped, so a foreign table stays in bounds.  edge_faces is required in TSS_BOUNDARY_CURVE only.
 *   state     q, float64 (V x 3), in the workspace in two buffers; q0 = the input widened.  The state stays float64 between the steps and is
 *             rounded to fp32 once, at the end.
 *   live      a vertex is LIVE iff its three input coordinates are finite.  A vertex that is not live never moves, never enters a sum, and
 *             its output row is its input row bit for bit.
 *   who moves never: an ISOLATED vertex, a pinned one (pinned[i] != 0; a NULL pinned pins nothing), one that is not live.
 *             TSS_BOUNDARY_FIXED  BOUNDARY and NONMANIFOLD vertices do not move; INTERIOR vertices use their whole row.
 *             TSS_BOUNDARY_CURVE  a BOUNDARY vertex uses only its entries with edge_faces == 1, so it slides along the boundary curve;
 *                                 NONMANIFOLD does not move; INTERIOR uses its whole row.
 *             TSS_BOUNDARY_FREE   every vertex with a non-empty row uses its whole row.
 *   one step with factor k.  Every read is from the previous state (Jacobi: ping-pong, never in place).  For a moving vertex i:
 *             s = the per-axis float64 sum, from 0, of q_j over the LIVE members j of its stencil in ascending neighbour order, n their
 *             number.  n == 0 leaves the vertex where it is; otherwise m = s / (double)n, d = m - q_i, q'_i = q_i + k d.  A vertex that
 *             does not move copies its state.
 *   iteration = the step with (double)lambda, then the step with (double)mu.  Both always run, so mu = 0 is the plain Laplacian.
 *             iterations == 0 returns the input bits.
 *   result    for a vertex that may move: out = (float) min(max(q, q0 - max_move), q0 + max_move) per axis, in float64 (max_move widened;
 *             +inf means no bound).  No vertex ends farther than max_move from where it started, on any axis.  Every other vertex is
 *             copied bit for bit.
 *
 * Face normals (tss_face_normals).  A face takes part iff it is kept, its indices lie in [0, V) and its nine coordinates are finite; the
 * indices need not be distinct (a degenerate face comes out invalid).  With p_k widened, e1 = p1 - p0, e2 = p2 - p0:
 * nx = e1y e2z - e1z e2y, ny = e1z e2x - e1x e2z, nz = e1x e2y - e1y e2x (ts_simplify.h's cross product), l2 = (nx nx + ny ny) + nz nz.
 * If l2 is finite and > 0: l = sqrt(l2), the row is (float)(n / l) and face_valid = 1; otherwise the row is 0 and face_valid = 0.
 *
 * Vertex normals (tss_vertex_normals).  Per vertex the float64 sum, from 0, over its incident participating faces in ascending face index; a
 * face counts once for a vertex, however often it names it.  TSS_NORMAL_AREA sums n itself (area weights, no square root in the sum);
 * TSS_NORMAL_UNIFORM sums n / l of the faces with a valid normal.  The sum is normalised by the rule above into vertex_normal and
 * vertex_valid; normal_sum (V x 3 float64, may be NULL) receives the raw sums, the part of the contract that needs no square root.
 * Angle weights are out of scope: they need an arc cosine, which no two libraries round alike.  The square root and the division are the
 * correctly rounded IEEE operations.
 *
 * Cost.  tss_adjacency is two stable LSD radix sorts of 6 F pairs on the bits of V, a prefix sum over 6 F head flags in the block-sum form
 * (every block adds the sums in front of it: nobody waits for anybody) and a lower-bound search per row.  tss_smooth is one launch per
 * step, 2 * iterations in all; a vertex is ONE thread's work and its sum is sequential by definition, so a hub of degree 10^5 is a serial
 * walk, as ts_simplify.h states for its one-cell case; the gather is 24-byte state rows behind a 4-byte index.  tss_vertex_normals is one
 * stable sort of 3 F (vertex, face) records and one thread per vertex, linear in the largest fan.
 *
 * Purity (DESIGN.md "Purity of the entry points").  One workspace serves every call in any order and may hold anything on entry; offsets,
 * all 6 F entries of neighbors and edge_faces, vertex_class, counts, out_vertices, face_normal, face_valid, vertex_normal, vertex_valid and
 * normal_sum are overwritten whatever they held; no byte outside tss_workspace_bytes(V, F) or an output's extent is written.
 */
#ifndef TS_SMOOTH_H
#define TS_SMOOTH_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSS_ISOLATED 0
#define TSS_INTERIOR 1
#define TSS_BOUNDARY 2
#define TSS_NONMANIFOLD 3

#define TSS_BOUNDARY_FIXED 0
#define TSS_BOUNDARY_CURVE 1
#define TSS_BOUNDARY_FREE 2

#define TSS_NORMAL_AREA 0
#define TSS_NORMAL_UNIFORM 1

/* The text of the calling thread's last error of this library. */
const char *tss_last_error(void);

/* Bytes of device workspace that serve every call below for V vertices and F faces.  Monotonic in V and in F. */
size_t tss_workspace_bytes(int32_t V, int32_t F);

/* faces: F*3 int32 (NULL with F == 0); keep: F bytes or NULL; offsets: V+1 int32; neighbors, edge_faces: 6*F int32; vertex_class: V bytes;
 * counts: four 64-bit device words {entries, boundary, manifold, nonmanifold}, overwritten.  F is at most 357913941. */
int tss_adjacency(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep, int32_t *offsets, int32_t *neighbors,
                  int32_t *edge_faces, uint8_t *vertex_class, unsigned long long *counts, void *workspace, size_t workspace_bytes,
                  void *stream);

/* vertices, out_vertices: V*3 floats (they may not alias); offsets: V+1 int32; neighbors, edge_faces: num_entries int32 (edge_faces may be
 * NULL outside TSS_BOUNDARY_CURVE); vertex_class: V bytes; pinned: V bytes or NULL.  The workspace is tss_workspace_bytes(V, 0) or more. */
int tss_smooth(int32_t V, const float *vertices, const int32_t *offsets, const int32_t *neighbors, const int32_t *edge_faces,
               int32_t num_entries, const uint8_t *vertex_class, const uint8_t *pinned, float lambda, float mu, int32_t iterations,
               int32_t boundary_mode, float max_move, float *out_vertices, void *workspace, size_t workspace_bytes, void *stream);

/* vertices: V*3 floats; faces: F*3 int32; keep: F bytes or NULL; face_normal: F*3 floats; face_valid: F bytes.  No workspace. */
int tss_face_normals(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, float *face_normal,
                     uint8_t *face_valid, void *stream);

/* vertices: V*3 floats; faces: F*3 int32 (NULL with F == 0); keep: F bytes or NULL; vertex_normal: V*3 floats; vertex_valid: V bytes;
 * normal_sum: V*3 doubles or NULL.  F is at most 357913941. */
int tss_vertex_normals(int32_t V, int32_t F, const float *vertices, const int32_t *faces, const uint8_t *keep, int32_t weighting,
                       float *vertex_normal, uint8_t *vertex_valid, double *normal_sum, void *workspace, size_t workspace_bytes,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_SMOOTH_H */
