/*
 * ts_manifold.h -- C ABI of libts_manifold.so: the fans of every vertex of an indexed triangle mesh, found and numbered on the device, and
 * the split that gives every extra fan a vertex of its own, which makes the mesh edge-manifold and vertex-manifold.
 * diff_recon_hip/mesh_manifold.py builds vertex_fans, split_nonmanifold and manifold_fused on it.
 *
 * A library of its own, beside libts2d.so, libts_geom.so, libts_bvh.so, libts_ray.so, libts_volume.so, libts_color.so, libts_simplify.so,
 * libts_smooth.so and libts_holes.so: the export lists of all nine are closed.  It links the product's radix_sort object and no other, and
 * keeps its own error text.  The error codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a negative count, a negative capacity, a null required pointer, a workspace below
 * tsf_workspace_bytes(V, F) return TS2D_ERR_INVALID with the text in tsf_last_error(); more than 715827882 faces (3 F corners in an int32;
 * the sort's layout asks for no less) is TS2D_ERR_CAPACITY, and so is, for tsf_split, V + 3 F above 2147483647 (the index of a new vertex).
 *
 * The result is a pure function of the input: the only atomics are integer (compare-exchange, minimum, add), nothing depends on thread
 * order.  There is no floating-point arithmetic at all -- positions and attributes are the caller's to copy, bit for bit -- so the unit is
 * built without floating-point flags.  The contract is written operation by operation in tests/ref_mesh_manifold.py.
 *
 * Participation.  A face TAKES PART by ts_smooth.h's rule: keep[f] != 0 (a NULL keep means all faces), its three indices lie in [0, V) and
 * are pairwise distinct.
 *
 * Corners.  Face f, slot k, is CORNER c = 3 f + k at vertex faces[f][k]; it is also half-edge c from that vertex (its tail) to
 * faces[f][(k + 1) % 3] (its head), which is ts_holes.h's numbering.
 *
 * Edge use.  The use count of the undirected edge {a, b} is the number of participating half-edges between a and b in either direction
 * (tss_adjacency's edge_faces).
 *
 * Links.  An edge {a, b} used EXACTLY TWICE, by half-edges of faces f and g, links the corner of f at a to the corner of g at a, and
 * likewise at b; direction does not matter.  An edge used once links nothing; an edge used three times or more links nothing either.
 *
 * Fans.  A FAN is a connected component of the link relation over the participating corners; all corners of a fan sit on one vertex.  A face
 * has exactly two edges at each of its vertices, so a fan is a path or a cycle of faces: that is why the split's result is manifold.
 *
 * tsf_fans writes every element of its outputs:
 *   corner_fan   3 F int32: the smallest corner of every corner's fan, or -1 for a corner of a face that does not take part.
 *   vertex_fans  V int32: the number of fans at every vertex, 0 for a vertex that no participating face names.
 *   counts       six 64-bit words {participating corners, fans, vertices with at least one fan, vertices with two or more fans, edges used
 *                three or more times, edges used exactly twice whose two half-edges run in the SAME direction}.  A same-direction edge is an
 *                orientation conflict: counted, still linked, not fixed.  The number of new vertices of the split is counts[1] - counts[2].
 * V == 0 or F == 0: nothing takes part; the outputs say so (-1, 0) and the counters are 0.
 *
 * Split (tsf_split).  corner_fan is tsf_fans' table for the same faces and the same keep, or any table of that shape: an entry outside
 * [0, 3 F), one that names a corner on a different vertex, or one on a face that does not take part counts as -1:
 * a foreign table stays in bounds.  The labels at a vertex are the entries of its participating corners that count.  At every vertex the fan with the smallest label
 * KEEPS the vertex; every other fan gets a NEW VERTEX; new vertices are numbered V, V + 1, ... in ascending fan label.  A pinch where two
 * holes meet becomes one boundary loop over both copies (two 3-loops become one 6-loop): the topologically honest answer, the holes are
 * merged, not paired.
 *
 * tsf_split writes every element of its outputs, to their capacity:
 *   out_faces          3 F int32: faces with every participating corner replaced by its fan's vertex; the rows of faces that do not take
 *                      part, and corners whose entry counts as -1, are copied bit for bit.
 *   new_vertex_source  capacity int32: the old vertex that new vertex V + i copies; -1 past the number of new vertices.
 *   new_vertex_fan     capacity int32: its fan label; -1 past the number of new vertices.  The host knows the number from tsf_fans' counts, so
 *                      there is no counting call; new vertices past the capacity are numbered and referenced by out_faces, not listed.
 *   totals             two 64-bit words {new vertices, corners rewritten (the corners that moved to a new vertex)}.
 * V == 0 or F == 0: out_faces is faces, the lists hold -1 and the totals are 0.
 *
 * A row that does not take part may name an index in [V, V + new vertices): copied bit for bit, it WOULD take part in the output.  A caller who
 * keeps such rows passes the participation of the input as `keep` to whatever reads the output; the promises below are stated that way.
 *
 * Promises (the reference checks them on every fixture; the device on its own output).  Over the participating faces of the output every
 * vertex has at most one fan and no edge is used three times or more; every edge that was used exactly twice is still used exactly twice, by
 * the same two faces; a second split adds nothing and returns the faces bit for bit; the faces of a manifold input come back bit for bit.
 *
 * Cost.  tsf_fans is two stable LSD sorts of the 3 F half-edge records (key: the larger, then the smaller end, on the bits of V; value: the
 * half-edge), two gathers, one pass over the sorted runs that performs two unions per edge used twice in a lock-free union-find over the 3 F
 * corners (csrc/ts_union_find.h: roots are the smallest index whatever the order of the unions; nobody waits for anybody, there is no lock
 * and no spin loop), one flatten and one vertex pass.  tsf_split is one pass that validates the labels and elects the keepers, a prefix sum
 * of 3 F flags in the block-sum form (every block adds the sums in front of it), a scatter and one pass that writes the faces.
 *
 * Purity (DESIGN.md "Purity of the entry points").  One workspace serves both calls in any order and may hold anything on entry; every output
 * above is overwritten whatever it held; no byte outside tsf_workspace_bytes(V, F) or an output's extent is written.
 */
#ifndef TS_MANIFOLD_H
#define TS_MANIFOLD_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The text of the calling thread's last error of this library. */
const char *tsf_last_error(void);

/* Bytes of device workspace that serve both calls below for V vertices and F faces.  Monotonic in V and in F. */
size_t tsf_workspace_bytes(int32_t V, int32_t F);

/* faces: F*3 int32; keep: F bytes or NULL; corner_fan: 3*F int32; vertex_fans: V int32; counts: six 64-bit device words, overwritten.
 * F is at most 715827882. */
int tsf_fans(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep, int32_t *corner_fan, int32_t *vertex_fans,
             unsigned long long *counts, void *workspace, size_t workspace_bytes, void *stream);

/* faces, out_faces: F*3 int32; keep: F bytes or NULL; corner_fan: 3*F int32; new_vertex_source, new_vertex_fan: capacity int32 (NULL with
 * capacity == 0); totals: two 64-bit device words, overwritten.  F is at most 715827882 and V + 3*F at most 2147483647. */
int tsf_split(int32_t V, int32_t F, const int32_t *faces, const uint8_t *keep, const int32_t *corner_fan, int32_t capacity, int32_t *out_faces,
              int32_t *new_vertex_source, int32_t *new_vertex_fan, unsigned long long *totals, void *workspace, size_t workspace_bytes,
              void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_MANIFOLD_H */
