/*
 * ts_volume.h -- C ABI of libts_volume.so: per-view depth fused into a truncated signed distance (TSDF) volume held in integers, the
 * volume's field, and the level set of any fp32 grid extracted by marching tetrahedra as one oriented, closed triangle soup.
 * diff_recon_hip/volume.py builds TSDFVolume, extract_isosurface and fuse_mesh on it.
 *
 * A library of its own, beside libts2d.so, libts_geom.so, libts_bvh.so and libts_ray.so: the export lists of all four are closed.
 * libts_volume.so links no object of the others and keeps its own error text.  The error codes are ts2d.h's.
 *
 * All pointers are device pointers; everything is enqueued on `stream` (a hipStream_t); no call allocates or synchronises with the host, so the
 * calls can be captured in a graph.
 * Argument checks are decided before any HIP call: a dimension below 1, a null required pointer, h or trunc (or a tangent) that is NaN,
 * infinite or not positive, an image size below 1, flags other than 0 or TSV_CARVE_UNCOVERED, min_weight below 1, iso NaN or infinite, a
 * negative capacity, a workspace below its size query return TS2D_ERR_INVALID with the text in the last-error call of this header.  A grid
 * of more than 2^27 samples, or an image of more than 2^31 - 1 pixels, is TS2D_ERR_CAPACITY.
 *
 * The volume.  nx * ny * nz samples; sample (i, j, k) has the linear index n = (k ny + j) nx + i and sits at
 * p[a] = (double)o[a] + (double)h * idx[a], o = (ox, oy, oz).  The state is two arrays over n: sum (int64) and weight (int32).
 * The units are built with -ffp-contract=off.  Everything below is float64, computed from the fp32 inputs widened to double, with every
 * operation rounded.
 *
 * Integration of one view.  One thread per sample, no atomics on the state.  M = the 16 floats of world_view_transform in the row-vector
 * convention (M[r][c] = view[4 r + c]).
 *   1  v[c] = ((p0 M[0][c] + p1 M[1][c]) + p2 M[2][c]) + M[3][c], z = v[2]; skipped unless z is finite and > 0.
 *   2  u = (v0 / (z tan_fovx) + 1) (0.5 W), col = floor(u); row likewise from v1, tan_fovy, H: the inverse of the pixel-centre rays of
 *      diff_recon_hip.camera_rays.  Skipped unless 0 <= col < W and 0 <= row < H (a NaN fails the test).
 *   3  skipped if `mask` (H W bytes, optional) is 0 at the pixel.
 *   4  d = depth[row W + col].  Skipped if d is NaN, infinite or < 0.  d == 0 is an uncovered pixel: with TSV_CARVE_UNCOVERED q = 2^20
 *      (free space), otherwise skipped.  Else sd = d - z; skipped if sd < -trunc; s = min(sd / trunc, 1.0), q = (int64) rint(s 2^20).
 *   5  sum += q, weight += 1.  A sample whose weight is INT32_MAX is skipped.
 *   6  `updated` (optional, one caller-cleared 64-bit word) gains the number of samples updated.
 * The sums are integers: the state after any set of views is bit-identical in any order, and the states of two volumes can be added.
 * Only updated samples are read and written back.
 *
 * Field.  field[n] = weight >= min_weight ? (float)((double)sum / ((double)weight 2^20)) : NaN (0x7FC00000).
 *
 * Extraction: marching tetrahedra on any fp32 grid.  A NaN or infinite value is "no data".  Cell (i, j, k), i < nx - 1, j < ny - 1,
 * k < nz - 1, has the corners c = bit0 x + bit1 y + bit2 z and is ACTIVE iff all eight corner values are finite.  Its six tetrahedra, in
 * order: (0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7) (0,4,5,7) (0,4,6,7).  INSIDE is f < iso, strictly.  By the number of inside corners of a
 * tetrahedron: one -- a triangle on the edges (in, out_k), out_k in tetrahedron order; three -- a triangle on the edges (out, in_k); two,
 * inside a, b and outside c, d in tetrahedron order -- the quad q0 = (a,c), q1 = (a,d), q2 = (b,d), q3 = (b,c) as (q0,q1,q2), (q0,q2,q3).
 * A triangle's 2nd and 3rd vertices are swapped where needed so that its normal points from inside to outside: one bit per (tetrahedron,
 * case), derived in exact integers by tests/ref_volume.py and carried by the kernel.
 * The vertex of an edge is a function of the edge alone: endpoints ordered by linear sample index a < b, t = (iso - fa) / (fb - fa),
 * g = ga + t (gb - ga) per axis in grid units, world = (double)o + (double)h g rounded to fp32.  Every tetrahedron that shares an edge
 * writes the same bits, so welding exact duplicates closes the soup; the decomposition is translation-invariant, so neighbouring cells
 * agree on every face diagonal.
 * Output: `triangles` = capacity * 9 floats (three private vertices per triangle), in ascending cell index, then tetrahedron, then the
 * order above; `cell` (optional, capacity int32) = the linear sample index of the triangle's cell corner 0; `total` = one int64 that always
 * receives the full count.  Only the first min(total, capacity) triangles are written.  capacity == 0 is the counting call (triangles may
 * be NULL); a second call depends on nothing the first left behind.
 *
 * Purity (DESIGN.md "Purity of the entry points").  The workspace and the outputs may hold anything on entry; field and total are
 * overwritten in full, triangles and cell up to min(total, capacity); sum, weight and updated are caller-owned accumulators; no byte outside
 * the size query or an output's extent is written.
 */
#ifndef TS_VOLUME_H
#define TS_VOLUME_H

#include "ts2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSV_CARVE_UNCOVERED 1 /* a depth of exactly 0 counts as free space instead of being skipped */
#define TSV_MAX_SAMPLES (1 << 27)

/* The text of the calling thread's last error of this library. */
const char *tsv_last_error(void);

/* view: 16 floats; depth: H*W floats; mask: H*W bytes or NULL; sum: nx*ny*nz int64; weight: nx*ny*nz int32; updated: one 64-bit device
 * word that the caller cleared, or NULL. */
int tsv_integrate(int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz, float h, float trunc, const float *view, float tan_fovx,
                  float tan_fovy, int32_t W, int32_t H, const float *depth, const uint8_t *mask, int32_t flags, int64_t *sum, int32_t *weight,
                  unsigned long long *updated, void *stream);

/* field: nx*ny*nz floats. */
int tsv_field(int32_t nx, int32_t ny, int32_t nz, const int64_t *sum, const int32_t *weight, int32_t min_weight, float *field, void *stream);

/* Bytes of device workspace of an extraction: per-cell counts and their prefix sums.  Monotonic in the number of samples. */
size_t tsv_extract_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);

/* field: nx*ny*nz floats; triangles: capacity*9 floats (NULL with capacity 0); cell: capacity int32 or NULL; total: one int64. */
int tsv_extract(int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz, float h, const float *field, float iso, int64_t capacity,
                float *triangles, int32_t *cell, int64_t *total, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TS_VOLUME_H */
