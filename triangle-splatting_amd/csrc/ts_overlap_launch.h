// ts_overlap_launch.h -- the launchers of mesh_overlap.hip as api_overlap.hip calls them (include/ts_overlap.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_overlap_bvh_bytes(int F); // the index size of F faces, from csrc/ts_bvh_layout.h: what the size query of include/ts_bvh.h answers
size_t ts_overlap_sort_workspace_bytes(int P);
// faces != nullptr: self mode (bvh_b, FB and count_b unused); otherwise the faces of bvh_a against bvh_b
hipError_t ts_overlap_query(int FA, const void *bvh_a, const int32_t *faces, int FB, const void *bvh_b, int32_t *count_a, int32_t *count_b,
                            uint64_t *stats, int capacity, int32_t *pairs, uint8_t *kind, unsigned long long *leaf_visits, hipStream_t s);
hipError_t ts_overlap_sort_pairs(int P, int bits_first, int bits_second, int32_t *pairs, uint8_t *kind, void *ws, hipStream_t s);
