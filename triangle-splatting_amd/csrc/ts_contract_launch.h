// ts_contract_launch.h -- the launchers of mesh_contract.hip as api_contract.hip calls them (include/ts_contract.h is the C ABI over them).
#pragma once
#include "ts2d_common.h"
size_t ts_contract_workspace_bytes(int V, int F);
hipError_t ts_contract_round(int V, int F, const float *vertices, const int32_t *faces, const uint8_t *keep, const uint8_t *pinned,
                             const double *quadrics, float max_cost, int max_collapses, float max_edge, float min_cos, float lambda, float reach,
                             uint32_t seed, int32_t *out_faces, uint8_t *out_keep, int32_t *vertex_target, float *out_vertices,
                             double *out_quadrics, double *vertex_blend, int32_t *edge_vertices, uint8_t *edge_state, int32_t *edge_removed,
                             uint8_t *edge_guard, double *edge_cost, float *edge_position, unsigned long long *totals, void *ws, hipStream_t s);
