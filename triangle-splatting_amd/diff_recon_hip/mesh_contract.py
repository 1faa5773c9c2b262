"""Decimating an indexed mesh to a face budget or an error bound by edge contraction, on the device: rounds of quadric-error collapses that
PLACE the survivor.

    contract_round(vertices, faces, quadrics, max_collapses, keep=None, max_cost=inf, max_edge=inf, max_normal_deg=30.0, pinned=None,
                   regularization=1e-3, reach=1.0, seed=0) -> ContractedRound                    one round
    placed_edges(...)                                                                            the classification of a round alone
    contract_mesh(vertices, faces, target_faces=None, ratio=None, max_cost=inf, ..., quadrics="carried" | "memoryless" | tensor,
                  regularization=1e-3, reach=1.0, max_rounds=256, compact=True, attributes=None,
                  attribute_valid=None) -> ContractedMesh                                        rounds until the budget is met
    contract_fused(mesh, ...)                                                                    the pass behind a weld, a fusion, a remesh, a split or a flip

mesh_decimate.py keeps the survivor of a collapse where it was: its output vertices are input vertices, and on a coarse mesh of a curved
surface those all lie on one side of the best-fitting faces.  This module is Garland and Heckbert's pair contraction on the same rounds:
where both ends of an edge are FREE the survivor moves to the minimum of the summed quadrics of the two ends, regularised towards the
midpoint (regularization, simplify_mesh's lambda) and kept within reach times the edge's largest axis extent of it; the position is rounded
to fp32 first, and the cost and the guards -- over the rings of BOTH ends -- are taken at the rounded position.  Where one end is held the
edge is mesh_decimate.py's half-edge collapse onto it, word for word.  Same vertex classes, same budget per round, same ranking and
independent set; the quadrics follow into the survivor's new frame, so quadrics="carried" still measures against the ORIGINAL surface.
vertex_blend says how far each placed survivor went towards the vertex it replaced, and attributes are blended by it.  The result is a
pure function of the input (include/ts_contract.h), bit-equal to a numpy reference (tests/ref_mesh_contract.py).

Native code: libts_contract.so beside this file (include/ts_contract.h, csrc/mesh_contract.hip), a twentieth library because the export
lists of the other nineteen are closed; bound with ctypes.  The initial quadrics are mesh_decimate.vertex_quadrics'.  No CPU / eager
fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, NamedTuple, Optional

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_contract

from .mesh_decimate import _budget_arg, _participating, _quadrics_arg, _quadrics_of, _rule_args, _stats
from .mesh_weld import _device_of, _faces_arg, _keep_arg, _vertices_arg

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_contract.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The contraction kernels have no CPU fallback."
    )
_lib = bind_contract(C.CDLL(_LIB_PATH))

CONTRACT_STATES = {"no_edge": 0, "not_eligible": 1, "too_costly": 2, "guarded": 3, "lost": 4, "collapsed": 5, "deferred": 6}  # TSU_*
CONTRACT_GUARDS = {"link": 1, "long": 2, "normal": 4, "held": 8}                                                             # TSU_GUARD_*
MAX_RING = 64                                                                                                                # TSU_MAX_RING
TOTAL_NAMES = ("edges", "candidates", "in_budget", "collapsed", "too_costly")  # tsu_contract's five words


class ContractedRound(NamedTuple):
    vertices: Optional[torch.Tensor]       # (V, 3) float32: the input's rows, the placed survivors moved; None from placed_edges
    faces: Optional[torch.Tensor]          # (F, 3) int32: the input's faces, r replaced by k around every winner; None from placed_edges
    face_keep: Optional[torch.Tensor]      # (F,) bool: False on the deleted faces (and where `keep` was); None from placed_edges
    vertex_target: Optional[torch.Tensor]  # (V,) int32: k for a removed r, v otherwise; None from placed_edges
    quadrics: Optional[torch.Tensor]       # (V, 10) float64: the input's rows, the winners' survivors merged in their new frames; None from placed_edges
    vertex_blend: Optional[torch.Tensor]   # (V,) float64 in [0, 1]: how far a placed survivor went towards its r; 0 elsewhere; None from placed_edges
    edge_vertices: torch.Tensor            # (E, 2) int32: (lo, hi), ascending -- the edges of the INPUT
    edge_state: torch.Tensor               # (E,) uint8: CONTRACT_STATES
    edge_removed: torch.Tensor             # (E,) int32: r of a candidate, -1 otherwise
    edge_guard: torch.Tensor               # (E,) uint8: CONTRACT_GUARDS of an eligible edge
    edge_cost: torch.Tensor                # (E,) float64: the cost of a candidate or a too costly edge, inf otherwise
    edge_position: torch.Tensor            # (E, 3) float32: where the survivor of a candidate goes, nan otherwise
    stats: Dict[str, object]               # TOTAL_NAMES, "deferred", "guarded", "max_cost_collapsed" (nan if nothing collapsed)


class ContractedMesh(NamedTuple):
    vertices: torch.Tensor               # (V', 3) float32: the surviving rows, the placed ones moved (all rows without compact)
    faces: torch.Tensor                  # (F', 3) int32
    face_keep: Optional[torch.Tensor]    # (F,) bool without compact; None with it (every returned face is kept)
    vertex_map: torch.Tensor             # (V,) int32: old -> new; the survivor's index for a removed vertex
    face_map: torch.Tensor               # (F',) int32: new -> old slot
    attributes: Optional[torch.Tensor]   # (V', ...) float32: the survivors' rows, blended where they moved, or None
    attribute_valid: Optional[torch.Tensor]  # (V',) bool, or None without attribute_valid
    quadrics: torch.Tensor               # (V', 10) float64: the quadrics of the survivors; a later call continues from them
    reached: bool                        # the participating faces are at most target_faces
    stats: Dict[str, object]             # rounds, collapsed, target_faces, participating_faces, reached, num_vertices, num_faces, per_round


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsu_last_error().decode()} (ts2d error {rc})")


def _placement_args(regularization, reach):
    lam, span = float(regularization), float(reach)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError("regularization must be finite and >= 0")
    if not (math.isfinite(span) and span >= 0.0):
        raise ValueError("reach must be finite and >= 0")
    return lam, span


def _workspace(V: int, F: int, device):
    return torch.empty((_lib.tsu_workspace_bytes(V, F),), device=device, dtype=torch.uint8) if F else None


def _contract_arrays(v, f, k, q, rule, placement, budget: int, seed: int, classify_only: bool, device):
    """(out_faces (F, 3), out_keep (F,) uint8, vertex_target (V,), out_vertices (V, 3), out_quadrics (V, 10) and vertex_blend (V,), or None
    six times; edge_vertices (3 F, 2); edge_state (3 F,) uint8; edge_removed (3 F,); edge_guard (3 F,) uint8; edge_cost (3 F,) float64;
    edge_position (3 F, 3); totals (5,) int64) as tsu_contract writes them, to their capacity.  Nothing is read back."""
    max_cost, max_edge, min_cos, pinned = rule
    lam, span = placement
    V, F = v.shape[0], f.shape[0]
    with torch.cuda.device(device):
        out_faces = None if classify_only else torch.empty((F, 3), device=device, dtype=torch.int32)
        out_keep = None if classify_only else torch.empty((F,), device=device, dtype=torch.uint8)
        target = None if classify_only else torch.empty((V,), device=device, dtype=torch.int32)
        out_v = None if classify_only else torch.empty((V, 3), device=device, dtype=torch.float32)
        out_q = None if classify_only else torch.empty((V, 10), device=device, dtype=torch.float64)
        blend = None if classify_only else torch.empty((V,), device=device, dtype=torch.float64)
        ev = torch.empty((3 * F, 2), device=device, dtype=torch.int32)
        state = torch.empty((3 * F,), device=device, dtype=torch.uint8)
        removed = torch.empty((3 * F,), device=device, dtype=torch.int32)
        guard = torch.empty((3 * F,), device=device, dtype=torch.uint8)
        cost = torch.empty((3 * F,), device=device, dtype=torch.float64)
        position = torch.empty((3 * F, 3), device=device, dtype=torch.float32)
        totals = torch.empty((5,), device=device, dtype=torch.int64)
        ws = _workspace(V, F, device)
        # an empty tensor still gets an (aligned) address where the call asks for "given": the six face outputs decide the mode
        ptr = (lambda t: t.data_ptr() if t is not None and t.numel() else None)
        given = (lambda t: None if t is None else (t.data_ptr() or 8))
        _check(_lib.tsu_contract(V, F, ptr(v), ptr(f), _native._ptr(k), _native._ptr(pinned), ptr(q), max_cost, budget, max_edge, min_cos, lam,
                                 span, int(seed) & 0xFFFFFFFF, given(out_faces), given(out_keep), given(target), given(out_v), given(out_q),
                                 given(blend), ptr(ev), ptr(state), ptr(removed), ptr(guard), ptr(cost), ptr(position), totals.data_ptr(),
                                 _native._ptr(ws), ws.numel() if ws is not None else 0, _native.stream()), "contract_round")
    return out_faces, out_keep, target, out_v, out_q, blend, ev, state, removed, guard, cost, position, totals


def _args(what, vertices, faces, keep, quadrics, max_cost, max_edge, max_normal_deg, pinned):
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    rule = _rule_args(v.shape[0], max_cost, max_edge, max_normal_deg, pinned)
    q = _quadrics_arg(quadrics, v.shape[0]) if quadrics is not None else None
    return v, f, k, q, rule, _device_of(what, v, f, k, q, rule[3])


def _one_round(what, vertices, faces, quadrics, max_collapses, keep, max_cost, max_edge, max_normal_deg, pinned, regularization, reach, seed,
               classify_only):
    budget = _budget_arg(max_collapses)
    placement = _placement_args(regularization, reach)
    v, f, k, q, rule, device = _args(what, vertices, faces, keep, quadrics, max_cost, max_edge, max_normal_deg, pinned)
    out_faces, out_keep, target, out_v, out_q, blend, ev, state, removed, guard, cost, position, totals = _contract_arrays(
        v, f, k, q, rule, placement, budget, seed, classify_only, device)
    t = _stats(totals, state, cost)
    E = t["edges"]
    return ContractedRound(out_v, out_faces, out_keep != 0 if out_keep is not None else None, target, out_q, blend, ev[:E], state[:E], removed[:E],
                           guard[:E], cost[:E], position[:E], t)


def contract_round(vertices: torch.Tensor, faces: torch.Tensor, quadrics: torch.Tensor, max_collapses: int, keep: Optional[torch.Tensor] = None,
                   max_cost: float = math.inf, max_edge: float = math.inf, max_normal_deg: float = 30.0, pinned: Optional[torch.Tensor] = None,
                   regularization: float = 1e-3, reach: float = 1.0, seed: int = 0) -> ContractedRound:
    """One round (module text).  quadrics (V, 10) float64: vertex_quadrics' or an earlier round's; max_collapses, max_cost, max_edge,
    max_normal_deg, pinned, seed, keep: decimate_round's; regularization: the pull towards the midpoint as a share of the quadric's trace
    (simplify_mesh's); reach: how far from the midpoint a survivor may go per axis, in units of the edge's largest axis extent (0: the
    midpoint).  The edge table is the input's, trimmed to its E edges.  One host read (the totals)."""
    return _one_round("contract_round", vertices, faces, quadrics, max_collapses, keep, max_cost, max_edge, max_normal_deg, pinned, regularization,
                      reach, seed, False)


def placed_edges(vertices: torch.Tensor, faces: torch.Tensor, quadrics: torch.Tensor, max_collapses: int, keep: Optional[torch.Tensor] = None,
                 max_cost: float = math.inf, max_edge: float = math.inf, max_normal_deg: float = 30.0, pinned: Optional[torch.Tensor] = None,
                 regularization: float = 1e-3, reach: float = 1.0, seed: int = 0) -> ContractedRound:
    """The classification of contract_round without the contraction: the six face- and vertex-side entries are None; edge_state, edge_cost
    and edge_position say what the round would do (the selection included) and where every candidate's survivor would go."""
    return _one_round("placed_edges", vertices, faces, quadrics, max_collapses, keep, max_cost, max_edge, max_normal_deg, pinned, regularization,
                      reach, seed, True)


def _blend_attributes(attrs, valid, round_target, blend):
    """(attributes, valid) after one round: the row of a survivor that moved towards its r (vertex_blend > 0) becomes
    (1 - t) attr_k + t attr_r in float64 rounded to the attributes' type -- where both rows are valid; the valid row's where one is; k's
    own, still invalid, where neither is.  Every other row stays.  No host read: the r of every k comes from one scatter."""
    V = round_target.shape[0]
    ids = torch.arange(V, device=round_target.device, dtype=torch.int64)
    target = round_target.to(torch.int64)
    r_of = torch.full((V,), -1, device=target.device, dtype=torch.int64)
    r_of.scatter_reduce_(0, target, torch.where(target != ids, ids, torch.full_like(ids, -1)), "amax")  # at most one r per k in a round
    moved = (r_of >= 0) & (blend > 0)
    r = r_of.clamp(min=0)
    shape = (V,) + (1,) * (attrs.dim() - 1)
    t = blend.reshape(shape)
    mixed = ((1.0 - t) * attrs.to(torch.float64) + t * attrs[r].to(torch.float64)).to(attrs.dtype)
    if valid is None:
        return torch.where(moved.reshape(shape), mixed, attrs), None
    both, only_r = moved & valid & valid[r], moved & ~valid & valid[r]
    out = torch.where(both.reshape(shape), mixed, torch.where(only_r.reshape(shape), attrs[r], attrs))
    return out, valid | only_r


def contract_mesh(vertices: torch.Tensor, faces: torch.Tensor, target_faces: Optional[int] = None, ratio: Optional[float] = None,
                  max_cost: float = math.inf, keep: Optional[torch.Tensor] = None, max_edge: float = math.inf, max_normal_deg: float = 30.0,
                  pinned: Optional[torch.Tensor] = None, quadrics="carried", regularization: float = 1e-3, reach: float = 1.0,
                  max_rounds: int = 256, compact: bool = True, attributes: Optional[torch.Tensor] = None,
                  attribute_valid: Optional[torch.Tensor] = None) -> ContractedMesh:
    """Rounds of contract_round with seed = round index until the faces that take part are at most target_faces (or ratio times their
    number at the start, rounded down), a round contracts nothing, or max_rounds: decimate_mesh's stop rules, budget
    ceil((participating faces - target) / 2) and quadric modes ("memoryless" recomputes the quadrics from the MOVED vertices).  Returns the
    moved vertices.  attributes (V, ...) floating point: blended round by round as (1 - t) attr_k + t attr_r with t = vertex_blend, in
    float64 rounded back, by attribute_valid (V,) bool as split_edges does; a held survivor keeps its row.  One host read per round and
    one for the participating faces."""
    if int(max_rounds) < 1:
        raise ValueError("max_rounds must be >= 1")
    if target_faces is not None and ratio is not None:
        raise ValueError("give target_faces or ratio (one of them)")
    if target_faces is None and ratio is None:
        if not math.isfinite(float(max_cost)):
            raise ValueError("give target_faces or ratio, or a finite max_cost")
        target_faces = 0
    if ratio is not None and not 0.0 <= float(ratio) <= 1.0:
        raise ValueError("ratio must lie in [0, 1]")
    if target_faces is not None and int(target_faces) < 0:
        raise ValueError("target_faces must be >= 0")
    mode = quadrics if isinstance(quadrics, str) else "given"
    if mode not in ("carried", "memoryless", "given"):
        raise ValueError('quadrics must be "carried", "memoryless" or a (num_vertices, 10) float64 tensor')
    placement = _placement_args(regularization, reach)
    v, f, k, q, rule, device = _args("contract_mesh", vertices, faces, keep, quadrics if mode == "given" else None, max_cost, max_edge,
                                     max_normal_deg, pinned)
    V, F = v.shape[0], f.shape[0]
    if attributes is not None and (attributes.dim() < 1 or attributes.shape[0] != V or not attributes.is_floating_point()):
        raise RuntimeError("attributes must be a floating-point tensor with num_vertices rows")
    if attribute_valid is not None and (attributes is None or attribute_valid.shape != (V,) or attribute_valid.dtype != torch.bool):
        raise RuntimeError("attribute_valid must be a bool tensor with dimensions (num_vertices,) beside attributes")
    attrs, valid = attributes, attribute_valid
    with torch.cuda.device(device):
        target = torch.arange(V, device=device, dtype=torch.int64)
        face_keep = k != 0 if k is not None else torch.ones((F,), device=device, dtype=torch.bool)
        count = int(_participating(v, f, k).sum())
    start_count = count
    goal = int(target_faces) if target_faces is not None else int(math.floor(float(ratio) * count))
    if q is None:
        q = _quadrics_of(v, f, k, device)
    per_round = []
    for r in range(int(max_rounds)):
        if count <= goal:
            break
        if mode == "memoryless" and r > 0:
            q = _quadrics_of(v, f, k, device)
        out_faces, out_keep, round_target, out_v, out_q, blend, _, state, _, _, cost, _, totals = _contract_arrays(
            v, f, k, q, rule, placement, _budget_arg((count - goal + 1) // 2), r, False, device)
        t = _stats(totals, state, cost)
        if t["collapsed"] == 0:  # the round copied its input
            break
        per_round.append(t)
        if attrs is not None:
            with torch.cuda.device(device):
                attrs, valid = _blend_attributes(attrs, valid, round_target, blend)
        v, f, k, q = out_v, out_faces, out_keep, out_q
        face_keep = out_keep != 0
        target = round_target.to(torch.int64)[target]
        count -= 2 * t["collapsed"]
    reached = count <= goal
    stats = {"rounds": len(per_round), "collapsed": sum(t["collapsed"] for t in per_round), "target_faces": goal, "participating_faces": count,
             "participating_faces_before": start_count, "reached": reached, "quadrics": mode, "regularization": placement[0], "reach": placement[1],
             "per_round": per_round}
    with torch.cuda.device(device):
        if not compact:
            stats.update(num_vertices=V, num_faces=F)
            return ContractedMesh(v, f, face_keep, target.to(torch.int32), torch.arange(F, device=device, dtype=torch.int32), attrs, valid, q,
                                  reached, stats)
        survives = target == torch.arange(V, device=device, dtype=torch.int64)
        new_index = torch.cumsum(survives, 0) - 1
        vertex_map = new_index[target]
        face_map = torch.nonzero(face_keep).reshape(-1)
        old = f[face_map].to(torch.int64)
        named = (old >= 0) & (old < V)  # a face that does not take part keeps an index that names no vertex as it is: it still names none
        new_faces = torch.where(named, vertex_map[old.clamp(0, max(V - 1, 0))] if V else old, old).to(torch.int32)
        kept_rows = torch.nonzero(survives).reshape(-1)
        stats.update(num_vertices=int(kept_rows.shape[0]), num_faces=int(face_map.shape[0]))
        return ContractedMesh(v[kept_rows], new_faces, None, vertex_map.to(torch.int32), face_map.to(torch.int32),
                              attrs[kept_rows] if attrs is not None else None, valid[kept_rows] if valid is not None else None, q[kept_rows],
                              reached, stats)


def contract_fused(mesh, target_faces: Optional[int] = None, ratio: Optional[float] = None, max_cost: float = math.inf,
                   max_edge: float = math.inf, max_normal_deg: float = 30.0, max_rounds: int = 256, pinned: Optional[torch.Tensor] = None,
                   quadrics="carried", regularization: float = 1e-3, reach: float = 1.0):
    """The pass behind a weld, a fusion, a remesh, a split or a flip: `mesh` is a WeldedMesh, a ColoredMesh or anything else with
    vertices, faces, stats and _replace; contract_mesh on it, compacted.  Returns the same kind of mesh with the moved vertices: a
    ColoredMesh has the colours of its placed survivors blended by vertex_blend and color_valid (an invalid survivor that moved towards a
    valid vertex takes its colour); a WeldedMesh has its face colours follow face_map and its vertex_map composed with the contraction's.
    stats keeps the mesh's entries, updates num_vertices / num_faces and gains contract_mesh's under "contract" with vertex_map, face_map
    and the survivors' quadrics beside them.  A welded soup has only boundary edges: every vertex is held, nothing collapses, and
    stats["contract"]["reached"] says so."""
    coloured = hasattr(mesh, "vertex_color")
    V = mesh.vertices.shape[0]
    r = contract_mesh(mesh.vertices, mesh.faces, target_faces=target_faces, ratio=ratio, max_cost=max_cost, max_edge=max_edge,
                      max_normal_deg=max_normal_deg, pinned=pinned, quadrics=quadrics, regularization=regularization, reach=reach,
                      max_rounds=max_rounds, attributes=mesh.vertex_color if coloured else None,
                      attribute_valid=mesh.color_valid if coloured else None)
    stats = dict(mesh.stats)
    stats["contract"] = dict(r.stats, vertex_map=r.vertex_map, face_map=r.face_map, quadrics_after=r.quadrics)
    stats.update(num_vertices=int(r.vertices.shape[0]), num_faces=int(r.faces.shape[0]))
    if coloured:
        return mesh._replace(vertices=r.vertices, faces=r.faces, vertex_color=r.attributes.contiguous(), color_valid=r.attribute_valid, stats=stats)
    if not hasattr(mesh, "vertex_map"):
        return mesh._replace(vertices=r.vertices, faces=r.faces, stats=stats)
    at = r.face_map.to(torch.int64)
    old = mesh.vertex_map.to(torch.int64)
    composed = torch.where((old >= 0) & (old < V), r.vertex_map[old.clamp(0, max(V - 1, 0))] if V else mesh.vertex_map, mesh.vertex_map)
    return mesh._replace(vertices=r.vertices, faces=r.faces, faces_color=mesh.faces_color[at] if mesh.faces_color is not None else None,
                         vertex_map=composed.to(mesh.vertex_map.dtype), stats=stats)


__all__ = ["CONTRACT_STATES", "CONTRACT_GUARDS", "TOTAL_NAMES", "MAX_RING", "ContractedRound", "ContractedMesh", "contract_round", "placed_edges",
           "contract_mesh", "contract_fused"]
