"""Decimating an indexed mesh to a face budget or an error bound, on the device: rounds of half-edge collapses ordered by quadric error.

    vertex_quadrics(vertices, faces, keep=None) -> (V, 10) float64                              the initial quadrics of a mesh
    decimate_round(vertices, faces, quadrics, max_collapses, keep=None, max_cost=inf, max_edge=inf, max_normal_deg=30.0, pinned=None,
                   seed=0) -> DecimatedRound                                                     one round
    cheapest_edges(...)                                                                          the classification of a round alone
    decimate_mesh(vertices, faces, target_faces=None, ratio=None, max_cost=inf, ..., quadrics="carried" | "memoryless" | tensor,
                  max_rounds=256, compact=True, attributes=None) -> DecimatedMesh                rounds until the budget is met
    decimate_fused(mesh, ...)                                                                    the pass behind a weld, a fusion, a remesh, a split or a flip

simplify_mesh merges whatever falls into one grid cell, connected or not, and its face count is an accident of the cell size;
collapse_short_edges orders its collapses by length and stops at a length.  This module answers "this surface in N faces": the collapses are
mesh_collapse.py's -- r -> k along an edge, no vertex moves, V - 1, E - 3, F - 2 each, same vertex classes, same link / long / normal guards,
same independent set at distance two -- but they are ordered by the quadric error of Garland and Heckbert: the sum of squared,
area-squared-weighted distances of the surviving vertex to the planes of the faces the removed vertex stood for.  Each round ranks its
candidates by (cost, priority, edge) and lets only the first max_collapses of them compete, so a round never overshoots the budget; the
quadrics follow the collapses (a survivor's quadric gains the removed vertex's, translated into its frame), so with quadrics="carried" the
error is always measured against the ORIGINAL surface.  The result is a pure function of the input (include/ts_decimate.h),
bit-equal to a numpy reference (tests/ref_mesh_decimate.py).

Native code: libts_decimate.so beside this file (include/ts_decimate.h, csrc/mesh_decimate.hip), a nineteenth library because the export
lists of the other eighteen are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, NamedTuple, Optional

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_decimate

from .mesh_weld import _device_of, _faces_arg, _keep_arg, _vertices_arg

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_decimate.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The decimation kernels have no CPU fallback."
    )
_lib = bind_decimate(C.CDLL(_LIB_PATH))

DECIMATE_STATES = {"no_edge": 0, "not_eligible": 1, "too_costly": 2, "guarded": 3, "lost": 4, "collapsed": 5, "deferred": 6}  # TSZ_*
DECIMATE_GUARDS = {"link": 1, "long": 2, "normal": 4, "held": 8}                                                             # TSZ_GUARD_*
MAX_RING = 64                                                                                                                # TSZ_MAX_RING
TOTAL_NAMES = ("edges", "candidates", "in_budget", "collapsed", "too_costly")  # tsz_decimate's five words
MAX_BUDGET = 2 ** 31 - 1


class DecimatedRound(NamedTuple):
    faces: Optional[torch.Tensor]          # (F, 3) int32: the input's faces, r replaced by k around every winner; None from cheapest_edges
    face_keep: Optional[torch.Tensor]      # (F,) bool: False on the deleted faces (and where `keep` was); None from cheapest_edges
    vertex_target: Optional[torch.Tensor]  # (V,) int32: k for a removed r, v otherwise; None from cheapest_edges
    quadrics: Optional[torch.Tensor]       # (V, 10) float64: the input's rows, the winners' survivors merged; None from cheapest_edges
    edge_vertices: torch.Tensor            # (E, 2) int32: (lo, hi), ascending -- the edges of the INPUT
    edge_state: torch.Tensor               # (E,) uint8: DECIMATE_STATES
    edge_removed: torch.Tensor             # (E,) int32: r of a candidate, -1 otherwise
    edge_guard: torch.Tensor               # (E,) uint8: DECIMATE_GUARDS over the directions of an eligible edge
    edge_cost: torch.Tensor                # (E,) float64: the cost of a candidate or a too costly edge, inf otherwise
    stats: Dict[str, object]               # TOTAL_NAMES, "deferred", "guarded", "max_cost_collapsed" (nan if nothing collapsed)


class DecimatedMesh(NamedTuple):
    vertices: torch.Tensor               # (V', 3) float32: the input's rows that survive (all of them without compact)
    faces: torch.Tensor                  # (F', 3) int32
    face_keep: Optional[torch.Tensor]    # (F,) bool without compact; None with it (every returned face is kept)
    vertex_map: torch.Tensor             # (V,) int32: old -> new; the survivor's index for a removed vertex
    face_map: torch.Tensor               # (F',) int32: new -> old slot
    attributes: Optional[torch.Tensor]   # (V', ...) the input's rows of the surviving vertices, or None
    quadrics: torch.Tensor               # (V', 10) float64: the quadrics of the survivors; a later call continues from them
    reached: bool                        # the participating faces are at most target_faces
    stats: Dict[str, object]             # rounds, collapsed, target_faces, participating_faces, reached, num_vertices, num_faces, per_round


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsz_last_error().decode()} (ts2d error {rc})")


def _min_cos_of(max_normal_deg: float) -> float:
    """cos(max_normal_deg) formed once in float64, rounded to fp32 and clamped to [0, 1] (mesh_collapse.min_cos_of)."""
    deg = float(max_normal_deg)
    if not 0.0 <= deg <= 90.0:
        raise ValueError("max_normal_deg must lie in [0, 90]")
    return min(1.0, max(0.0, C.c_float(math.cos(math.radians(deg))).value))


def _quadrics_arg(quadrics: torch.Tensor, V: int) -> torch.Tensor:
    if quadrics.shape != (V, 10) or quadrics.dtype != torch.float64:
        raise RuntimeError("quadrics must be a float64 tensor with dimensions (num_vertices, 10)")
    return quadrics.detach().contiguous()


def _rule_args(V: int, max_cost, max_edge, max_normal_deg, pinned):
    """(max_cost, max_edge, min_cos, pinned (V,) uint8 / bool or None)."""
    max_cost, max_edge = float(max_cost), float(max_edge)
    if not max_cost >= 0.0:
        raise ValueError("max_cost must be >= 0 (inf: no bound)")
    if not max_edge > 0.0:
        raise ValueError("max_edge must be > 0 (inf: no bound)")
    if pinned is not None:
        if pinned.shape != (V,) or pinned.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError("pinned must be a bool or uint8 tensor with dimensions (num_vertices,)")
        pinned = pinned.contiguous()
    return max_cost, max_edge, _min_cos_of(max_normal_deg), pinned


def _budget_arg(max_collapses) -> int:
    n = int(max_collapses)
    if n < 0:
        raise ValueError("max_collapses must be >= 0")
    return min(n, MAX_BUDGET)


def _workspace(V: int, F: int, device):
    return torch.empty((_lib.tsz_workspace_bytes(V, F),), device=device, dtype=torch.uint8) if F else None


def _quadrics_of(v: torch.Tensor, f: torch.Tensor, k: Optional[torch.Tensor], device) -> torch.Tensor:
    V, F = v.shape[0], f.shape[0]
    with torch.cuda.device(device):
        out = torch.empty((V, 10), device=device, dtype=torch.float64)
        ws = _workspace(V, F, device)
        ptr = (lambda t: t.data_ptr() if t is not None and t.numel() else None)
        _check(_lib.tsz_vertex_quadrics(V, F, ptr(v), ptr(f), _native._ptr(k), ptr(out), _native._ptr(ws), ws.numel() if ws is not None else 0,
                                        _native.stream()), "vertex_quadrics")
    return out


def _decimate_arrays(v, f, k, q, rule, budget: int, seed: int, classify_only: bool, device):
    """(out_faces (F, 3), out_keep (F,) uint8, vertex_target (V,) and out_quadrics (V, 10), or None four times; edge_vertices (3 F, 2);
    edge_state (3 F,) uint8; edge_removed (3 F,); edge_guard (3 F,) uint8; edge_cost (3 F,) float64; totals (5,) int64) as tsz_decimate
    writes them, to their capacity.  Nothing is read back."""
    max_cost, max_edge, min_cos, pinned = rule
    V, F = v.shape[0], f.shape[0]
    with torch.cuda.device(device):
        out_faces = None if classify_only else torch.empty((F, 3), device=device, dtype=torch.int32)
        out_keep = None if classify_only else torch.empty((F,), device=device, dtype=torch.uint8)
        target = None if classify_only else torch.empty((V,), device=device, dtype=torch.int32)
        out_q = None if classify_only else torch.empty((V, 10), device=device, dtype=torch.float64)
        ev = torch.empty((3 * F, 2), device=device, dtype=torch.int32)
        state = torch.empty((3 * F,), device=device, dtype=torch.uint8)
        removed = torch.empty((3 * F,), device=device, dtype=torch.int32)
        guard = torch.empty((3 * F,), device=device, dtype=torch.uint8)
        cost = torch.empty((3 * F,), device=device, dtype=torch.float64)
        totals = torch.empty((5,), device=device, dtype=torch.int64)
        ws = _workspace(V, F, device)
        # an empty tensor still gets an (aligned) address where the call asks for "given": the four face outputs decide the mode
        ptr = (lambda t: t.data_ptr() if t is not None and t.numel() else None)
        given = (lambda t: None if t is None else (t.data_ptr() or 8))
        _check(_lib.tsz_decimate(V, F, ptr(v), ptr(f), _native._ptr(k), _native._ptr(pinned), ptr(q), max_cost, budget, max_edge, min_cos,
                                 int(seed) & 0xFFFFFFFF, given(out_faces), given(out_keep), given(target), given(out_q), ptr(ev), ptr(state),
                                 ptr(removed), ptr(guard), ptr(cost), totals.data_ptr(), _native._ptr(ws), ws.numel() if ws is not None else 0,
                                 _native.stream()), "decimate_round")
    return out_faces, out_keep, target, out_q, ev, state, removed, guard, cost, totals


def _stats(totals: torch.Tensor, state: torch.Tensor, cost: torch.Tensor) -> Dict[str, object]:
    won = state == DECIMATE_STATES["collapsed"]
    largest = torch.where(won, cost, torch.full_like(cost, -1.0)).max() if cost.numel() else cost.new_tensor(-1.0)
    guarded = (state == DECIMATE_STATES["guarded"]).sum()
    numbers = torch.cat([totals.to(torch.float64), guarded.to(torch.float64)[None], largest[None]]).tolist()  # the one host read of a round
    t: Dict[str, object] = {name: int(n) for name, n in zip(TOTAL_NAMES, numbers[:5])}
    t["deferred"] = t["candidates"] - t["in_budget"]
    t["guarded"] = int(numbers[5])
    t["max_cost_collapsed"] = float(numbers[6]) if t["collapsed"] else float("nan")
    return t


def _args(what, vertices, faces, keep, quadrics, max_cost, max_edge, max_normal_deg, pinned):
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    rule = _rule_args(v.shape[0], max_cost, max_edge, max_normal_deg, pinned)
    q = _quadrics_arg(quadrics, v.shape[0]) if quadrics is not None else None
    return v, f, k, q, rule, _device_of(what, v, f, k, q, rule[3])


def vertex_quadrics(vertices: torch.Tensor, faces: torch.Tensor, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(V, 10) float64, a00 a01 a02 a11 a12 a22 b0 b1 b2 c per vertex in the vertex's own frame: the sum over its ring faces (in ascending
    corner index, finite ones only) of the outer product of the unnormalised normal; b = c = 0.  Nothing is read back."""
    v, f = _vertices_arg(vertices), _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    return _quadrics_of(v, f, k, _device_of("vertex_quadrics", v, f, k))


def _one_round(what, vertices, faces, quadrics, max_collapses, keep, max_cost, max_edge, max_normal_deg, pinned, seed, classify_only):
    budget = _budget_arg(max_collapses)
    v, f, k, q, rule, device = _args(what, vertices, faces, keep, quadrics, max_cost, max_edge, max_normal_deg, pinned)
    out_faces, out_keep, target, out_q, ev, state, removed, guard, cost, totals = _decimate_arrays(v, f, k, q, rule, budget, seed, classify_only, device)
    t = _stats(totals, state, cost)
    E = t["edges"]
    return DecimatedRound(out_faces, out_keep != 0 if out_keep is not None else None, target, out_q, ev[:E], state[:E], removed[:E], guard[:E],
                          cost[:E], t)


def decimate_round(vertices: torch.Tensor, faces: torch.Tensor, quadrics: torch.Tensor, max_collapses: int, keep: Optional[torch.Tensor] = None,
                   max_cost: float = math.inf, max_edge: float = math.inf, max_normal_deg: float = 30.0, pinned: Optional[torch.Tensor] = None,
                   seed: int = 0) -> DecimatedRound:
    """One round (module text).  quadrics (V, 10) float64: vertex_quadrics' or an earlier round's; max_collapses: the budget of the round --
    only the first max_collapses candidates in (cost, priority, edge) order compete, the others are deferred; max_cost: no collapse costs
    more; max_edge, max_normal_deg, pinned, seed, keep: collapse_edges'.  The edge table is the input's, trimmed to its E edges.  One host
    read (the totals)."""
    return _one_round("decimate_round", vertices, faces, quadrics, max_collapses, keep, max_cost, max_edge, max_normal_deg, pinned, seed, False)


def cheapest_edges(vertices: torch.Tensor, faces: torch.Tensor, quadrics: torch.Tensor, max_collapses: int, keep: Optional[torch.Tensor] = None,
                   max_cost: float = math.inf, max_edge: float = math.inf, max_normal_deg: float = 30.0, pinned: Optional[torch.Tensor] = None,
                   seed: int = 0) -> DecimatedRound:
    """The classification of decimate_round without the collapse: faces, face_keep, vertex_target and quadrics are None, edge_state and
    edge_cost say what the round would do (the selection included)."""
    return _one_round("cheapest_edges", vertices, faces, quadrics, max_collapses, keep, max_cost, max_edge, max_normal_deg, pinned, seed, True)


def _participating(v: torch.Tensor, f: torch.Tensor, k: Optional[torch.Tensor]) -> torch.Tensor:
    """(F,) bool: kept, the three indices in [0, V) and pairwise distinct."""
    ok = ((f >= 0) & (f < v.shape[0])).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    return ok & (k != 0) if k is not None else ok


def decimate_mesh(vertices: torch.Tensor, faces: torch.Tensor, target_faces: Optional[int] = None, ratio: Optional[float] = None,
                  max_cost: float = math.inf, keep: Optional[torch.Tensor] = None, max_edge: float = math.inf, max_normal_deg: float = 30.0,
                  pinned: Optional[torch.Tensor] = None, quadrics="carried", max_rounds: int = 256, compact: bool = True,
                  attributes: Optional[torch.Tensor] = None) -> DecimatedMesh:
    """Rounds of decimate_round with seed = round index until the faces that take part are at most target_faces (or ratio times their
    number at the start, rounded down), a round collapses nothing, or max_rounds.  Exactly one of target_faces / ratio, unless max_cost is
    finite: then target_faces defaults to 0, error-bounded decimation.  Each round's budget is ceil((participating faces - target) / 2), so
    the result never has fewer than target_faces - 1 faces (a collapse removes two).  quadrics: "carried" computes vertex_quadrics once and
    carries every round's output quadrics into the next, so the error is measured against the original surface; "memoryless" recomputes them
    from the current faces every round; a (V, 10) float64 tensor continues from an earlier call's.  compact, attributes, vertex_map and
    face_map: collapse_short_edges'.  One host read per round and one for the participating faces."""
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
    v, f, k, q, rule, device = _args("decimate_mesh", vertices, faces, keep, quadrics if mode == "given" else None, max_cost, max_edge,
                                     max_normal_deg, pinned)
    V, F = v.shape[0], f.shape[0]
    if attributes is not None and (attributes.dim() < 1 or attributes.shape[0] != V):
        raise RuntimeError("attributes must have num_vertices rows")
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
        out_faces, out_keep, round_target, out_q, _, state, _, _, cost, totals = _decimate_arrays(v, f, k, q, rule, _budget_arg((count - goal + 1) // 2),
                                                                                                  r, False, device)
        t = _stats(totals, state, cost)
        if t["collapsed"] == 0:  # the round copied its input
            break
        per_round.append(t)
        f, k, q = out_faces, out_keep, out_q
        face_keep = out_keep != 0
        target = round_target.to(torch.int64)[target]
        count -= 2 * t["collapsed"]
    reached = count <= goal
    stats = {"rounds": len(per_round), "collapsed": sum(t["collapsed"] for t in per_round), "target_faces": goal, "participating_faces": count,
             "participating_faces_before": start_count, "reached": reached, "quadrics": mode, "per_round": per_round}
    with torch.cuda.device(device):
        if not compact:
            stats.update(num_vertices=V, num_faces=F)
            return DecimatedMesh(v, f, face_keep, target.to(torch.int32), torch.arange(F, device=device, dtype=torch.int32), attributes, q, reached,
                                 stats)
        survives = target == torch.arange(V, device=device, dtype=torch.int64)
        new_index = torch.cumsum(survives, 0) - 1
        vertex_map = new_index[target]
        face_map = torch.nonzero(face_keep).reshape(-1)
        old = f[face_map].to(torch.int64)
        named = (old >= 0) & (old < V)  # a face that does not take part keeps an index that names no vertex as it is: it still names none
        new_faces = torch.where(named, vertex_map[old.clamp(0, max(V - 1, 0))] if V else old, old).to(torch.int32)
        kept_rows = torch.nonzero(survives).reshape(-1)
        stats.update(num_vertices=int(kept_rows.shape[0]), num_faces=int(face_map.shape[0]))
        return DecimatedMesh(v[kept_rows], new_faces, None, vertex_map.to(torch.int32), face_map.to(torch.int32),
                             attributes[kept_rows] if attributes is not None else None, q[kept_rows], reached, stats)


def decimate_fused(mesh, target_faces: Optional[int] = None, ratio: Optional[float] = None, max_cost: float = math.inf,
                   max_edge: float = math.inf, max_normal_deg: float = 30.0, max_rounds: int = 256, pinned: Optional[torch.Tensor] = None,
                   quadrics="carried"):
    """The pass behind a weld, a fusion, a remesh, a split or a flip: `mesh` is a WeldedMesh, a ColoredMesh or anything else with
    vertices, faces, stats and _replace; decimate_mesh on it, compacted.  Returns the same kind of mesh: a ColoredMesh keeps the colour and
    the validity of its surviving vertices (no vertex moves, nothing is interpolated); a WeldedMesh has its face colours follow face_map and
    its vertex_map composed with the decimation's.  stats keeps the mesh's entries, updates num_vertices / num_faces and gains
    decimate_mesh's under "decimate" with vertex_map, face_map and the survivors' quadrics beside them.  A welded soup has only boundary
    edges: every vertex is held, nothing collapses, and stats["decimate"]["reached"] says so."""
    coloured = hasattr(mesh, "vertex_color")
    V = mesh.vertices.shape[0]
    carried = torch.cat([mesh.vertex_color, mesh.color_valid.to(mesh.vertex_color.dtype)[:, None]], dim=1) if coloured else None
    r = decimate_mesh(mesh.vertices, mesh.faces, target_faces=target_faces, ratio=ratio, max_cost=max_cost, max_edge=max_edge,
                      max_normal_deg=max_normal_deg, pinned=pinned, quadrics=quadrics, max_rounds=max_rounds, attributes=carried)
    stats = dict(mesh.stats)
    stats["decimate"] = dict(r.stats, vertex_map=r.vertex_map, face_map=r.face_map, quadrics_after=r.quadrics)
    stats.update(num_vertices=int(r.vertices.shape[0]), num_faces=int(r.faces.shape[0]))
    if coloured:
        return mesh._replace(vertices=r.vertices, faces=r.faces, vertex_color=r.attributes[:, :-1].contiguous(),
                             color_valid=r.attributes[:, -1] != 0, stats=stats)
    if not hasattr(mesh, "vertex_map"):
        return mesh._replace(vertices=r.vertices, faces=r.faces, stats=stats)
    at = r.face_map.to(torch.int64)
    old = mesh.vertex_map.to(torch.int64)
    composed = torch.where((old >= 0) & (old < V), r.vertex_map[old.clamp(0, max(V - 1, 0))] if V else mesh.vertex_map, mesh.vertex_map)
    return mesh._replace(vertices=r.vertices, faces=r.faces, faces_color=mesh.faces_color[at] if mesh.faces_color is not None else None,
                         vertex_map=composed.to(mesh.vertex_map.dtype), stats=stats)


__all__ = ["DECIMATE_STATES", "DECIMATE_GUARDS", "TOTAL_NAMES", "MAX_RING", "DecimatedRound", "DecimatedMesh", "vertex_quadrics", "decimate_round",
           "cheapest_edges", "decimate_mesh", "decimate_fused"]
