"""Making an indexed mesh coarser along its own connectivity, on the device: rounds of half-edge collapses of short edges.

    collapse_edges(vertices, faces, keep=None, min_edge=None, vertex_limit=None, max_edge=inf, max_normal_deg=30.0, pinned=None, seed=0)
                                                                                               one round -> CollapsedMesh
    short_edges(...)                                                                           the classification of a round alone
    collapse_short_edges(..., max_rounds=64, compact=True, attributes=None) -> CoarsenedMesh   rounds until one collapses nothing
    collapse_fused(mesh, min_edge, ...)                                                        the pass behind a weld, a fusion, a split or a flip
    isotropic_remesh(vertices, faces, target_edge, iterations=3, ...) -> RemeshedMesh          split, collapse, flip (and smooth), repeated

split_edges makes a mesh finer and flip_edges re-connects it; simplify_mesh merges whatever falls into one grid cell, connected or not, and
cannot aim at one bad face.  A half-edge collapse r -> k along an edge {r, k} replaces r by k in every face around r and deletes the two
faces on the edge: no vertex moves, the output's vertices are a subset of the input's, and closedness, pieces and the Euler characteristic
stay (V - 1, E - 3, F - 2 per collapse).  The result is a pure function of the input (include/ts_collapse.h), bit-equal to a
numpy reference (tests/ref_mesh_collapse.py):

    free       a vertex named by a face that takes part, finite, not pinned, all of whose edges have exactly two faces that run along them
               in opposite directions, with at most 64 corners; every other vertex is held: boundaries and pinned features keep their shape
    eligible   flip_edges' rule, and at least one end is free
    short      shorter than min_edge (than the smaller vertex_limit of its ends)
    direction  hi -> lo first, lo -> hi where hi is held or guarded
    guards     link: no neighbour of r but the two opposite vertices is adjacent to k, and no face would be doubled; long: no new edge is
               longer than max_edge; normal: no face around r turns its normal by more than max_normal_deg, folds or degenerates
    selection  shortest first, ties by a 32-bit mix of (lo, hi, seed), then the smaller edge; a candidate collapses iff it is the first of
               the closed rings of both its ends: no two winners within two edges of each other.  The rest wait for the next round

Native code: libts_collapse.so beside this file (include/ts_collapse.h, csrc/mesh_collapse.hip), an eighteenth library because the export
lists of the other seventeen are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, NamedTuple, Optional

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_collapse

from .mesh_weld import _device_of, _faces_arg, _keep_arg, _vertices_arg

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_collapse.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The edge-collapse kernels have no CPU fallback."
    )
_lib = bind_collapse(C.CDLL(_LIB_PATH))

COLLAPSE_STATES = {"no_edge": 0, "not_eligible": 1, "long_enough": 2, "guarded": 3, "lost": 4, "collapsed": 5}  # TSP_*
COLLAPSE_GUARDS = {"link": 1, "long": 2, "normal": 4, "held": 8}                                               # TSP_GUARD_*
MARK_SHORTER, MARK_VERTEX_LIMIT = 1, 2                                                                         # TSP_MARK_*
MAX_RING = 64                                                                                                  # TSP_MAX_RING
TOTAL_NAMES = ("edges", "short", "candidates", "collapsed")  # tsp_collapse's four words


class CollapsedMesh(NamedTuple):
    faces: Optional[torch.Tensor]          # (F, 3) int32: the input's faces, r replaced by k around every winner; None from short_edges
    face_keep: Optional[torch.Tensor]      # (F,) bool: False on the deleted faces (and where `keep` was); None from short_edges
    vertex_target: Optional[torch.Tensor]  # (V,) int32: k for a removed r, v otherwise; None from short_edges
    edge_vertices: torch.Tensor            # (E, 2) int32: (lo, hi), ascending -- the edges of the INPUT
    edge_state: torch.Tensor               # (E,) uint8: COLLAPSE_STATES
    edge_removed: torch.Tensor             # (E,) int32: r of a candidate, -1 otherwise
    edge_guard: torch.Tensor               # (E,) uint8: COLLAPSE_GUARDS of the directions tried
    stats: Dict[str, int]                  # TOTAL_NAMES, "guarded" = short - candidates, "guarded_<guard>" per bit over the guarded edges


class CoarsenedMesh(NamedTuple):
    vertices: torch.Tensor               # (V', 3) float32: the input's rows that survive (all of them without compact)
    faces: torch.Tensor                  # (F', 3) int32
    face_keep: Optional[torch.Tensor]    # (F,) bool without compact; None with it (every returned face is kept)
    vertex_map: torch.Tensor             # (V,) int32: old -> new; the survivor's index for a removed vertex
    face_map: torch.Tensor               # (F',) int32: new -> old slot
    attributes: Optional[torch.Tensor]   # (V', ...) the input's rows of the surviving vertices, or None
    converged: bool                      # the last round collapsed nothing
    stats: Dict[str, object]             # rounds, collapsed, guarded, converged, num_vertices, num_faces, per_round


class RemeshedMesh(NamedTuple):
    vertices: torch.Tensor
    faces: torch.Tensor
    pinned: Optional[torch.Tensor]  # (V',) bool: the caller's pins carried through the maps, or None
    stats: Dict[str, object]        # target_edge, iterations (per step), quality and edge_length before / after


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsp_last_error().decode()} (ts2d error {rc})")


def min_cos_of(max_normal_deg: float) -> float:
    """cos(max_normal_deg) formed once in float64, rounded to fp32 and clamped to [0, 1]: the min_cos of include/ts_collapse.h.
    0 <= max_normal_deg <= 90."""
    deg = float(max_normal_deg)
    if not 0.0 <= deg <= 90.0:
        raise ValueError("max_normal_deg must lie in [0, 90]")
    return min(1.0, max(0.0, C.c_float(math.cos(math.radians(deg))).value))


def _collapse_arrays(v: torch.Tensor, f: torch.Tensor, k: Optional[torch.Tensor], pinned: Optional[torch.Tensor], mode: int, min_edge: float,
                     limit: Optional[torch.Tensor], max_edge: float, min_cos: float, seed: int, classify_only: bool, device):
    """(out_faces (F, 3), out_keep (F,) uint8 and vertex_target (V,), or None three times; edge_vertices (3 F, 2); edge_state (3 F,) uint8;
    edge_removed (3 F,); edge_guard (3 F,) uint8; totals (4,) int64) as tsp_collapse writes them, to their capacity.  Nothing is read back."""
    V, F = v.shape[0], f.shape[0]
    with torch.cuda.device(device):
        out_faces = None if classify_only else torch.empty((F, 3), device=device, dtype=torch.int32)
        out_keep = None if classify_only else torch.empty((F,), device=device, dtype=torch.uint8)
        target = None if classify_only else torch.empty((V,), device=device, dtype=torch.int32)
        ev = torch.empty((3 * F, 2), device=device, dtype=torch.int32)
        state = torch.empty((3 * F,), device=device, dtype=torch.uint8)
        removed = torch.empty((3 * F,), device=device, dtype=torch.int32)
        guard = torch.empty((3 * F,), device=device, dtype=torch.uint8)
        totals = torch.empty((4,), device=device, dtype=torch.int64)
        ws = torch.empty((_lib.tsp_workspace_bytes(V, F),), device=device, dtype=torch.uint8) if F else None
        # an empty tensor still gets an address where the call asks for "given": the three face outputs decide the mode
        ptr = (lambda t: t.data_ptr() if t is not None and t.numel() else None)
        given = (lambda t: None if t is None else (t.data_ptr() or 1))
        _check(_lib.tsp_collapse(V, F, ptr(v), ptr(f), _native._ptr(k), _native._ptr(pinned), mode, min_edge, _native._ptr(limit), max_edge,
                                 min_cos, int(seed) & 0xFFFFFFFF, given(out_faces), given(out_keep), given(target), ptr(ev), ptr(state),
                                 ptr(removed), ptr(guard), totals.data_ptr(), _native._ptr(ws), ws.numel() if ws is not None else 0,
                                 _native.stream()), "collapse_edges")
    return out_faces, out_keep, target, ev, state, removed, guard, totals


def _rule_args(V: int, min_edge, vertex_limit, max_edge, max_normal_deg, pinned):
    """(mode, min_edge, vertex_limit (V,) float32 or None, max_edge, min_cos, pinned (V,) uint8 / bool or None)."""
    if (min_edge is None) == (vertex_limit is None):
        raise ValueError("give min_edge or vertex_limit (one of them)")
    mode, limit = MARK_SHORTER, None
    if min_edge is not None:
        min_edge = float(min_edge)
        if not min_edge >= 0.0:
            raise ValueError("min_edge must be >= 0")
    else:
        if vertex_limit.shape != (V,):
            raise RuntimeError("vertex_limit must have dimensions (num_vertices,)")
        mode, min_edge, limit = MARK_VERTEX_LIMIT, 0.0, vertex_limit.detach().to(torch.float32).contiguous()
    max_edge = float(max_edge)
    if not max_edge > 0.0:
        raise ValueError("max_edge must be > 0 (inf: no bound)")
    if pinned is not None:
        if pinned.shape != (V,) or pinned.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError("pinned must be a bool or uint8 tensor with dimensions (num_vertices,)")
        pinned = pinned.contiguous()
    return mode, min_edge, limit, max_edge, min_cos_of(max_normal_deg), pinned


def _args(what, vertices, faces, keep, min_edge, vertex_limit, max_edge, max_normal_deg, pinned):
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    rule = _rule_args(v.shape[0], min_edge, vertex_limit, max_edge, max_normal_deg, pinned)
    return v, f, k, rule, _device_of(what, v, f, k, rule[2], rule[5])


def _stats(totals: torch.Tensor, state: torch.Tensor, guard: torch.Tensor) -> Dict[str, int]:
    guarded = state == COLLAPSE_STATES["guarded"]
    bits = torch.stack([(guarded & ((guard & bit) != 0)).sum() for bit in COLLAPSE_GUARDS.values()])
    numbers = [int(x) for x in torch.cat([totals, bits]).tolist()]  # the one host read of a round
    t = dict(zip(TOTAL_NAMES, numbers[:4]))
    t["guarded"] = t["short"] - t["candidates"]
    t.update({f"guarded_{name}": n for name, n in zip(COLLAPSE_GUARDS, numbers[4:])})
    return t


def _round(v, f, k, rule, seed, classify_only, device):
    mode, min_edge, limit, max_edge, min_cos, pinned = rule
    return _collapse_arrays(v, f, k, pinned, mode, min_edge, limit, max_edge, min_cos, seed, classify_only, device)


def _one_round(what, vertices, faces, keep, min_edge, vertex_limit, max_edge, max_normal_deg, pinned, seed, classify_only) -> CollapsedMesh:
    v, f, k, rule, device = _args(what, vertices, faces, keep, min_edge, vertex_limit, max_edge, max_normal_deg, pinned)
    out_faces, out_keep, target, ev, state, removed, guard, totals = _round(v, f, k, rule, seed, classify_only, device)
    t = _stats(totals, state, guard)
    E = t["edges"]
    return CollapsedMesh(out_faces, out_keep != 0 if out_keep is not None else None, target, ev[:E], state[:E], removed[:E], guard[:E], t)


def collapse_edges(vertices: torch.Tensor, faces: torch.Tensor, keep: Optional[torch.Tensor] = None, min_edge: Optional[float] = None,
                   vertex_limit: Optional[torch.Tensor] = None, max_edge: float = math.inf, max_normal_deg: float = 30.0,
                   pinned: Optional[torch.Tensor] = None, seed: int = 0) -> CollapsedMesh:
    """One round of collapses (module text).  min_edge: the edges shorter than it are short; vertex_limit (V,): the edges shorter than the
    smaller limit of their ends; max_edge: no collapse creates a longer edge; max_normal_deg: no face turns its normal further; pinned
    (V,) bool / uint8: vertices that are never removed; seed: mixed into the priorities.  `keep` says which faces take part, all faces are
    returned, face_keep False on the deleted ones; vertices do not change.  The edge table is the input's, trimmed to its E edges.  One
    host read (the totals)."""
    return _one_round("collapse_edges", vertices, faces, keep, min_edge, vertex_limit, max_edge, max_normal_deg, pinned, seed, False)


def short_edges(vertices: torch.Tensor, faces: torch.Tensor, keep: Optional[torch.Tensor] = None, min_edge: Optional[float] = None,
                vertex_limit: Optional[torch.Tensor] = None, max_edge: float = math.inf, max_normal_deg: float = 30.0,
                pinned: Optional[torch.Tensor] = None, seed: int = 0) -> CollapsedMesh:
    """The classification of collapse_edges without the collapse: faces, face_keep and vertex_target are None, edge_state says what the
    round would do (the selection included)."""
    return _one_round("short_edges", vertices, faces, keep, min_edge, vertex_limit, max_edge, max_normal_deg, pinned, seed, True)


def collapse_short_edges(vertices: torch.Tensor, faces: torch.Tensor, keep: Optional[torch.Tensor] = None, min_edge: Optional[float] = None,
                         vertex_limit: Optional[torch.Tensor] = None, max_edge: float = math.inf, max_normal_deg: float = 30.0,
                         pinned: Optional[torch.Tensor] = None, max_rounds: int = 64, compact: bool = True,
                         attributes: Optional[torch.Tensor] = None) -> CoarsenedMesh:
    """Rounds of collapse_edges with seed = round index until one collapses nothing, at most max_rounds of them; every round reads the faces
    and the face_keep of the one before, the vertices never change.  A round that has a candidate collapses at least one edge (the first
    of all candidates wins), so the last round of a converged run had none: every edge still short is guarded or has two held ends
    (stats["guarded"]).  compact: the removed vertices and the deleted faces are dropped once at the end (plain torch: a cumulative sum
    and gathers); vertex_map then names the new index of every old vertex, the survivor's for a removed one, face_map the old slot of every
    face, and `attributes` (V, ...) are gathered to the surviving vertices.  One host read per round."""
    if int(max_rounds) < 1:
        raise ValueError("max_rounds must be >= 1")
    v, f, k, rule, device = _args("collapse_short_edges", vertices, faces, keep, min_edge, vertex_limit, max_edge, max_normal_deg, pinned)
    V, F = v.shape[0], f.shape[0]
    if attributes is not None and (attributes.dim() < 1 or attributes.shape[0] != V):
        raise RuntimeError("attributes must have num_vertices rows")
    with torch.cuda.device(device):
        target = torch.arange(V, device=device, dtype=torch.int64)
        face_keep = k != 0 if k is not None else torch.ones((F,), device=device, dtype=torch.bool)
    per_round, converged, last = [], False, {"guarded": 0}
    for r in range(int(max_rounds)):
        out_faces, out_keep, round_target, _, state, _, guard, totals = _round(v, f, k, rule, r, False, device)
        last = _stats(totals, state, guard)
        if last["collapsed"] == 0:  # the round copied its input
            converged = True
            break
        per_round.append(last)
        f, k = out_faces, out_keep
        face_keep = out_keep != 0
        target = round_target.to(torch.int64)[target]
    stats = {"rounds": len(per_round), "collapsed": sum(t["collapsed"] for t in per_round), "guarded": last["guarded"], "converged": converged,
             "per_round": per_round}
    stats.update({name: n for name, n in last.items() if name.startswith("guarded_")})
    with torch.cuda.device(device):
        if not compact:
            stats.update(num_vertices=V, num_faces=F)
            return CoarsenedMesh(v, f, face_keep, target.to(torch.int32), torch.arange(F, device=device, dtype=torch.int32), attributes,
                                 converged, stats)
        survives = target == torch.arange(V, device=device, dtype=torch.int64)
        new_index = torch.cumsum(survives, 0) - 1
        vertex_map = new_index[target]
        face_map = torch.nonzero(face_keep).reshape(-1)
        old = f[face_map].to(torch.int64)
        named = (old >= 0) & (old < V)  # a face that does not take part keeps an index that names no vertex as it is: it still names none
        new_faces = torch.where(named, vertex_map[old.clamp(0, max(V - 1, 0))] if V else old, old).to(torch.int32)
        kept_rows = torch.nonzero(survives).reshape(-1)
        stats.update(num_vertices=int(kept_rows.shape[0]), num_faces=int(face_map.shape[0]))
        return CoarsenedMesh(v[kept_rows], new_faces, None, vertex_map.to(torch.int32), face_map.to(torch.int32),
                             attributes[kept_rows] if attributes is not None else None, converged, stats)


def collapse_fused(mesh, min_edge: float, max_edge: float = math.inf, max_normal_deg: float = 30.0, max_rounds: int = 64,
                   pinned: Optional[torch.Tensor] = None):
    """The pass behind a weld, a fusion, a split or a flip: `mesh` is a WeldedMesh or a ColoredMesh; collapse_short_edges on it, compacted.
    Returns the same kind of mesh: a ColoredMesh keeps the colour and the validity of its surviving vertices (no vertex moves, nothing is
    interpolated); a WeldedMesh has its face colours follow face_map and its vertex_map composed with the collapse's (face_keep speaks of
    the soup and stays).  stats keeps the mesh's entries, updates num_vertices / num_faces and gains collapse_short_edges' under "collapse"
    with vertex_map and face_map beside them."""
    coloured = hasattr(mesh, "vertex_color")
    V = mesh.vertices.shape[0]
    carried = torch.cat([mesh.vertex_color, mesh.color_valid.to(mesh.vertex_color.dtype)[:, None]], dim=1) if coloured else None
    r = collapse_short_edges(mesh.vertices, mesh.faces, min_edge=min_edge, max_edge=max_edge, max_normal_deg=max_normal_deg, pinned=pinned,
                             max_rounds=max_rounds, attributes=carried)
    stats = dict(mesh.stats)
    stats["collapse"] = dict(r.stats, vertex_map=r.vertex_map, face_map=r.face_map)
    stats.update(num_vertices=int(r.vertices.shape[0]), num_faces=int(r.faces.shape[0]))
    if coloured:
        return mesh._replace(vertices=r.vertices, faces=r.faces, vertex_color=r.attributes[:, :-1].contiguous(),
                             color_valid=r.attributes[:, -1] != 0, stats=stats)
    at = r.face_map.to(torch.int64)
    old = mesh.vertex_map.to(torch.int64)
    composed = torch.where((old >= 0) & (old < V), r.vertex_map[old.clamp(0, max(V - 1, 0))] if V else mesh.vertex_map, mesh.vertex_map)
    return mesh._replace(vertices=r.vertices, faces=r.faces, faces_color=mesh.faces_color[at] if mesh.faces_color is not None else None,
                         vertex_map=composed.to(mesh.vertex_map.dtype), stats=stats)


def _shape_report(vertices, faces) -> Dict[str, object]:
    """triangle_quality (minimum, 1st percentile, median) and the edge lengths (minimum, mean, maximum) of a mesh; two host reads."""
    from .mesh_flip import triangle_quality
    from .mesh_subdivide import mesh_edges
    q = triangle_quality(vertices, faces)
    q = q[~q.isnan()]
    quality = [float(x) for x in torch.quantile(q, torch.tensor([0.0, 0.01, 0.5], device=q.device, dtype=q.dtype)).tolist()] if q.numel() else []
    length = mesh_edges(vertices.shape[0], faces, vertices=vertices).length
    length = length[~length.isnan()]
    spread = [float(length.min()), float(length.mean()), float(length.max())] if length.numel() else []
    return {"quality": quality, "edge_length": spread, "num_vertices": int(vertices.shape[0]), "num_faces": int(faces.shape[0])}


def isotropic_remesh(vertices: torch.Tensor, faces: torch.Tensor, target_edge: float, iterations: int = 3, max_normal_deg: float = 30.0,
                     smooth: bool = False, pinned: Optional[torch.Tensor] = None) -> RemeshedMesh:
    """The remeshing loop of Botsch and Kobbelt on the operators of this package, `iterations` times: split_long_edges above 4/3
    target_edge; collapse_short_edges below 4/5 target_edge, with max_edge = 4/3 target_edge so that the two do not undo each other;
    delaunay_flips; with smooth, one smooth_mesh pass (tangential only insofar as Taubin's pair of steps does not shrink).  A flip knows
    no edge bound, so one more split and collapse closes the loop (stats["closing"]): where the splits converged no returned edge is longer
    than 4/3 target_edge, and every returned edge below 4/5 target_edge is guarded or has two held ends.  pinned (V,)
    bool / uint8 is carried through the maps: a midpoint is pinned iff both ends of its edge are, a survivor keeps its pin.  stats: the
    per-step stats of every iteration, and triangle_quality (minimum / 1st percentile / median) and the edge lengths (minimum / mean /
    maximum) before and after."""
    from .mesh_flip import delaunay_flips
    from .mesh_smooth import smooth_mesh
    from .mesh_subdivide import split_long_edges
    target_edge, iterations = float(target_edge), int(iterations)
    if not (math.isfinite(target_edge) and target_edge > 0.0):
        raise ValueError("target_edge must be finite and > 0")
    if iterations < 1:
        raise ValueError("iterations must be >= 1")
    v, f = _vertices_arg(vertices), _faces_arg(faces)
    pin = None
    if pinned is not None:
        if pinned.shape != (v.shape[0],) or pinned.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError("pinned must be a bool or uint8 tensor with dimensions (num_vertices,)")
        pin = pinned != 0
    _device_of("isotropic_remesh", v, f, pin)
    high, low = 4.0 / 3.0 * target_edge, 4.0 / 5.0 * target_edge
    stats: Dict[str, object] = {"target_edge": target_edge, "before": _shape_report(v, f), "iterations": []}

    def split_and_collapse(v, f, pin, step):
        s = split_long_edges(v, f, max_edge=high)
        if pin is not None:
            ends = s.vertex_edge[v.shape[0]:].to(torch.int64)
            grown = torch.cat([pin, torch.zeros((ends.shape[0],), device=pin.device, dtype=torch.bool)])
            for _ in range(max(1, s.stats["rounds"])):  # a later round's midpoint may halve an edge that ends in an earlier round's
                grown[v.shape[0]:] = grown[ends[:, 0]] & grown[ends[:, 1]]
            pin = grown
        step["split"] = {k: s.stats[k] for k in ("rounds", "converged", "new_vertices", "faces")}
        c = collapse_short_edges(s.vertices, s.faces, min_edge=low, max_edge=high, max_normal_deg=max_normal_deg, pinned=pin, attributes=pin)
        step["collapse"] = {k: c.stats[k] for k in c.stats if k != "per_round"}
        return c.vertices, c.faces, c.attributes

    for _ in range(iterations):
        step: Dict[str, object] = {}
        v, f, pin = split_and_collapse(v, f, pin, step)
        d = delaunay_flips(v, f, max_dihedral_deg=max_normal_deg)
        f = d.faces
        step["flip"] = {k: d.stats[k] for k in ("rounds", "flipped", "guarded", "converged")}
        if smooth:
            m = smooth_mesh(v, f, iterations=1, pinned=pin)
            v = m.vertices
            step["smooth"] = dict(m.stats)
        stats["iterations"].append(step)
    # a flip (and a smoothing step) knows no edge bound: one more split and collapse, so that what is returned has no edge above 4/3
    # target_edge where the split converged, and none below 4/5 target_edge that a collapse could still take
    stats["closing"] = {}
    v, f, pin = split_and_collapse(v, f, pin, stats["closing"])
    stats["after"] = _shape_report(v, f)
    return RemeshedMesh(v, f, pin, stats)


__all__ = ["COLLAPSE_STATES", "COLLAPSE_GUARDS", "TOTAL_NAMES", "MARK_SHORTER", "MARK_VERTEX_LIMIT", "MAX_RING", "CollapsedMesh", "CoarsenedMesh",
           "RemeshedMesh", "collapse_edges", "short_edges", "collapse_short_edges", "collapse_fused", "isotropic_remesh", "min_cos_of"]
