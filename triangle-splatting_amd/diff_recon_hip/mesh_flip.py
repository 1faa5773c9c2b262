"""Improving the connectivity of an indexed mesh, on the device: rounds of edge flips toward the Delaunay condition.

    flip_edges(vertices, faces, keep=None, max_dihedral_deg=30.0, seed=0) -> FlippedMesh       one round
    delaunay_flips(vertices, faces, keep=None, max_dihedral_deg=30.0, max_rounds=64) -> DelaunayMesh    rounds until one flips nothing
    nondelaunay_edges(vertices, faces, keep=None, max_dihedral_deg=30.0, seed=0) -> FlippedMesh  the classification of a round alone
    triangle_quality(vertices, faces, keep=None)                                              4 sqrt(3) area / sum of squared edge lengths
    flip_fused(mesh, max_dihedral_deg=30.0, max_rounds=64)                                      the pass behind a weld, a fusion or a split

split_edges cuts faces from a corner to a midpoint where the marked region ends, fill_holes closes a long loop with a fan of slivers, and
marching tetrahedra and vertex clustering care for position, not shape.  A flip replaces the edge between two faces by the other diagonal
of their quad: no vertex moves, the numbers of vertices, edges and faces stay, and with them closedness, pieces and the Euler
characteristic.  The result is a pure function of the input (include/ts_flip.h), bit-equal to a numpy reference
(tests/ref_mesh_flip.py):

    eligible   an edge of exactly two participating faces that run along it in opposite directions, with distinct opposite vertices c, d and
               finite coordinates
    criterion  the angles at c and d sum to more than pi: decided on dot products and squared cross products in float64, by cases on their
               signs, without a square root or a division; a cocircular quad stays, a zero-area cap goes
    guards     the new edge c-d is not an edge of the mesh already; it would not flip back; the two faces are flatter than max_dihedral_deg
               (creases stay); neither new face folds over
    selection  a candidate wins against the candidates among the four other edges of its two faces by a 32-bit mix of (lo, hi, seed), ties to
               the smaller edge; of the winners that propose the same new edge the smallest edge flips.  The rest wait for the next round

Native code: libts_flip.so beside this file (include/ts_flip.h, csrc/mesh_flip.hip), a seventeenth library because the export lists of the
other sixteen are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, NamedTuple, Optional

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_flip

from .mesh_weld import _device_of, _faces_arg, _keep_arg, _vertices_arg

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_flip.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The edge-flip kernels have no CPU fallback."
    )
_lib = bind_flip(C.CDLL(_LIB_PATH))

EDGE_STATES = {"no_edge": 0, "not_eligible": 1, "delaunay": 2, "guarded": 3, "lost": 4, "duplicate": 5, "flipped": 6}  # TSE_*
TOTAL_NAMES = ("edges", "nondelaunay", "candidates", "flipped")  # tse_flip's four words


class FlippedMesh(NamedTuple):
    faces: Optional[torch.Tensor]         # (F, 3) int32: the input's faces, the slots of flipped pairs rewritten; None from nondelaunay_edges
    face_flipped: Optional[torch.Tensor]  # (F,) bool: the slots that were rewritten; None from nondelaunay_edges
    edge_vertices: torch.Tensor           # (E, 2) int32: (lo, hi), ascending -- the edges of the INPUT
    edge_state: torch.Tensor              # (E,) uint8: EDGE_STATES
    edge_opposite: torch.Tensor           # (E, 2) int32: (c, d) of an eligible edge, -1 otherwise
    stats: Dict[str, int]                 # TOTAL_NAMES, and "guarded" = nondelaunay - candidates


class DelaunayMesh(NamedTuple):
    faces: torch.Tensor         # (F, 3) int32
    face_flipped: torch.Tensor  # (F,) bool: the slots some round rewrote
    converged: bool             # the last round flipped nothing
    stats: Dict[str, object]    # rounds, flipped, guarded, converged, per_round (TOTAL_NAMES each)


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tse_last_error().decode()} (ts2d error {rc})")


def min_cos_of(max_dihedral_deg: float) -> float:
    """cos(max_dihedral_deg) formed once in float64 and rounded to fp32: the min_cos of include/ts_flip.h.  0 <= max_dihedral_deg <= 180."""
    deg = float(max_dihedral_deg)
    if not 0.0 <= deg <= 180.0:
        raise ValueError("max_dihedral_deg must lie in [0, 180]")
    return min(1.0, max(-1.0, C.c_float(math.cos(math.radians(deg))).value))


def _flip_arrays(v: torch.Tensor, f: torch.Tensor, k: Optional[torch.Tensor], min_cos: float, seed: int, classify_only: bool, device):
    """(out_faces (F, 3) and face_flipped (F,) uint8, or None twice; edge_vertices (3 F, 2); edge_state (3 F,) uint8; edge_opposite (3 F, 2);
    totals (4,) int64) as tse_flip writes them, to their capacity.  Nothing is read back."""
    V, F = v.shape[0], f.shape[0]
    with torch.cuda.device(device):
        out_faces = None if classify_only else torch.empty((F, 3), device=device, dtype=torch.int32)
        flipped = None if classify_only else torch.empty((F,), device=device, dtype=torch.uint8)
        ev = torch.empty((3 * F, 2), device=device, dtype=torch.int32)
        state = torch.empty((3 * F,), device=device, dtype=torch.uint8)
        opposite = torch.empty((3 * F, 2), device=device, dtype=torch.int32)
        totals = torch.empty((4,), device=device, dtype=torch.int64)
        ws = torch.empty((_lib.tse_workspace_bytes(V, F),), device=device, dtype=torch.uint8) if F else None
        # an empty tensor still gets an address where the call asks for "given": out_faces / face_flipped decide the mode
        ptr = (lambda t: t.data_ptr() if t is not None and t.numel() else None)
        given = (lambda t: None if t is None else (t.data_ptr() or 1))
        _check(_lib.tse_flip(V, F, ptr(v), ptr(f), _native._ptr(k), min_cos, int(seed) & 0xFFFFFFFF, given(out_faces), given(flipped), ptr(ev),
                             ptr(state), ptr(opposite), totals.data_ptr(), _native._ptr(ws), ws.numel() if ws is not None else 0,
                             _native.stream()), "flip_edges")
    return out_faces, flipped, ev, state, opposite, totals


def _args(what, vertices, faces, keep):
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    return v, f, k, _device_of(what, v, f, k)


def _stats(totals: torch.Tensor) -> Dict[str, int]:
    t = dict(zip(TOTAL_NAMES, (int(x) for x in totals.tolist())))  # the one host read of a round
    t["guarded"] = t["nondelaunay"] - t["candidates"]
    return t


def _one_round(what, vertices, faces, keep, max_dihedral_deg, seed, classify_only) -> FlippedMesh:
    v, f, k, device = _args(what, vertices, faces, keep)
    out_faces, flipped, ev, state, opposite, totals = _flip_arrays(v, f, k, min_cos_of(max_dihedral_deg), seed, classify_only, device)
    t = _stats(totals)
    E = t["edges"]
    return FlippedMesh(out_faces, flipped != 0 if flipped is not None else None, ev[:E], state[:E], opposite[:E], t)


def flip_edges(vertices: torch.Tensor, faces: torch.Tensor, keep: Optional[torch.Tensor] = None, max_dihedral_deg: float = 30.0,
               seed: int = 0) -> FlippedMesh:
    """One round of flips (module text).  `keep` only says which faces take part, all faces are returned; max_dihedral_deg: an edge whose two
    faces meet at a larger angle is a crease and stays (180: every edge may flip); seed: mixed into the priorities, so another seed picks
    another independent set among the same candidates.  The edge table is the input's, trimmed to its E edges.  One host read (the totals)."""
    return _one_round("flip_edges", vertices, faces, keep, max_dihedral_deg, seed, False)


def nondelaunay_edges(vertices: torch.Tensor, faces: torch.Tensor, keep: Optional[torch.Tensor] = None, max_dihedral_deg: float = 30.0,
                      seed: int = 0) -> FlippedMesh:
    """The classification of flip_edges without the flip: faces and face_flipped are None, edge_state says what the round would do (the
    selection included)."""
    return _one_round("nondelaunay_edges", vertices, faces, keep, max_dihedral_deg, seed, True)


def delaunay_flips(vertices: torch.Tensor, faces: torch.Tensor, keep: Optional[torch.Tensor] = None, max_dihedral_deg: float = 30.0,
                   max_rounds: int = 64) -> DelaunayMesh:
    """Rounds of flip_edges with seed = round index until one flips nothing, at most max_rounds of them.  A round that has a candidate flips
    at least one edge, so the last round of a converged run had none: every non-Delaunay edge left is guarded (stats["guarded"]).  On a
    planar triangulation in exact arithmetic the flips end (each one lowers the surface lifted to the paraboloid); for non-planar quads under
    rounding this is no theorem, hence the cap.  One host read per round."""
    if int(max_rounds) < 1:
        raise ValueError("max_rounds must be >= 1")
    v, f, k, device = _args("delaunay_flips", vertices, faces, keep)
    min_cos = min_cos_of(max_dihedral_deg)
    with torch.cuda.device(device):
        union = torch.zeros((f.shape[0],), device=device, dtype=torch.bool)
    per_round, converged, guarded = [], False, 0
    for r in range(int(max_rounds)):
        out_faces, flipped, _, _, _, totals = _flip_arrays(v, f, k, min_cos, r, False, device)
        t = _stats(totals)
        guarded = t["guarded"]
        if t["flipped"] == 0:  # the round copied its input
            converged = True
            break
        per_round.append(t)
        union |= flipped != 0
        f = out_faces
    stats = {"rounds": len(per_round), "flipped": sum(t["flipped"] for t in per_round), "guarded": guarded, "converged": converged,
             "per_round": per_round}
    return DelaunayMesh(f, union, converged, stats)


def triangle_quality(vertices: torch.Tensor, faces: torch.Tensor, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(F,) float64: 4 sqrt(3) area / (sum of the three squared edge lengths), 1 for an equilateral face and 0 for a degenerate one; NaN for a
    face that does not take part (masked, an index out of range or repeated) or has a zero-length perimeter.  Plain torch: for reports."""
    v, f = _vertices_arg(vertices), _faces_arg(faces)  # on whatever device they live
    k = _keep_arg(keep, f.shape[0])
    V = v.shape[0]
    i = f.to(torch.int64)
    ok = ((i >= 0) & (i < V)).all(1) & (i[:, 0] != i[:, 1]) & (i[:, 1] != i[:, 2]) & (i[:, 0] != i[:, 2])
    if k is not None:
        ok &= k != 0
    p = v.double()[i.clamp(0, max(V - 1, 0))] if V else torch.zeros((f.shape[0], 3, 3), device=f.device, dtype=torch.float64)
    e0, e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 1], p[:, 0] - p[:, 2]
    area = 0.5 * torch.linalg.cross(e0, -e2).norm(dim=1)
    total = e0.square().sum(1) + e1.square().sum(1) + e2.square().sum(1)
    q = 4.0 * math.sqrt(3.0) * area / total
    return torch.where(ok, q, torch.full_like(q, float("nan")))


def flip_fused(mesh, max_dihedral_deg: float = 30.0, max_rounds: int = 64):
    """The pass behind a weld, a fusion or a split: `mesh` is a WeldedMesh or a ColoredMesh (weld_mesh, fuse_colored_mesh, split_fused,
    fill_fused ...); delaunay_flips on it.  Returns the same kind of mesh with its faces replaced: vertices, vertex colours, vertex_map and
    face_keep speak of vertices and of the soup, which a flip leaves alone.  The face colours of a WeldedMesh stay with their slots;
    stats["flip"] holds delaunay_flips' stats with face_flipped beside them: the slots whose colour is stale and should be baked again."""
    r = delaunay_flips(mesh.vertices, mesh.faces, max_dihedral_deg=max_dihedral_deg, max_rounds=max_rounds)
    stats = dict(mesh.stats)
    stats["flip"] = dict(r.stats, face_flipped=r.face_flipped)
    return mesh._replace(faces=r.faces, stats=stats)


__all__ = ["EDGE_STATES", "TOTAL_NAMES", "FlippedMesh", "DelaunayMesh", "flip_edges", "delaunay_flips", "nondelaunay_edges", "triangle_quality",
           "flip_fused", "min_cos_of"]
