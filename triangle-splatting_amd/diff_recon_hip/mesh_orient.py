"""Orienting an indexed mesh consistently, on the device: every orientable piece made to wind one way, the pieces that cannot be oriented
reported, the way each piece faces chosen by a stated rule.

    orient_faces(vertices, faces, keep=None, outward="majority") -> OrientedMesh   the faces with some rows reversed, the flips, the pieces
    orient_fused(mesh, outward="majority")                                          the pass behind manifold_fused, before fill_fused

A welded soup has no preferred winding and a simplified mesh has conflicts where cells pinch; vertex_normals cancels where two neighbours
wind opposite ways, fill_holes continues whatever orientation it finds, and a viewer that culls back faces shows holes.  This is the pass
that repairs it.  The result is a pure function of the input (include/ts_orient.h), bit-equal to a numpy reference:

    link      an edge used by exactly two participating half-edges links its two faces: EVEN when the half-edges run in opposite directions,
              ODD when they run in the same direction (a conflict); an edge used once or three times and more links nothing
    piece     a connected component of the links, labelled by its smallest face, its anchor
    flip      the parity of any path from the anchor, found by a lock-free union-find over the doubled graph (every face as given and
              reversed); a piece in which both parities reach a face is NON-ORIENTABLE (a Moebius strip, a Klein bottle): counted, its
              faces returned bit for bit
    outward   "anchor": the anchor keeps its direction; "majority": the piece is inverted when more than half of its faces would be
              flipped, which changes the fewest faces; "volume": the piece is inverted when its signed volume about its anchor vertex is
              negative, so a closed piece faces outward
    written   a reversed face (a, b, c) becomes (a, c, b); every other row, and every face that does not take part (not kept, an index out
              of range or repeated), comes back bit for bit

Vertices, per-vertex and per-face fields are untouched: the faces keep their order and number.  Run after split_nonmanifold, where every
shared edge links; an edge that three faces share links nothing.

Native code: libts_orient.so beside this file (include/ts_orient.h, csrc/mesh_orient.hip), an eleventh library because the export lists
of the other ten are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, NamedTuple, Optional

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_orient

from .mesh_weld import _device_of, _faces_arg, _keep_arg, _vertices_arg

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_orient.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The face-orientation kernels have no CPU fallback."
    )
_lib = bind_orient(C.CDLL(_LIB_PATH))

COUNT_NAMES = ("faces", "pieces", "nonorientable_pieces", "nonorientable_faces", "linking_edges", "same_direction_before",
               "same_direction_after", "faces_flipped", "pieces_inverted", "nonfinite_terms")  # tsw_orient's ten words
OUTWARD = {"anchor": 0, "majority": 1, "volume": 2}  # tsw_orient's modes


class OrientedMesh(NamedTuple):
    faces: torch.Tensor       # (F, 3) int32: the input's faces, the flipped rows as (a, c, b)
    face_flip: torch.Tensor   # (F,) bool: the rows that were reversed
    face_piece: torch.Tensor  # (F,) int32: the smallest face of every face's piece, or -1
    stats: Dict[str, int]     # COUNT_NAMES


def library_path() -> str:
    return _LIB_PATH


def _mode(outward: str) -> int:
    if outward not in OUTWARD:
        raise ValueError(f"outward must be one of {', '.join(OUTWARD)}, got {outward!r}")
    return OUTWARD[outward]


def _orient_arrays(v: Optional[torch.Tensor], V: int, f: torch.Tensor, k: Optional[torch.Tensor], mode: int, device):
    """(face_piece (F,) int32, face_flip (F,) uint8, out_faces (F, 3) int32, counts (10,) int64) as tsw_orient writes them.  Nothing is read
    back.  v: the (V, 3) fp32 vertices, handed to the library in mode 2 only."""
    F = f.shape[0]
    with torch.cuda.device(device):
        face_piece = torch.empty((F,), device=device, dtype=torch.int32)
        face_flip = torch.empty((F,), device=device, dtype=torch.uint8)
        out_faces = torch.empty((F, 3), device=device, dtype=torch.int32)
        counts = torch.empty((10,), device=device, dtype=torch.int64)
        ws = torch.empty((_lib.tsw_workspace_bytes(V, F),), device=device, dtype=torch.uint8) if V and F else None
        rc = _lib.tsw_orient(V, F, v.data_ptr() if mode == 2 and V else None, f.data_ptr() if F else None, _native._ptr(k), mode,
                             face_piece.data_ptr() if F else None, face_flip.data_ptr() if F else None, out_faces.data_ptr() if F else None,
                             counts.data_ptr(), _native._ptr(ws), ws.numel() if ws is not None else 0, _native.stream())
        if rc != 0:
            raise RuntimeError(f"orient_faces: {_lib.tsw_last_error().decode()} (ts2d error {rc})")
    return face_piece, face_flip, out_faces, counts


def orient_faces(vertices: torch.Tensor, faces: torch.Tensor, keep: Optional[torch.Tensor] = None, outward: str = "majority") -> OrientedMesh:
    """Makes every orientable piece of the mesh wind one way (module text).  `keep` only says which faces take part; all F faces are returned,
    in their order.  stats: the ten counts of tsw_orient under COUNT_NAMES; one host read."""
    mode = _mode(outward)
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    device = _device_of("orient_faces", v, f, k)
    face_piece, face_flip, out_faces, counts = _orient_arrays(v, v.shape[0], f, k, mode, device)
    stats = dict(zip(COUNT_NAMES, (int(x) for x in counts.tolist())))
    return OrientedMesh(out_faces, face_flip != 0, face_piece, stats)


def orient_fused(mesh, outward: str = "majority"):
    """The pass behind a fusion: `mesh` is what volume.extract() / fuse_mesh / fuse_colored_mesh / simplify_fused / manifold_fused returned
    (a WeldedMesh or a ColoredMesh); orient_faces.  Returns the same kind of mesh with `faces` replaced and orient_faces' stats under
    stats["orient"]; every other field is the input's own."""
    r = orient_faces(mesh.vertices, mesh.faces, outward=outward)
    stats = dict(mesh.stats)
    stats["orient"] = dict(r.stats, outward=outward)
    return mesh._replace(faces=r.faces, stats=stats)


__all__ = ["OrientedMesh", "orient_faces", "orient_fused", "COUNT_NAMES", "OUTWARD"]
