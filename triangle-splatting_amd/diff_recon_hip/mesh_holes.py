"""Closing the holes of an indexed mesh, on the device: its boundary loops found, ordered and numbered, and a centroid fan over each short one.

    boundary_loops(num_vertices, faces, keep=None, adjacency=None) -> BoundaryLoops     every boundary loop as CSR over half-edges
    loop_vertices(loops, faces) -> (L,) int32                                            the member tails: the vertices along the loops
    fill_holes(vertices, faces, max_loop_edges=None, vertex_attributes=None, attribute_valid=None, keep=None, loops=None) -> FilledMesh
    fill_fused(mesh, max_loop_edges)                                                     the pass behind a fusion, before smooth_fused

A region no view observed has weight 0 in a fused volume; the cells that touch it emit nothing and the surface ends there in a boundary loop.
This is the pass between extraction and smooth_mesh that closes the small ones.  The result is a pure function of the input
(include/ts_holes.h), bit-equal to a numpy reference:

    half-edge  face f, corner k, is half-edge 3 f + k, from faces[f][k] (its tail) to faces[f][(k + 1) % 3] (its head); it is a boundary
               half-edge iff its face takes part (kept, indices in range and distinct) and vertex_adjacency counts one face on its edge
    loop       a vertex is simple iff exactly one boundary half-edge leaves it and exactly one arrives; the successor of a boundary half-edge
               is the one that leaves its head, if that head is simple.  A loop is a cycle of successors, listed from its smallest half-edge;
               loops are numbered by that half-edge.  Half-edges on chains that end at a vertex that is not simple (a pinch, a bow tie) are
               open: counted, never filled
    fill       a loop longer than max_loop_edges is left alone, and so are the outline of a lone triangle and a loop with a non-finite
               vertex.  A loop of three gets one face; any other gets one new vertex at the float64 mean of its vertices, in loop order, and
               one face per edge, oriented so that the surface's orientation continues over the cap.  Attributes are averaged over the
               members that have one

A centroid fan over a long loop is flat and slivered: max_loop_edges is what keeps the outer boundary of an open surface open.

Native code: libts_holes.so beside this file (include/ts_holes.h, csrc/mesh_holes.hip), a ninth library because the export lists of the
other eight are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError.  A loop's status and sums are one
thread's work (sequential by definition): a loop of very many edges is a serial walk unless max_loop_edges turns it away."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, NamedTuple, Optional

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_holes

from .mesh_weld import _device_of, _faces_arg, _keep_arg, _vertices_arg

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_holes.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The boundary-loop and hole-filling kernels have no CPU fallback."
    )
_lib = bind_holes(C.CDLL(_LIB_PATH))

LOOP_STATUS = {"filled": 0, "too_long": 1, "lone_face": 2, "dead": 3}  # TSH_FILLED .. TSH_DEAD
UNBOUNDED = 2 ** 31 - 1                                                # max_loop_edges=None


class BoundaryLoops(NamedTuple):
    half_edge_loop: torch.Tensor   # (3 F,) int32: the loop of every half-edge, or -1
    loop_offsets: torch.Tensor     # (loops + 1,) int32: loop i is [loop_offsets[i], loop_offsets[i + 1]) of loop_half_edges
    loop_half_edges: torch.Tensor  # (members,) int32: the half-edges of every loop, from its smallest along the boundary
    stats: Dict[str, int]          # boundary_half_edges, loop_half_edges, loops, nonsimple_vertices, open_half_edges


class FilledMesh(NamedTuple):
    vertices: torch.Tensor                     # (V + new, 3) float32: the input's vertices, then the new ones
    faces: torch.Tensor                        # (F + new, 3) int32: the input's faces, then the new ones
    vertex_attributes: Optional[torch.Tensor]  # (V + new, C) float32, or None
    attribute_valid: Optional[torch.Tensor]    # (V + new,) bool, or None
    new_vertex: torch.Tensor                   # (V + new,) bool: smooth_mesh(pinned=~new_vertex) relaxes the caps alone
    face_loop: torch.Tensor                    # (F + new,) int32: the loop a new face closes, -1 for the input's faces
    loop_status: torch.Tensor                  # (loops,) uint8: LOOP_STATUS
    loops: BoundaryLoops
    stats: Dict[str, object]


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tsh_last_error().decode()} (ts2d error {rc})")


def _workspace(V: int, F: int, device) -> torch.Tensor:
    return torch.empty((_lib.tsh_workspace_bytes(V, F),), device=device, dtype=torch.uint8)


def _loops_arrays(V: int, f: torch.Tensor, k: Optional[torch.Tensor], offsets: torch.Tensor, neighbors: torch.Tensor, edge_faces: torch.Tensor,
                  num_entries: int, device):
    """(half_edge_loop (3 F,), loop_offsets (F + 1,), loop_half_edges (3 F,), counts (4,) int64) as tsh_loops writes them.  Nothing is read back."""
    F = f.shape[0]
    with torch.cuda.device(device):
        half_edge_loop = torch.empty((3 * F,), device=device, dtype=torch.int32)
        loop_offsets = torch.empty((F + 1,), device=device, dtype=torch.int32)
        loop_half_edges = torch.empty((3 * F,), device=device, dtype=torch.int32)
        counts = torch.empty((4,), device=device, dtype=torch.int64)
        ws = _workspace(V, F, device) if V and F else None
        _check(_lib.tsh_loops(V, F, f.data_ptr() if F else None, _native._ptr(k), offsets.data_ptr(), neighbors.data_ptr() if num_entries else None,
                              edge_faces.data_ptr() if num_entries else None, num_entries, half_edge_loop.data_ptr() if F else None,
                              loop_offsets.data_ptr(), loop_half_edges.data_ptr() if F else None, counts.data_ptr(), _native._ptr(ws),
                              ws.numel() if ws is not None else 0, _native.stream()), "boundary_loops")
    return half_edge_loop, loop_offsets, loop_half_edges, counts


def boundary_loops(num_vertices: int, faces: torch.Tensor, keep: Optional[torch.Tensor] = None, adjacency=None) -> BoundaryLoops:
    """The boundary loops of an indexed mesh (module text).  adjacency: vertex_adjacency's result for these faces and this keep, when it is
    at hand.  loop_offsets / loop_half_edges are trimmed to stats["loops"] / stats["loop_half_edges"], the one host read beyond the
    adjacency's."""
    V = int(num_vertices)
    if V < 0:
        raise ValueError("num_vertices must be >= 0")
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    device = _device_of("boundary_loops", f, k)
    if adjacency is None:
        from .mesh_smooth import vertex_adjacency
        adjacency = vertex_adjacency(V, f, k)
    if adjacency.offsets.shape != (V + 1,):
        raise RuntimeError("adjacency was built for another number of vertices")
    _device_of("boundary_loops", f, adjacency.offsets, adjacency.neighbors, adjacency.edge_faces)
    nb, ef = adjacency.neighbors.contiguous(), adjacency.edge_faces.contiguous()
    half_edge_loop, loop_offsets, loop_half_edges, counts = _loops_arrays(V, f, k, adjacency.offsets.contiguous(), nb, ef,
                                                                          min(nb.shape[0], ef.shape[0]), device)
    boundary, members, loops, nonsimple = (int(x) for x in counts.tolist())
    stats = {"boundary_half_edges": boundary, "loop_half_edges": members, "loops": loops, "nonsimple_vertices": nonsimple,
             "open_half_edges": boundary - members}
    return BoundaryLoops(half_edge_loop, loop_offsets[:loops + 1].contiguous(), loop_half_edges[:members].contiguous(), stats)


def loop_vertices(loops: BoundaryLoops, faces: torch.Tensor) -> torch.Tensor:
    """(members,) int32: the tail of every member of loop_half_edges, i.e. the vertices along every loop, split by loop_offsets."""
    f = _faces_arg(faces)
    return f.reshape(-1)[loops.loop_half_edges.to(torch.int64)]


def _fill_arrays(v: torch.Tensor, f: torch.Tensor, loop_offsets: torch.Tensor, loop_half_edges: torch.Tensor, num_loops: int, num_members: int,
                 max_loop_edges: int, attrs: Optional[torch.Tensor], valid: Optional[torch.Tensor], device):
    """(loop_status, new_vertices, new_attributes, new_attr_valid, new_faces, new_face_loop, totals) to their capacity, as tsh_fill writes them."""
    V, F = v.shape[0], f.shape[0]
    channels = attrs.shape[1] if attrs is not None else 0
    with torch.cuda.device(device):
        status = torch.empty((num_loops,), device=device, dtype=torch.uint8)
        new_vertices = torch.empty((num_loops, 3), device=device, dtype=torch.float32)
        new_attrs = torch.empty((num_loops, channels), device=device, dtype=torch.float32) if channels else None
        new_valid = torch.empty((num_loops,), device=device, dtype=torch.uint8) if channels else None
        new_faces = torch.empty((num_members, 3), device=device, dtype=torch.int32)
        new_face_loop = torch.empty((num_members,), device=device, dtype=torch.int32)
        totals = torch.empty((3,), device=device, dtype=torch.int64)
        ws = _workspace(V, F, device) if num_loops else None
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        _check(_lib.tsh_fill(V, F, ptr(v), ptr(f), num_loops, ptr(loop_offsets), ptr(loop_half_edges), num_members, max_loop_edges, ptr(attrs),
                             ptr(valid) if channels else None, channels, ptr(status), ptr(new_vertices), ptr(new_attrs), ptr(new_valid),
                             ptr(new_faces), ptr(new_face_loop), totals.data_ptr(), _native._ptr(ws), ws.numel() if ws is not None else 0,
                             _native.stream()), "fill_holes")
    return status, new_vertices, new_attrs, new_valid, new_faces, new_face_loop, totals


def fill_holes(vertices: torch.Tensor, faces: torch.Tensor, max_loop_edges: Optional[int] = None, vertex_attributes: Optional[torch.Tensor] = None,
               attribute_valid: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
               loops: Optional[BoundaryLoops] = None) -> FilledMesh:
    """Closes every boundary loop of at most max_loop_edges edges (None: every loop) with a centroid fan (module text).  The input's vertices
    and faces come first, bit for bit (all of them: `keep` only says which faces take part in the boundary); vertex_attributes (V, C) float32
    and attribute_valid (V,) bool / uint8 are carried to the new vertices; loops: boundary_loops' result for these faces and this keep, when
    it is at hand.  stats: boundary_loops' four counts and open_half_edges, filled_loops, new_vertices, new_faces, the number of loops per
    status (LOOP_STATUS's names) and longest_loop."""
    limit = UNBOUNDED if max_loop_edges is None else int(max_loop_edges)
    if limit < 0:
        raise ValueError("max_loop_edges must be >= 0 or None")
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    device = _device_of("fill_holes", v, f, k, vertex_attributes, attribute_valid)
    V, F = v.shape[0], f.shape[0]
    attrs = valid = None
    if vertex_attributes is not None:
        if vertex_attributes.dim() != 2 or vertex_attributes.shape[0] != V:
            raise RuntimeError("vertex_attributes must have dimensions (num_vertices, C)")
        attrs = vertex_attributes.detach().to(torch.float32).contiguous()
        if attribute_valid is not None:
            if attribute_valid.shape != (V,) or attribute_valid.dtype not in (torch.bool, torch.uint8):
                raise RuntimeError("attribute_valid must be a bool or uint8 tensor with dimensions (num_vertices,)")
            valid = attribute_valid.contiguous()
    elif attribute_valid is not None:
        raise RuntimeError("attribute_valid needs vertex_attributes")
    if loops is None:
        loops = boundary_loops(V, f, k)
    if loops.half_edge_loop.shape != (3 * F,):
        raise RuntimeError("loops were found for another number of faces")
    num_loops, num_members = loops.loop_offsets.shape[0] - 1, loops.loop_half_edges.shape[0]
    status, new_vertices, new_attrs, new_valid, new_faces, new_face_loop, totals = _fill_arrays(
        v, f, loops.loop_offsets, loops.loop_half_edges, num_loops, num_members, limit, attrs, valid, device)
    filled, nv, nf = (int(x) for x in totals.tolist())
    with torch.cuda.device(device):
        out_v = torch.cat([v, new_vertices[:nv]])
        out_f = torch.cat([f, new_faces[:nf]])
        new_vertex = torch.zeros((V + nv,), device=device, dtype=torch.bool)
        new_vertex[V:] = True
        face_loop = torch.cat([torch.full((F,), -1, device=device, dtype=torch.int32), new_face_loop[:nf]])
        out_a = out_valid = None
        if attrs is not None:
            if attrs.shape[1]:
                out_a = torch.cat([attrs, new_attrs[:nv]])
                out_valid = torch.cat([valid != 0 if valid is not None else torch.ones((V,), device=device, dtype=torch.bool), new_valid[:nv] != 0])
            else:
                out_a = torch.cat([attrs, attrs.new_zeros((nv, 0))])
                out_valid = torch.cat([valid != 0 if valid is not None else torch.ones((V,), device=device, dtype=torch.bool),
                                       torch.zeros((nv,), device=device, dtype=torch.bool)])
        per_status = torch.bincount(status.to(torch.int64), minlength=4).tolist() if num_loops else [0, 0, 0, 0]
        longest = int(torch.diff(loops.loop_offsets).max().item()) if num_loops else 0
    stats = dict(loops.stats)
    stats.update(filled_loops=filled, new_vertices=nv, new_faces=nf, longest_loop=longest,
                 **{name: int(per_status[code]) for name, code in LOOP_STATUS.items()})
    return FilledMesh(out_v, out_f, out_a, out_valid, new_vertex, face_loop, status, loops, stats)


def fill_fused(mesh, max_loop_edges: Optional[int]):
    """The pass behind a fusion: `mesh` is what volume.extract() / fuse_mesh / fuse_colored_mesh / simplify_fused / smooth_fused returned (a
    WeldedMesh or a ColoredMesh); fill_holes with max_loop_edges.  Returns the same kind of mesh: a ColoredMesh carries vertex_color /
    color_valid through as attributes (a cap's vertex takes the mean colour of its loop's vertices that have one, 0.5 where none has); a
    WeldedMesh keeps vertex_map / face_keep (they speak of the fusion's soup, which gained nothing) and faces_color becomes None.  stats
    keeps the fusion's entries, updates num_vertices / num_faces and gains fill_holes' under "fill"."""
    coloured = hasattr(mesh, "vertex_color")
    color, valid = (mesh.vertex_color, mesh.color_valid) if coloured else (None, None)
    r = fill_holes(mesh.vertices, mesh.faces, max_loop_edges, vertex_attributes=color, attribute_valid=valid)
    stats = dict(mesh.stats)
    stats["fill"] = r.stats
    stats.update(num_vertices=int(r.vertices.shape[0]), num_faces=int(r.faces.shape[0]))
    if coloured:
        color = torch.where(r.attribute_valid[:, None], r.vertex_attributes, torch.full_like(r.vertex_attributes, 0.5))
        return mesh._replace(vertices=r.vertices, faces=r.faces, vertex_color=color, color_valid=r.attribute_valid, stats=stats)
    return mesh._replace(vertices=r.vertices, faces=r.faces, faces_color=None, stats=stats)


__all__ = ["BoundaryLoops", "FilledMesh", "boundary_loops", "loop_vertices", "fill_holes", "fill_fused", "LOOP_STATUS"]
