"""Smoothing and shading an indexed mesh, on the device: the one-ring of every vertex, Taubin lambda|mu smoothing over it, and the unit
normals of faces and vertices.

    vertex_adjacency(num_vertices, faces, keep=None) -> MeshAdjacency      the one-ring of every vertex as CSR, edge use counts, vertex classes
    smooth_mesh(vertices, faces, iterations=10, lam=0.5, mu=-0.53, boundary="fixed", pinned=None, max_move=None, adjacency=None)
                                                     -> SmoothedMesh        Taubin smoothing (mu=0: the plain Laplacian, which shrinks)
    face_normals(vertices, faces, keep=None) / vertex_normals(vertices, faces, weighting="area", keep=None) -> (normals, valid)
    smooth_fused(mesh, volume, iterations=10, max_move_voxels=1.0, **kw)    the pass behind a fusion, bounded in voxels of its volume
    mesh_normal_consistency(mesh_a, mesh_b, samples, seed=0) -> dict        the score reported beside Chamfer and F-score
    save_glb_shaded_mesh(path, vertices, faces, vertex_normal, vertex_color=None)   save_glb_mesh's container with a NORMAL accessor

The level set that volume.py extracts carries the depth noise of its views and the staircase of its grid; this is the pass between
extraction and simplify_mesh.  The result is a pure function of the input (include/ts_smooth.h), bit-equal to a numpy
float64 reference:

    one-ring   a face takes part iff it is kept, its indices are in range and pairwise distinct; row v of the CSR table holds v's distinct
               neighbours ascending, and beside each the number of faces that use the edge
    classes    isolated (empty row), interior (every edge used twice), boundary (some edge used once, none three times), nonmanifold
    step       q'_i = q_i + k (mean of the live stencil members - q_i), every read from the previous state, the state in float64 from the
               first step to the last and rounded once; an iteration is the step with lam, then the step with mu
    boundary   "fixed": boundary and nonmanifold vertices stay; "curve": a boundary vertex slides along the boundary curve (its stencil is
               its boundary neighbours); "free": every vertex uses its whole row
    max_move   no vertex ends farther than max_move from where it started, on any axis
    normals    the cross product (p1 - p0) x (p2 - p0) in float64, normalised; a vertex sums its faces' cross products ("area") or their unit
               normals ("uniform") in ascending face order

Native code: libts_smooth.so beside this file (include/ts_smooth.h, csrc/mesh_smooth.hip), an eighth library because the export lists of the
other seven are closed; bound with ctypes.  No CPU / eager fallback: a missing library is an ImportError.  A vertex is one thread's work
(its sums are sequential by definition): a hub of very high degree is a serial walk."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import struct
from pathlib import Path
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D._abi import bind_smooth

from .mesh_weld import _device_of, _faces_arg, _keep_arg, _vertices_arg

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libts_smooth.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: build it with `python triangle-splatting_amd/build.py` (hipcc, gfx950). "
        "The mesh smoothing and normal kernels have no CPU fallback."
    )
_lib = bind_smooth(C.CDLL(_LIB_PATH))

VERTEX_CLASSES = {"isolated": 0, "interior": 1, "boundary": 2, "nonmanifold": 3}  # TSS_ISOLATED .. TSS_NONMANIFOLD
BOUNDARY_MODES = {"fixed": 0, "curve": 1, "free": 2}                              # TSS_BOUNDARY_FIXED / _CURVE / _FREE
NORMAL_WEIGHTINGS = {"area": 0, "uniform": 1}                                     # TSS_NORMAL_AREA / _UNIFORM


class MeshAdjacency(NamedTuple):
    offsets: torch.Tensor       # (V + 1,) int32: row v is [offsets[v], offsets[v + 1])
    neighbors: torch.Tensor     # (entries,) int32: the distinct neighbours of every vertex, ascending per row
    edge_faces: torch.Tensor    # (entries,) int32: the number of faces that use the edge to that neighbour
    vertex_class: torch.Tensor  # (V,) uint8: VERTEX_CLASSES
    stats: Dict[str, int]       # entries, boundary, manifold, nonmanifold (counted over entries: twice the edge census)


class SmoothedMesh(NamedTuple):
    vertices: torch.Tensor      # (V, 3) float32
    adjacency: MeshAdjacency
    stats: Dict[str, object]    # moved, max_displacement


def library_path() -> str:
    return _LIB_PATH


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {_lib.tss_last_error().decode()} (ts2d error {rc})")


def _workspace(V: int, F: int, device) -> torch.Tensor:
    return torch.empty((_lib.tss_workspace_bytes(V, F),), device=device, dtype=torch.uint8)


def _adjacency_arrays(V: int, f: torch.Tensor, k: Optional[torch.Tensor], device):
    """(offsets, neighbors, edge_faces, vertex_class, counts) with all 6 F entries, as tss_adjacency writes them.  Nothing is read back."""
    F = f.shape[0]
    with torch.cuda.device(device):
        offsets = torch.empty((V + 1,), device=device, dtype=torch.int32)
        neighbors = torch.empty((6 * F,), device=device, dtype=torch.int32)
        edge_faces = torch.empty((6 * F,), device=device, dtype=torch.int32)
        cls = torch.empty((V,), device=device, dtype=torch.uint8)
        counts = torch.empty((4,), device=device, dtype=torch.int64)
        ws = _workspace(V, F, device) if V and F else None
        _check(_lib.tss_adjacency(V, F, f.data_ptr() if F else None, _native._ptr(k), offsets.data_ptr(), neighbors.data_ptr() if F else None,
                                  edge_faces.data_ptr() if F else None, cls.data_ptr() if V else None, counts.data_ptr(), _native._ptr(ws),
                                  ws.numel() if ws is not None else 0, _native.stream()), "vertex_adjacency")
        if V == 0:  # the no-op writes counts only
            offsets.zero_()
            neighbors.fill_(-1)
            edge_faces.zero_()
    return offsets, neighbors, edge_faces, cls, counts


def vertex_adjacency(num_vertices: int, faces: torch.Tensor, keep: Optional[torch.Tensor] = None) -> MeshAdjacency:
    """The one-ring of every vertex (module text).  neighbors / edge_faces are trimmed to stats["entries"], the one host read."""
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    device = _device_of("vertex_adjacency", f, k)
    V = int(num_vertices)
    if V < 0:
        raise ValueError("num_vertices must be >= 0")
    offsets, neighbors, edge_faces, cls, counts = _adjacency_arrays(V, f, k, device)
    entries, boundary, manifold, nonmanifold = (int(x) for x in counts.tolist())
    stats = {"entries": entries, "boundary": boundary, "manifold": manifold, "nonmanifold": nonmanifold}
    return MeshAdjacency(offsets, neighbors[:entries].contiguous(), edge_faces[:entries].contiguous(), cls, stats)


def smooth_mesh(vertices: torch.Tensor, faces: torch.Tensor, iterations: int = 10, lam: float = 0.5, mu: float = -0.53,
                boundary: str = "fixed", pinned: Optional[torch.Tensor] = None, max_move: Optional[float] = None,
                adjacency: Optional[MeshAdjacency] = None) -> SmoothedMesh:
    """Taubin smoothing of an indexed mesh (module text); the faces do not change.  pinned: (V,) bool / uint8, vertices that stay;
    max_move: the per-axis bound on every vertex's displacement (None: none); adjacency: vertex_adjacency's result for these faces, when
    it is at hand.  stats: moved (the vertices whose position changed) and max_displacement (the largest displacement of a finite vertex
    on any axis; float)."""
    if boundary not in BOUNDARY_MODES:
        raise ValueError(f"boundary must be one of {sorted(BOUNDARY_MODES)}, not {boundary!r}")
    iterations, lam, mu = int(iterations), float(lam), float(mu)
    bound = math.inf if max_move is None else float(max_move)
    if iterations < 0:
        raise ValueError("iterations must be >= 0")
    if not (math.isfinite(lam) and math.isfinite(mu)):
        raise ValueError("lam and mu must be finite")
    if not bound >= 0.0:
        raise ValueError("max_move must be >= 0 or None")
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    device = _device_of("smooth_mesh", v, f, pinned)
    V = v.shape[0]
    if pinned is not None:
        if pinned.shape != (V,) or pinned.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError("pinned must be a bool or uint8 tensor with dimensions (num_vertices,)")
        pinned = pinned.contiguous()
    if adjacency is None:
        adjacency = vertex_adjacency(V, f)
    if adjacency.offsets.shape != (V + 1,) or adjacency.vertex_class.shape != (V,):
        raise RuntimeError("adjacency was built for another number of vertices")
    nb, ef = adjacency.neighbors.contiguous(), adjacency.edge_faces.contiguous()
    with torch.cuda.device(device):
        out = torch.empty((V, 3), device=device, dtype=torch.float32)
        moved, displacement = 0, 0.0
        if V:
            ws = _workspace(V, 0, device)
            E = nb.shape[0]
            _check(_lib.tss_smooth(V, v.data_ptr(), adjacency.offsets.data_ptr(), nb.data_ptr() if E else None, ef.data_ptr() if E else None,
                                   min(E, ef.shape[0]), adjacency.vertex_class.data_ptr(), _native._ptr(pinned), lam, mu, iterations,
                                   BOUNDARY_MODES[boundary], bound, out.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream()), "smooth_mesh")
            moved = int((out.view(torch.int32) != v.view(torch.int32)).any(dim=1).sum().item())
            d = (out.to(torch.float64) - v.to(torch.float64)).abs()
            d = d[torch.isfinite(d)]
            displacement = float(d.max().item()) if d.numel() else 0.0
    return SmoothedMesh(out, adjacency, {"moved": moved, "max_displacement": displacement})


def face_normals(vertices: torch.Tensor, faces: torch.Tensor, keep: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(normals (F, 3) float32, valid (F,) bool): the unit normal of every face; zero and invalid for a face that `keep` drops, that names
    a vertex outside [0, V), that has a non-finite coordinate or no area."""
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    device = _device_of("face_normals", v, f, k)
    V, F = v.shape[0], f.shape[0]
    with torch.cuda.device(device):
        normals = torch.empty((F, 3), device=device, dtype=torch.float32)
        valid = torch.empty((F,), device=device, dtype=torch.uint8)
        if F:
            _check(_lib.tss_face_normals(V, F, _native._ptr(v), f.data_ptr(), _native._ptr(k), normals.data_ptr(), valid.data_ptr(),
                                         _native.stream()), "face_normals")
    return normals, valid != 0


def vertex_normals(vertices: torch.Tensor, faces: torch.Tensor, weighting: str = "area", keep: Optional[torch.Tensor] = None,
                   normal_sum: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(normals (V, 3) float32, valid (V,) bool): the normalised sum over every vertex's faces of their cross products ("area") or of their
    unit normals ("uniform").  `normal_sum`: a contiguous (V, 3) float64 tensor that receives the raw sums."""
    if weighting not in NORMAL_WEIGHTINGS:
        raise ValueError(f"weighting must be one of {sorted(NORMAL_WEIGHTINGS)}, not {weighting!r}")
    v = _vertices_arg(vertices)
    f = _faces_arg(faces)
    k = _keep_arg(keep, f.shape[0])
    device = _device_of("vertex_normals", v, f, k, normal_sum)
    V, F = v.shape[0], f.shape[0]
    if normal_sum is not None and (normal_sum.shape != (V, 3) or normal_sum.dtype != torch.float64 or not normal_sum.is_contiguous()):
        raise RuntimeError("normal_sum must be a contiguous float64 tensor with dimensions (num_vertices, 3)")
    with torch.cuda.device(device):
        normals = torch.empty((V, 3), device=device, dtype=torch.float32)
        valid = torch.empty((V,), device=device, dtype=torch.uint8)
        if V:
            ws = _workspace(V, F, device)
            _check(_lib.tss_vertex_normals(V, F, v.data_ptr(), f.data_ptr() if F else None, _native._ptr(k), NORMAL_WEIGHTINGS[weighting],
                                           normals.data_ptr(), valid.data_ptr(), _native._ptr(normal_sum), ws.data_ptr(), ws.numel(),
                                           _native.stream()), "vertex_normals")
    return normals, valid != 0


def smooth_fused(mesh, volume, iterations: int = 10, max_move_voxels: float = 1.0, **kw):
    """The pass behind a fusion: `mesh` is what volume.extract() / fuse_mesh / fuse_colored_mesh returned for `volume` (a WeldedMesh or a
    ColoredMesh); smooth_mesh with max_move = max_move_voxels voxels of that volume (None: no bound), so the surface stays within that of
    its level set on every axis; **kw goes to smooth_mesh (lam, mu, boundary, pinned, adjacency).  The faces and the vertex count do not
    change: the same kind of mesh comes back with new vertices, every other field untouched; stats gains smooth_mesh's under "smooth",
    with max_displacement_voxels beside it."""
    bound = None if max_move_voxels is None else float(max_move_voxels) * float(volume.voxel_size)
    s = smooth_mesh(mesh.vertices, mesh.faces, iterations, max_move=bound, **kw)
    stats = dict(mesh.stats)
    stats["smooth"] = {**s.stats, "iterations": int(iterations), "max_displacement_voxels": s.stats["max_displacement"] / float(volume.voxel_size)}
    return mesh._replace(vertices=s.vertices, stats=stats)


def _one_way_consistency(normals_a, valid_a, sample_face, normals_b, valid_b, closest_face):
    found = closest_face >= 0
    fa, fb = sample_face.to(torch.int64), closest_face.clamp(min=0).to(torch.int64)
    use = found & valid_a[fa] & valid_b[fb]
    dots = (normals_a[fa].to(torch.float64) * normals_b[fb].to(torch.float64)).sum(dim=1)[use]
    n = int(dots.numel())
    mean = float(dots.sum().item()) / n if n else float("nan")
    mean_abs = float(dots.abs().sum().item()) / n if n else float("nan")
    return mean, mean_abs, n, int(use.numel()) - n


def mesh_normal_consistency(mesh_a, mesh_b, samples: int, seed: int = 0) -> Dict[str, object]:
    """Normal consistency between mesh_a = (vertices, faces) and mesh_b: `samples` surface points of a, drawn with `seed`
    (sample_mesh_surface: each comes with its face), their closest faces on b (MeshBVH.closest), and the mean over the samples of the dot
    product of the two unit face normals (a_to_b); the same from b to a with `seed + 1` (b_to_a).  normal_consistency is the mean of the
    two, abs_normal_consistency the same with the absolute value of every dot product, for unoriented meshes.  A sample whose own face or
    whose closest face has no valid normal (or that finds no face) is left out and counted in a_dropped / b_dropped; a_count / b_count
    are what remains.  Sums in float64."""
    from .mesh_distance import sample_mesh_surface
    from .mesh_surface import MeshBVH
    (va, fa), (vb, fb) = mesh_a, mesh_b
    na, oka = face_normals(va, fa)
    nb, okb = face_normals(vb, fb)
    sa = sample_mesh_surface(va, fa, samples, seed)
    sb = sample_mesh_surface(vb, fb, samples, int(seed) + 1)
    face_ab, _, _ = MeshBVH(vb, fb).closest(sa.points)
    face_ba, _, _ = MeshBVH(va, fa).closest(sb.points)
    ab, ab_abs, a_count, a_dropped = _one_way_consistency(na, oka, sa.face, nb, okb, face_ab)
    ba, ba_abs, b_count, b_dropped = _one_way_consistency(nb, okb, sb.face, na, oka, face_ba)
    return {"a_to_b": ab, "b_to_a": ba, "normal_consistency": (ab + ba) / 2, "abs_a_to_b": ab_abs, "abs_b_to_a": ba_abs,
            "abs_normal_consistency": (ab_abs + ba_abs) / 2, "a_count": a_count, "b_count": b_count, "a_dropped": a_dropped,
            "b_dropped": b_dropped}


def save_glb_shaded_mesh(path, vertices, faces, vertex_normal, vertex_color=None) -> None:
    """Writes the indexed mesh (vertices (V, 3), faces (F, 3), vertex_normal (V, 3), vertex_color (V, 3) in [0, 1] or None; tensors or
    arrays) as a glTF 2.0 binary in the container of save_glb_mesh: POSITION float32, NORMAL float32, COLOR_0 uint8 VEC4 normalised (alpha
    255; left out without colours), uint32 indices.  diff_recon_hip.mesh_renderer.load_glb_mesh and raw_triangle.read_glb read it back."""
    import numpy as np
    host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    pos = np.ascontiguousarray(host(vertices), dtype="<f4").reshape(-1, 3)
    nrm = np.ascontiguousarray(host(vertex_normal), dtype="<f4").reshape(-1, 3)
    idx = np.ascontiguousarray(host(faces).reshape(-1), dtype="<u4")
    if len(nrm) != len(pos):
        raise ValueError("vertex_normal must have one row per vertex")
    arrays, attributes = [(pos, 34962), (nrm, 34962)], {"POSITION": 0, "NORMAL": 1}
    accessors = [
        {"bufferView": 0, "componentType": 5126, "count": int(len(pos)), "type": "VEC3",
         "min": [float(x) for x in (pos.min(axis=0) if len(pos) else np.zeros(3))], "max": [float(x) for x in (pos.max(axis=0) if len(pos) else np.zeros(3))]},
        {"bufferView": 1, "componentType": 5126, "count": int(len(nrm)), "type": "VEC3"},
    ]
    if vertex_color is not None:
        rgb = np.nan_to_num(host(vertex_color).astype(np.float64).reshape(-1, 3), nan=0.0)
        if len(rgb) != len(pos):
            raise ValueError("vertex_color must have one row per vertex")
        col = np.concatenate([np.round(np.clip(rgb, 0.0, 1.0) * 255.0), np.full((len(pos), 1), 255.0)], axis=1).astype(np.uint8)
        attributes["COLOR_0"] = len(arrays)
        accessors.append({"bufferView": len(arrays), "componentType": 5121, "normalized": True, "count": int(len(col)), "type": "VEC4"})
        arrays.append((np.ascontiguousarray(col), 34962))
    accessors.append({"bufferView": len(arrays), "componentType": 5125, "count": int(len(idx)), "type": "SCALAR"})
    arrays.append((idx, 34963))
    blobs, views, off = [], [], 0
    for arr, target in arrays:
        raw = arr.tobytes()
        views.append({"buffer": 0, "byteOffset": off, "byteLength": len(raw), "target": target})
        raw += b"\x00" * (-len(raw) % 4)
        blobs.append(raw)
        off += len(raw)
    doc = {
        "asset": {"version": "2.0", "generator": "diff_recon_hip.mesh_smooth"},
        "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"name": "geometry_0", "mesh": 0}],
        "meshes": [{"name": "geometry_0", "primitives": [{"attributes": attributes, "indices": len(arrays) - 1, "mode": 4}]}],
        "buffers": [{"byteLength": off}], "bufferViews": views, "accessors": accessors,
    }
    js = json.dumps(doc, separators=(",", ":")).encode("utf-8")
    js += b" " * (-len(js) % 4)
    binary = b"".join(blobs)
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        f.write(struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(js) + 8 + len(binary)))
        f.write(struct.pack("<I4s", len(js), b"JSON") + js)
        f.write(struct.pack("<I4s", len(binary), b"BIN\x00") + binary)


__all__ = ["MeshAdjacency", "SmoothedMesh", "vertex_adjacency", "smooth_mesh", "face_normals", "vertex_normals", "smooth_fused",
           "mesh_normal_consistency", "save_glb_shaded_mesh", "VERTEX_CLASSES", "BOUNDARY_MODES", "NORMAL_WEIGHTINGS"]
