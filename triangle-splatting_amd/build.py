"""Builds libts2d.so (the C-ABI HIP library of include/ts2d.h) for gfx950 with hipcc, in-tree, the package's binding of it, and
libts_geom.so (include/ts_geom.h: the mesh-distance library of diff_recon_hip, GEOM_SOURCES + the product's own radix_sort object) and
libts_bvh.so (include/ts_bvh.h: the triangle index and closest-point query of diff_recon_hip/mesh_surface.py, BVH_SOURCES + the same object) and
libts_ray.so (include/ts_ray.h: the first-hit ray query of diff_recon_hip/mesh_ray.py on that index, RAY_SOURCES + the same object) and
libts_volume.so (include/ts_volume.h: the TSDF volume and the marching tetrahedra of diff_recon_hip/volume.py, VOLUME_SOURCES alone) and
libts_color.so (include/ts_color.h: the colour volume, the grid sampler and the vertex-attribute pass of diff_recon_hip/color_volume.py, COLOR_SOURCES alone) and
libts_simplify.so (include/ts_simplify.h: the vertex clustering, the quadric placement and the duplicate-face sweep of diff_recon_hip/mesh_simplify.py, SIMPLIFY_SOURCES + the radix_sort object) and
libts_smooth.so (include/ts_smooth.h: the one-ring adjacency, the Taubin smoothing and the face / vertex normals of diff_recon_hip/mesh_smooth.py, SMOOTH_SOURCES + the radix_sort object) and
libts_holes.so (include/ts_holes.h: the boundary loops and the centroid fans of diff_recon_hip/mesh_holes.py, HOLES_SOURCES alone) and
libts_manifold.so (include/ts_manifold.h: the vertex fans and the non-manifold split of diff_recon_hip/mesh_manifold.py, MANIFOLD_SOURCES + the radix_sort object) and
libts_orient.so (include/ts_orient.h: the consistent orientation of diff_recon_hip/mesh_orient.py, ORIENT_SOURCES + the radix_sort object) and
libts_atlas.so (include/ts_atlas.h: the texel index, the face totals, the resolve and the draw of diff_recon_hip/mesh_texture.py's texture atlas, ATLAS_SOURCES alone) and
libts_inside.so (include/ts_inside.h: the crossing counts of a ray and the signed distance of diff_recon_hip/mesh_inside.py on the index of libts_bvh.so, INSIDE_SOURCES + the radix_sort object) and
libts_winding.so (include/ts_winding.h: the generalised winding number and its signed distance of diff_recon_hip/mesh_winding.py on the index of libts_bvh.so, WINDING_SOURCES + the radix_sort object) and
libts_overlap.so (include/ts_overlap.h: the triangle-overlap query, self-intersections and mesh-mesh pairs, of diff_recon_hip/mesh_overlap.py on the index of libts_bvh.so, OVERLAP_SOURCES + the radix_sort object) and
libts_subdivide.so (include/ts_subdivide.h: the edge table and the conforming split at the midpoints of marked edges of diff_recon_hip/mesh_subdivide.py, SUBDIVIDE_SOURCES + the radix_sort object) and
libts_flip.so (include/ts_flip.h: the round of edge flips toward the Delaunay condition of diff_recon_hip/mesh_flip.py, FLIP_SOURCES + the radix_sort object) and
libts_collapse.so (include/ts_collapse.h: the round of half-edge collapses of short edges of diff_recon_hip/mesh_collapse.py, COLLAPSE_SOURCES + the radix_sort object) and
libts_decimate.so (include/ts_decimate.h: the vertex quadrics and the round of quadric-error collapses under a budget of diff_recon_hip/mesh_decimate.py, DECIMATE_SOURCES + the radix_sort object) and
libts_contract.so (include/ts_contract.h: the round of quadric-error edge contractions that place the survivor, under a budget, of diff_recon_hip/mesh_contract.py, CONTRACT_SOURCES + the radix_sort object).

    python triangle-splatting_amd/build.py [--force] [--verbose] [--lab]
    python triangle-splatting_amd/build.py --variant TAG [--lab] [--all "FLAGS"] [--unit NAME="FLAGS" ...]

Output: triangle-splatting_amd/diff_triangle_rasterization_2D/libts2d.so, triangle-splatting_amd/diff_recon_hip/libts_geom.so, libts_bvh.so, libts_ray.so, libts_volume.so, libts_color.so, libts_simplify.so, libts_smooth.so, libts_holes.so, libts_manifold.so, libts_orient.so, libts_atlas.so, libts_inside.so, libts_winding.so, libts_overlap.so, libts_subdivide.so, libts_flip.so, libts_collapse.so, libts_decimate.so and libts_contract.so, and the torch extension bindings/_ts2d_torch_C.so (bindings/
ts2d_torch_ext.cpp, linked -lts2d with an $ORIGIN-relative runpath), both git-ignored.  Every library carries the soname libts2d.so, so the
extension's dependency on libts2d.so is met by whichever of them _C.py loaded first (TS2D_LIBRARY_PATH).
--lab builds tools/bin/libts2d_lab.so as well: the same objects + the test hooks of tools/lab/lab_hooks.hip and api.hip compiled with
-DTS2D_LAB, which exports the switches and readers of csrc/ts2d_lab.h.  The product library contains one blend path per variant and reads no
environment; only tools/ and tests/ load the lab library (TS2D_LIBRARY_PATH, see _C.py).
--variant TAG builds an A/B or instrumentation variant instead: each unit named by --unit (an object name of objects(): render_group_fwd,
depth_order, emit, lab/api, ...) is compiled with the product's own command line plus FLAGS into build/variants/TAG/; --all appends FLAGS to every unit (the lab
units too with --lab).  Every other unit links the product's object.  Output: tools/bin/libts2d_TAG.so, with --lab also
tools/bin/libts2d_lab_TAG.so (TS2D_LIBRARY_PATH / TS2D_LAB_LIBRARY_PATH); the product's libraries are not written.  E.g. the lane-group
statistics build: --variant stats --lab --unit render_group_fwd=-DTS2D_STATS --unit render_group_bwd=-DTS2D_STATS; a depth-order switch-over
under test: --variant split16 --unit depth_order=-DTS_DEPTH_SPLIT_MAX_VALUE=1600000; the emission's register budget: --unit emit=-DTS_EMIT_WAVES=5.
hipcc cross-compiles without a GPU.  Per-file flags matter:
  * preprocess.hip is built with -ffp-contract=off (bit-comparable integer state, see the file header);
  * the blend kernels use the default fast contraction and hardware float atomics (-munsafe-fp-atomics).
"""
from __future__ import annotations

import argparse
import hashlib
import os
import re
import shlex
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "diff_triangle_rasterization_2D")
OBJ_DIR = os.path.join(HERE, "build")
VARIANT_DIR = os.path.join(OBJ_DIR, "variants")
LIB = os.path.join(OUT_DIR, "libts2d.so")
EXT_SRC = os.path.join(HERE, "bindings", "ts2d_torch_ext.cpp")
EXT = os.path.join(HERE, "bindings", "_ts2d_torch_C.so")
ARCH = "gfx950"

COMMON = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-munsafe-fp-atomics", "-Wall", "-Wno-unused-function",
          "-Wno-unused-result", "-DNDEBUG", "-fvisibility=hidden"]  # exports = what include/*.h declares (api*.hip), nothing else
SOURCES = {
    "preprocess.hip": ["-ffp-contract=off"],
    "preprocess3d.hip": ["-ffp-contract=off"],
    "mesh_preprocess.hip": ["-ffp-contract=off"],  # the opaque mesh renderer (include/ts_mesh.h): per-face setup ...
    "mesh_resolve.hip": ["-ffp-contract=off"],     # ... and the per-pixel depth test (what is fused there is written as fmaf)
    "mesh_census.hip": [],                         # the per-face census over face_idx (integer sums; nothing to contract)
    "mesh_weld.hip": ["-ffp-contract=off"],        # vertex welding and edge topology (include/ts_weld.h): the fp32 pair test rounds every operation
    "shgrad.hip": ["-ffp-contract=off"],
    "photometric.hip": [],
    "depth_normal.hip": ["-ffp-contract=off"],
    "aux_losses.hip": ["-ffp-contract=off"],
    "regularizers.hip": ["-ffp-contract=off"],
    "resample.hip": ["-ffp-contract=off"],
    "knn.hip": [],
    "model_update.hip": [],
    "optim.hip": ["-ffp-contract=off"],
    "radix_sort.hip": [],   # the binning, three units over csrc/ts2d_radix.h: the radix passes, the tile sort, the sort for other callers ...
    "depth_order.hip": [],  # ... steps 1-2: the triangles in depth order, their tile counts, N ...
    "emit.hip": [],         # ... steps 3 and 5: instance emission, tile ranges
    "select.hip": [],
    # the 2D blend kernels: ONE source, two translation units (TSG_PART), so that each kernel gets the machine-scheduler strategy it measured best
    # with (round 5, profiles/r05_sched_strategies.txt: max-ilp +1.3 % for the forward, -1 % for the backward; round 6: profiles/r06_blend_ab.txt)
    "render_group.hip@fwd": ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-fno-slp-vectorize", "-DTSG_PART=1", "-mllvm", "-amdgpu-sched-strategy=max-ilp"],
    "render_group.hip@bwd": ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-fno-slp-vectorize", "-DTSG_PART=2"],
    "render3d_group.hip": ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-fno-slp-vectorize"],
    "api.hip": [],       # the C ABI, one file per group of public headers (csrc/ts2d_api.h is what they share): include/ts2d.h ...
    "api_loss.hip": [],  # ... ts_loss.h ...
    "api_model.hip": [], # ... ts_model.h, ts_optim.h, ts_knn.h ...
    "api_mesh.hip": [],  # ... ts_mesh.h, ts_weld.h
}
LAB_SOURCES = {  # libts2d_lab.so only
    "lab_hooks.hip": [],  # sort / scan test hooks + their rocPRIM comparators (csrc/ts2d_lab.h)
    "api.hip": ["-DTS2D_LAB"],
}
GEOM_SOURCES = {  # libts_geom.so only (include/ts_geom.h): a second product library, because libts2d.so's export list is closed
    "mesh_distance.hip": ["-ffp-contract=off"],  # cross-set nearest search and surface sampler: every fp32 / fp64 operation rounds
    "api_geom.hip": [],                          # its C ABI and its own error text (api.hip is not linked)
}
GEOM_SHARED = ["radix_sort"]  # the product's own objects it links as well: the radix sort of the search's front half (no undefined project symbol)
GEOM_LIB = os.path.join(HERE, "diff_recon_hip", "libts_geom.so")
BVH_SOURCES = {  # libts_bvh.so only (include/ts_bvh.h): a third product library, the export lists of the other two are closed
    "mesh_bvh.hip": ["-ffp-contract=off"],  # the triangle index and the closest-point query: every fp64 / fp32 operation rounds
    "api_bvh.hip": [],                      # its C ABI and its own error text
}
BVH_SHARED = ["radix_sort"]  # the sort of the Morton codes, of the faces and of the queries
BVH_LIB = os.path.join(HERE, "diff_recon_hip", "libts_bvh.so")
RAY_SOURCES = {  # libts_ray.so only (include/ts_ray.h): a fourth product library, the export lists of the other three are closed
    "mesh_ray.hip": ["-ffp-contract=off"],  # the first hit of a ray on the index of libts_bvh.so (csrc/ts_bvh_layout.h): every fp64 operation rounds
    "api_ray.hip": [],                      # its C ABI and its own error text
}
RAY_SHARED = ["radix_sort"]  # the sort of the Morton codes of the ray origins
RAY_LIB = os.path.join(HERE, "diff_recon_hip", "libts_ray.so")
VOLUME_SOURCES = {  # libts_volume.so only (include/ts_volume.h): a fifth product library, the export lists of the other four are closed
    "volume.hip": ["-ffp-contract=off"],  # TSDF integration, field and marching tetrahedra: every fp64 operation rounds
    "api_volume.hip": [],                 # its C ABI and its own error text
}
VOLUME_LIB = os.path.join(HERE, "diff_recon_hip", "libts_volume.so")  # it links no product object: there is no VOLUME_SHARED
COLOR_SOURCES = {  # libts_color.so only (include/ts_color.h): a sixth product library, the export lists of the other five are closed
    "color_volume.hip": ["-ffp-contract=off"],  # colour integration, colour field, grid sampler, vertex-attribute interpolation: every fp64 operation rounds
    "api_color.hip": [],                        # its C ABI and its own error text
}
COLOR_LIB = os.path.join(HERE, "diff_recon_hip", "libts_color.so")  # it links no product object: there is no COLOR_SHARED
SIMPLIFY_SOURCES = {  # libts_simplify.so only (include/ts_simplify.h): a seventh product library, the export lists of the other six are closed
    "mesh_simplify.hip": ["-ffp-contract=off"],  # cell keys, cluster labels, quadric placement, duplicate-face sweep: every fp64 operation rounds
    "api_simplify.hip": [],                      # its C ABI and its own error text
}
SIMPLIFY_SHARED = ["radix_sort"]  # the sorts of the cell keys, of the cluster members, of the face incidences and of the rotated triples
SIMPLIFY_LIB = os.path.join(HERE, "diff_recon_hip", "libts_simplify.so")
SMOOTH_SOURCES = {  # libts_smooth.so only (include/ts_smooth.h): an eighth product library, the export lists of the other seven are closed
    "mesh_smooth.hip": ["-ffp-contract=off"],  # one-ring adjacency, Taubin steps, face and vertex normals: every fp64 operation rounds
    "api_smooth.hip": [],                      # its C ABI and its own error text
}
SMOOTH_SHARED = ["radix_sort"]  # the two sorts of the directed edge records and the sort of the face incidences
SMOOTH_LIB = os.path.join(HERE, "diff_recon_hip", "libts_smooth.so")
HOLES_SOURCES = {  # libts_holes.so only (include/ts_holes.h): a ninth product library, the export lists of the other eight are closed
    "mesh_holes.hip": ["-ffp-contract=off"],  # boundary loops by pointer doubling, centroid fans: every fp64 operation of the fill rounds
    "api_holes.hip": [],                      # its C ABI and its own error text
}
HOLES_LIB = os.path.join(HERE, "diff_recon_hip", "libts_holes.so")  # it links no product object: there is no HOLES_SHARED
MANIFOLD_SOURCES = {  # libts_manifold.so only (include/ts_manifold.h): a tenth product library, the export lists of the other nine are closed
    "mesh_manifold.hip": [],  # vertex fans by sort and union-find, the split: integers only, so no floating-point flag is needed
    "api_manifold.hip": [],   # its C ABI and its own error text
}
MANIFOLD_SHARED = ["radix_sort"]  # the two sorts of the half-edge records
MANIFOLD_LIB = os.path.join(HERE, "diff_recon_hip", "libts_manifold.so")
ORIENT_SOURCES = {  # libts_orient.so only (include/ts_orient.h): an eleventh product library, the export lists of the other ten are closed
    "mesh_orient.hip": ["-ffp-contract=off"],  # pieces and flips by sort and union-find over the doubled graph; the fp64 volume terms of mode 2 round every operation
    "api_orient.hip": [],                      # its C ABI and its own error text
}
ORIENT_SHARED = ["radix_sort"]  # the two sorts of the half-edge records
ORIENT_LIB = os.path.join(HERE, "diff_recon_hip", "libts_orient.so")
ATLAS_SOURCES = {  # libts_atlas.so only (include/ts_atlas.h): a twelfth product library, the export lists of the other eleven are closed
    "mesh_atlas.hip": ["-ffp-contract=off"],  # the texel of a pixel, face totals, resolve, draw: every fp64 operation rounds (csrc/ts_mesh_bary.h, shared with color_volume.hip)
    "api_atlas.hip": [],                      # its C ABI and its own error text
}
ATLAS_LIB = os.path.join(HERE, "diff_recon_hip", "libts_atlas.so")  # it links no product object: there is no ATLAS_SHARED
INSIDE_SOURCES = {  # libts_inside.so only (include/ts_inside.h): a thirteenth product library, the export lists of the other twelve are closed
    "mesh_inside.hip": ["-ffp-contract=off"],  # all hits of a ray in half crossings, the signed distance: every fp64 operation rounds (csrc/ts_ray_tests.h, shared with mesh_ray.hip)
    "api_inside.hip": [],                      # its C ABI and its own error text
}
INSIDE_SHARED = ["radix_sort"]  # the sort of the Morton codes of the ray origins
INSIDE_LIB = os.path.join(HERE, "diff_recon_hip", "libts_inside.so")
WINDING_SOURCES = {  # libts_winding.so only (include/ts_winding.h): a fourteenth product library, the export lists of the other thirteen are closed
    "mesh_winding.hip": ["-ffp-contract=off"],  # node moments, face and node terms of the generalised winding number, its signed distance: every fp64 operation rounds
    "api_winding.hip": [],                      # its C ABI and its own error text
}
WINDING_SHARED = ["radix_sort"]  # the sort of the Morton codes of the query points
WINDING_LIB = os.path.join(HERE, "diff_recon_hip", "libts_winding.so")
OVERLAP_SOURCES = {  # libts_overlap.so only (include/ts_overlap.h): a fifteenth product library, the export lists of the other fourteen are closed
    "mesh_overlap.hip": ["-ffp-contract=off"],  # plane values and segment tests of the triangle-triangle test, the sort of the pair list: every fp64 operation rounds
    "api_overlap.hip": [],                      # its C ABI and its own error text
}
OVERLAP_SHARED = ["radix_sort"]  # the two sorts of the pair list
OVERLAP_LIB = os.path.join(HERE, "diff_recon_hip", "libts_overlap.so")
SUBDIVIDE_SOURCES = {  # libts_subdivide.so only (include/ts_subdivide.h): a sixteenth product library, the export lists of the other fifteen are closed
    "mesh_subdivide.hip": ["-ffp-contract=off"],  # edge lengths, midpoints, interpolated attributes, the diagonal rule: every fp64 operation rounds
    "api_subdivide.hip": [],                      # its C ABI and its own error text
}
SUBDIVIDE_SHARED = ["radix_sort"]  # the two sorts of the half-edge records
SUBDIVIDE_LIB = os.path.join(HERE, "diff_recon_hip", "libts_subdivide.so")
FLIP_SOURCES = {  # libts_flip.so only (include/ts_flip.h): a seventeenth product library, the export lists of the other sixteen are closed
    "mesh_flip.hip": ["-ffp-contract=off"],  # the criterion, the flatness and the fold guard: every fp64 operation rounds
    "api_flip.hip": [],                      # its C ABI and its own error text
}
FLIP_SHARED = ["radix_sort"]  # the two sorts of the half-edge records and the two of the winners' new edges
FLIP_LIB = os.path.join(HERE, "diff_recon_hip", "libts_flip.so")
COLLAPSE_SOURCES = {  # libts_collapse.so only (include/ts_collapse.h): an eighteenth product library, the export lists of the other seventeen are closed
    "mesh_collapse.hip": ["-ffp-contract=off"],  # edge lengths and the normal guard: every fp64 operation rounds
    "api_collapse.hip": [],                      # its C ABI and its own error text
}
COLLAPSE_SHARED = ["radix_sort"]  # the two sorts of the half-edge records and the sort of the corner records
COLLAPSE_LIB = os.path.join(HERE, "diff_recon_hip", "libts_collapse.so")
DECIMATE_SOURCES = {  # libts_decimate.so only (include/ts_decimate.h): a nineteenth product library, the export lists of the other eighteen are closed
    "mesh_decimate.hip": ["-ffp-contract=off"],  # quadrics, costs and the guards of csrc/ts_collapse_round.h: every fp64 operation rounds
    "api_decimate.hip": [],                      # its C ABI and its own error text
}
DECIMATE_SHARED = ["radix_sort"]  # the sorts of the half-edge and corner records and the three of the ranking
DECIMATE_LIB = os.path.join(HERE, "diff_recon_hip", "libts_decimate.so")
CONTRACT_SOURCES = {  # libts_contract.so only (include/ts_contract.h): a twentieth product library, the export lists of the other nineteen are closed
    "mesh_contract.hip": ["-ffp-contract=off"],  # the edge quadric, the solve, p* and the guards at p*: every fp64 operation rounds
    "api_contract.hip": [],                      # its C ABI and its own error text
}
CONTRACT_SHARED = ["radix_sort"]  # the sorts of the half-edge and corner records and the three of the ranking
CONTRACT_LIB = os.path.join(HERE, "diff_recon_hip", "libts_contract.so")
BIN_DIR = os.path.join(os.path.dirname(HERE), "tools", "bin")
LAB_LIB = os.path.join(BIN_DIR, "libts2d_lab.so")
LAB_SRC = os.path.join(os.path.dirname(HERE), "tools", "lab")  # lab_hooks.hip: the test hooks, outside the product's csrc/; it includes csrc's headers (-I)
HEADERS = ["ts2d_common.h", "ts2d_radix.h", "ts2d_api.h", "ts_knn_front.h", "ts_weld_launch.h", "ts_geom_launch.h", "ts_bvh_launch.h", "ts_bvh_layout.h", "ts_bvh_walk.h", "ts_ray_launch.h", "ts_volume_launch.h", "ts_color_launch.h", "ts_simplify_launch.h", "ts_smooth_launch.h", "ts_holes_launch.h", "ts_manifold_launch.h", "ts_orient_launch.h", "ts_atlas_launch.h", "ts_inside_launch.h", "ts_winding_launch.h", "ts_overlap_launch.h", "ts_subdivide_launch.h", "ts_flip_launch.h", "ts_collapse_launch.h", "ts_collapse_round.h", "ts_decimate_launch.h", "ts_contract_launch.h", "ts_ray_tests.h", "ts_mesh_bary.h", "ts_union_find.h", "ts_mesh_common.h", "ts_mesh_scan.h", "ts_mesh_runs.h", "ts_mesh_edges.h", "ts_mesh_edge_ids.h", "ts2d_lab.h", "ts2d_math.h", "ts2d_wave.h", "ts2d_group.h", "ts2d_support.h", "ts2d_sh.h", "ts2d_stage.h", "ts2d_preprocess_launch.h", "ts2d_imgops.h", "ts2d_select.h", "ts2d_tri.h", os.path.join("..", "..", "include", "ts2d.h"),
           os.path.join("..", "..", "include", "ts_loss.h"),
           os.path.join("..", "..", "include", "ts_knn.h"),
           os.path.join("..", "..", "include", "ts_model.h"),
           os.path.join("..", "..", "include", "ts_optim.h"),
           os.path.join("..", "..", "include", "ts_mesh.h"),
           os.path.join("..", "..", "include", "ts_weld.h"),
           os.path.join("..", "..", "include", "ts_geom.h"),
           os.path.join("..", "..", "include", "ts_bvh.h"),
           os.path.join("..", "..", "include", "ts_ray.h"),
           os.path.join("..", "..", "include", "ts_volume.h"),
           os.path.join("..", "..", "include", "ts_color.h"),
           os.path.join("..", "..", "include", "ts_simplify.h"),
           os.path.join("..", "..", "include", "ts_smooth.h"),
           os.path.join("..", "..", "include", "ts_holes.h"),
           os.path.join("..", "..", "include", "ts_manifold.h"),
           os.path.join("..", "..", "include", "ts_orient.h"),
           os.path.join("..", "..", "include", "ts_atlas.h"),
           os.path.join("..", "..", "include", "ts_inside.h"),
           os.path.join("..", "..", "include", "ts_winding.h"),
           os.path.join("..", "..", "include", "ts_overlap.h"),
           os.path.join("..", "..", "include", "ts_subdivide.h"),
           os.path.join("..", "..", "include", "ts_flip.h"),
           os.path.join("..", "..", "include", "ts_collapse.h"),
           os.path.join("..", "..", "include", "ts_decimate.h"),
           os.path.join("..", "..", "include", "ts_contract.h")]


def hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: libts2d.so cannot be built (no CPU fallback exists by design)")


_TOOLCHAIN_ID = {}


def _toolchain_id(cc: str) -> str:
    if cc not in _TOOLCHAIN_ID:
        r = subprocess.run([cc, "--version"], capture_output=True, text=True)
        _TOOLCHAIN_ID[cc] = hashlib.sha1((r.stdout + r.stderr).encode()).hexdigest()
    return _TOOLCHAIN_ID[cc]


def _newest_header() -> float:
    return max(os.path.getmtime(os.path.join(CSRC, h)) for h in HEADERS)


def _sources(lab: bool) -> dict:
    if not lab:
        return dict(SOURCES)
    sources = {k: v for k, v in SOURCES.items() if k != "api.hip"}  # the product's objects are shared
    sources.update({("lab/" + k): v for k, v in LAB_SOURCES.items()})
    return sources


def _unit(key: str) -> str:
    src, _, part = key.partition("@")  # "file.hip@tag": the same source compiled into file_tag.o with its own flags
    return src[: -len(".hip")] + ("_" + part if part else "")


def units(lab: bool = False) -> list:
    """The translation units build(lab=lab) links, in link order: their objects' paths under build/ without .o."""
    return [_unit(k) for k in _sources(lab)]


def _object(unit: str, variant: str | None = None) -> str:
    return os.path.join(OBJ_DIR if variant is None else os.path.join(VARIANT_DIR, variant), unit + ".o")


def objects(lab: bool = False, variant: str | None = None, extra: dict | None = None) -> list:
    """The objects build(lab=lab, variant=variant, extra=extra) links: a unit with extra flags from the variant's directory, the others the product's."""
    extra = extra or {}
    return [_object(u, variant if extra.get(u) else None) for u in units(lab)]


def library(lab: bool = False, variant: str | None = None) -> str:
    if variant is None:
        return LAB_LIB if lab else LIB
    return os.path.join(BIN_DIR, f"libts2d_lab_{variant}.so" if lab else f"libts2d_{variant}.so")


def command(unit: str, extra=(), variant: str | None = None, cc: str = "hipcc") -> list:
    """The compile command of one unit: COMMON + its SOURCES / LAB_SOURCES entry, then `extra`; with extra flags the object goes to the variant's directory."""
    table = {_unit(k): (k, v) for lab in (False, True) for k, v in _sources(lab).items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units are {', '.join(table)}")
    key, flags = table[unit]
    src = os.path.join(CSRC, os.path.basename(key.partition("@")[0]))
    if not os.path.exists(src):  # a lab-only source
        src = os.path.join(LAB_SRC, os.path.basename(src))
        flags = list(flags) + ["-I" + CSRC]
    return [cc, *COMMON, *flags, *extra, "-c", src, "-o", _object(unit, variant if extra else None)]


def geom_units() -> list:
    """The translation units of libts_geom.so that are its own (GEOM_SOURCES); it links the objects of GEOM_SHARED besides."""
    return [_unit(k) for k in GEOM_SOURCES]


def geom_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of GEOM_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in GEOM_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_geom.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def geom_objects() -> list:
    return [_object(u) for u in geom_units()] + [_object(u) for u in GEOM_SHARED]


def bvh_units() -> list:
    """The translation units of libts_bvh.so that are its own (BVH_SOURCES); it links the objects of BVH_SHARED besides."""
    return [_unit(k) for k in BVH_SOURCES]


def bvh_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of BVH_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in BVH_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_bvh.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def bvh_objects() -> list:
    return [_object(u) for u in bvh_units()] + [_object(u) for u in BVH_SHARED]


def ray_units() -> list:
    """The translation units of libts_ray.so that are its own (RAY_SOURCES); it links the objects of RAY_SHARED besides."""
    return [_unit(k) for k in RAY_SOURCES]


def ray_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of RAY_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in RAY_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_ray.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def ray_objects() -> list:
    return [_object(u) for u in ray_units()] + [_object(u) for u in RAY_SHARED]


def volume_units() -> list:
    """The translation units of libts_volume.so (VOLUME_SOURCES): all of its objects."""
    return [_unit(k) for k in VOLUME_SOURCES]


def volume_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of VOLUME_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in VOLUME_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_volume.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def volume_objects() -> list:
    return [_object(u) for u in volume_units()]


def color_units() -> list:
    """The translation units of libts_color.so (COLOR_SOURCES): all of its objects."""
    return [_unit(k) for k in COLOR_SOURCES]


def color_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of COLOR_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in COLOR_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_color.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def color_objects() -> list:
    return [_object(u) for u in color_units()]


def simplify_units() -> list:
    """The translation units of libts_simplify.so that are its own (SIMPLIFY_SOURCES); it links the objects of SIMPLIFY_SHARED besides."""
    return [_unit(k) for k in SIMPLIFY_SOURCES]


def simplify_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of SIMPLIFY_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in SIMPLIFY_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_simplify.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def simplify_objects() -> list:
    return [_object(u) for u in simplify_units()] + [_object(u) for u in SIMPLIFY_SHARED]


def smooth_units() -> list:
    """The translation units of libts_smooth.so that are its own (SMOOTH_SOURCES); it links the objects of SMOOTH_SHARED besides."""
    return [_unit(k) for k in SMOOTH_SOURCES]


def smooth_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of SMOOTH_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in SMOOTH_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_smooth.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def smooth_objects() -> list:
    return [_object(u) for u in smooth_units()] + [_object(u) for u in SMOOTH_SHARED]


def holes_units() -> list:
    """The translation units of libts_holes.so (HOLES_SOURCES): all of its objects."""
    return [_unit(k) for k in HOLES_SOURCES]


def holes_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of HOLES_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in HOLES_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_holes.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def holes_objects() -> list:
    return [_object(u) for u in holes_units()]


def manifold_units() -> list:
    """The translation units of libts_manifold.so that are its own (MANIFOLD_SOURCES); it links the objects of MANIFOLD_SHARED besides."""
    return [_unit(k) for k in MANIFOLD_SOURCES]


def manifold_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of MANIFOLD_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in MANIFOLD_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_manifold.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def manifold_objects() -> list:
    return [_object(u) for u in manifold_units()] + [_object(u) for u in MANIFOLD_SHARED]


def orient_units() -> list:
    """The translation units of libts_orient.so that are its own (ORIENT_SOURCES); it links the objects of ORIENT_SHARED besides."""
    return [_unit(k) for k in ORIENT_SOURCES]


def orient_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of ORIENT_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in ORIENT_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_orient.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def orient_objects() -> list:
    return [_object(u) for u in orient_units()] + [_object(u) for u in ORIENT_SHARED]


def atlas_units() -> list:
    """The translation units of libts_atlas.so (ATLAS_SOURCES): all of its objects."""
    return [_unit(k) for k in ATLAS_SOURCES]


def atlas_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of ATLAS_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in ATLAS_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_atlas.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def atlas_objects() -> list:
    return [_object(u) for u in atlas_units()]


def inside_units() -> list:
    """The translation units of libts_inside.so that are its own (INSIDE_SOURCES); it links the objects of INSIDE_SHARED besides."""
    return [_unit(k) for k in INSIDE_SOURCES]


def inside_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of INSIDE_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in INSIDE_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_inside.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def inside_objects() -> list:
    return [_object(u) for u in inside_units()] + [_object(u) for u in INSIDE_SHARED]


def winding_units() -> list:
    """The translation units of libts_winding.so that are its own (WINDING_SOURCES); it links the objects of WINDING_SHARED besides."""
    return [_unit(k) for k in WINDING_SOURCES]


def winding_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of WINDING_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in WINDING_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_winding.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def winding_objects() -> list:
    return [_object(u) for u in winding_units()] + [_object(u) for u in WINDING_SHARED]


def overlap_units() -> list:
    """The translation units of libts_overlap.so that are its own (OVERLAP_SOURCES); it links the objects of OVERLAP_SHARED besides."""
    return [_unit(k) for k in OVERLAP_SOURCES]


def overlap_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of OVERLAP_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in OVERLAP_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_overlap.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def overlap_objects() -> list:
    return [_object(u) for u in overlap_units()] + [_object(u) for u in OVERLAP_SHARED]


def subdivide_units() -> list:
    """The translation units of libts_subdivide.so that are its own (SUBDIVIDE_SOURCES); it links the objects of SUBDIVIDE_SHARED besides."""
    return [_unit(k) for k in SUBDIVIDE_SOURCES]


def subdivide_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of SUBDIVIDE_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in SUBDIVIDE_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_subdivide.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def subdivide_objects() -> list:
    return [_object(u) for u in subdivide_units()] + [_object(u) for u in SUBDIVIDE_SHARED]


def flip_units() -> list:
    """The translation units of libts_flip.so that are its own (FLIP_SOURCES); it links the objects of FLIP_SHARED besides."""
    return [_unit(k) for k in FLIP_SOURCES]


def flip_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of FLIP_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in FLIP_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_flip.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def flip_objects() -> list:
    return [_object(u) for u in flip_units()] + [_object(u) for u in FLIP_SHARED]


def collapse_units() -> list:
    """The translation units of libts_collapse.so that are its own (COLLAPSE_SOURCES); it links the objects of COLLAPSE_SHARED besides."""
    return [_unit(k) for k in COLLAPSE_SOURCES]


def collapse_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of COLLAPSE_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in COLLAPSE_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_collapse.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def collapse_objects() -> list:
    return [_object(u) for u in collapse_units()] + [_object(u) for u in COLLAPSE_SHARED]


def decimate_units() -> list:
    """The translation units of libts_decimate.so that are its own (DECIMATE_SOURCES); it links the objects of DECIMATE_SHARED besides."""
    return [_unit(k) for k in DECIMATE_SOURCES]


def decimate_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of DECIMATE_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in DECIMATE_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_decimate.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def decimate_objects() -> list:
    return [_object(u) for u in decimate_units()] + [_object(u) for u in DECIMATE_SHARED]


def contract_units() -> list:
    """The translation units of libts_contract.so that are its own (CONTRACT_SOURCES); it links the objects of CONTRACT_SHARED besides."""
    return [_unit(k) for k in CONTRACT_SOURCES]


def contract_command(unit: str, cc: str = "hipcc") -> list:
    """The compile command of one unit of CONTRACT_SOURCES: COMMON + its flags, like command()."""
    table = {_unit(k): (k, v) for k, v in CONTRACT_SOURCES.items()}
    if unit not in table:
        raise ValueError(f"unknown unit {unit!r}; the units of libts_contract.so are {', '.join(table)}")
    key, flags = table[unit]
    return [cc, *COMMON, *flags, "-c", os.path.join(CSRC, key), "-o", _object(unit)]


def contract_objects() -> list:
    return [_object(u) for u in contract_units()] + [_object(u) for u in CONTRACT_SHARED]


def ext_command(cc: str = "hipcc") -> list:
    """The build command of the torch extension (the reference's ext.cpp signatures plus the package's *_ex entry points over the C ABI)."""
    import sysconfig
    import torch  # include / library directories only
    ti = os.path.dirname(torch.__file__)
    return [cc, "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1", "-DTORCH_EXTENSION_NAME=_ts2d_torch_C",
            f"-I{ti}/include", f"-I{ti}/include/torch/csrc/api/include", f"-I{sysconfig.get_paths()['include']}", "-I/opt/rocm/include", "-w", "-x",
            "c++", EXT_SRC, "-x", "none", f"-L{ti}/lib", "-ltorch", "-ltorch_cpu", "-ltorch_hip", "-lc10", "-lc10_hip", "-ltorch_python", f"-L{OUT_DIR}",
            "-lts2d", "-Wl,-rpath,$ORIGIN/../diff_triangle_rasterization_2D", "-o", EXT]


def _fresh(out: str, key: str, newer_than: float) -> bool:
    # an output is only reused when it was produced by this very command line with this very compiler (its stamp out.cmd holds `key`): a toolchain
    # update must not leave its outputs behind for the next build
    stamp = out + ".cmd"
    return os.path.exists(out) and os.path.exists(stamp) and open(stamp).read() == key and os.path.getmtime(out) >= newer_than


def build(force: bool = False, verbose: bool = False, lab: bool = False, variant: str | None = None, extra: dict | None = None) -> str:
    """Compiles the stale objects and links libts2d.so (lab: and libts2d_lab.so, returned), then builds the torch extension.  variant = TAG:
    tools/bin/libts2d_TAG.so (lab: and libts2d_lab_TAG.so, returned) instead, the units named in extra = {unit: [flags]} compiled with those
    flags appended."""
    extra = {u: list(f) for u, f in (extra or {}).items() if f}
    if variant is None and extra:
        raise ValueError("extra flags need a variant tag")
    if variant is not None and not re.fullmatch(r"[A-Za-z0-9_.+-]+", variant):
        raise ValueError(f"bad variant tag {variant!r}")
    libs = [False, True] if lab else [False]
    known = dict.fromkeys(u for l in libs for u in units(l))
    unknown = [u for u in extra if u not in known]
    if unknown:
        raise ValueError(f"unknown unit(s) {', '.join(unknown)}; the units are {', '.join(known)}" + ("" if lab else " (lab units need --lab)"))
    cc = hipcc()
    tool = _toolchain_id(cc)
    me = os.path.abspath(__file__)
    hdr_t = max(_newest_header(), os.path.getmtime(me))
    jobs = []
    cmds = [command(u, extra.get(u, ()), variant, cc) for u in known]
    if variant is None:  # the other nineteen product libraries: include/ts_geom.h, ts_bvh.h, ts_ray.h, ts_volume.h, ts_color.h, ts_simplify.h, ts_smooth.h, ts_holes.h, ts_manifold.h, ts_orient.h, ts_atlas.h, ts_inside.h, ts_winding.h, ts_overlap.h, ts_subdivide.h, ts_flip.h, ts_collapse.h, ts_decimate.h, ts_contract.h
        cmds += [geom_command(u, cc) for u in geom_units()] + [bvh_command(u, cc) for u in bvh_units()] + [ray_command(u, cc) for u in ray_units()]
        cmds += [volume_command(u, cc) for u in volume_units()] + [color_command(u, cc) for u in color_units()]
        cmds += [simplify_command(u, cc) for u in simplify_units()] + [smooth_command(u, cc) for u in smooth_units()]
        cmds += [holes_command(u, cc) for u in holes_units()] + [manifold_command(u, cc) for u in manifold_units()]
        cmds += [orient_command(u, cc) for u in orient_units()] + [atlas_command(u, cc) for u in atlas_units()]
        cmds += [inside_command(u, cc) for u in inside_units()] + [winding_command(u, cc) for u in winding_units()]
        cmds += [overlap_command(u, cc) for u in overlap_units()] + [subdivide_command(u, cc) for u in subdivide_units()]
        cmds += [flip_command(u, cc) for u in flip_units()] + [collapse_command(u, cc) for u in collapse_units()]
        cmds += [decimate_command(u, cc) for u in decimate_units()] + [contract_command(u, cc) for u in contract_units()]
    for cmd in cmds:
        s, o = cmd[-3], cmd[-1]
        os.makedirs(os.path.dirname(o), exist_ok=True)
        key = tool + "\n" + " ".join(cmd)
        if force or not _fresh(o, key, max(os.path.getmtime(s), hdr_t)):
            jobs.append((o, cmd, key))

    def make(out, cmd, key):
        stamp = out + ".cmd"
        if os.path.exists(stamp):
            os.remove(stamp)
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        if verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)
        with open(stamp, "w") as f:
            f.write(key)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(lambda job: make(*job), jobs))
    compiled = {o for o, _, _ in jobs}
    for l in libs:
        lib, objs = library(l, variant), objects(l, variant, extra)
        cmd = [cc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-Wl,-soname,libts2d.so", "-o", lib, *objs]
        key = tool + "\n" + " ".join(cmd)
        if force or compiled.intersection(objs) or not _fresh(lib, key, max(os.path.getmtime(o) for o in objs)):
            os.makedirs(os.path.dirname(lib), exist_ok=True)
            make(lib, cmd, key)
    for out, soname, objs in ((GEOM_LIB, "libts_geom.so", geom_objects()), (BVH_LIB, "libts_bvh.so", bvh_objects()),
                              (RAY_LIB, "libts_ray.so", ray_objects()), (VOLUME_LIB, "libts_volume.so", volume_objects()),
                              (COLOR_LIB, "libts_color.so", color_objects()),
                              (SIMPLIFY_LIB, "libts_simplify.so", simplify_objects()),
                              (SMOOTH_LIB, "libts_smooth.so", smooth_objects()),
                              (HOLES_LIB, "libts_holes.so", holes_objects()),
                              (MANIFOLD_LIB, "libts_manifold.so", manifold_objects()),
                              (ORIENT_LIB, "libts_orient.so", orient_objects()),
                              (ATLAS_LIB, "libts_atlas.so", atlas_objects()),
                              (INSIDE_LIB, "libts_inside.so", inside_objects()),
                              (WINDING_LIB, "libts_winding.so", winding_objects()),
                              (OVERLAP_LIB, "libts_overlap.so", overlap_objects()),
                              (SUBDIVIDE_LIB, "libts_subdivide.so", subdivide_objects()),
                              (FLIP_LIB, "libts_flip.so", flip_objects()),
                              (COLLAPSE_LIB, "libts_collapse.so", collapse_objects()),
                              (DECIMATE_LIB, "libts_decimate.so", decimate_objects()),
                              (CONTRACT_LIB, "libts_contract.so", contract_objects())) if variant is None else ():
        cmd = [cc, "-shared", "-fPIC", f"--offload-arch={ARCH}", f"-Wl,-soname,{soname}", "-o", out, *objs]
        key = tool + "\n" + " ".join(cmd)
        if force or compiled.intersection(objs) or not _fresh(out, key, max(os.path.getmtime(o) for o in objs)):
            make(out, cmd, key)
    if variant is None:  # the package has no other binding, so a build against another torch must not be reused: torch's version is in the key
        import torch
        cmd = ext_command(cc)
        key = f"{tool}\ntorch {torch.__version__}\n" + " ".join(cmd)
        deps = (EXT_SRC, os.path.join(os.path.dirname(HERE), "include", "ts2d.h"), me)
        if force or not _fresh(EXT, key, max(os.path.getmtime(d) for d in deps)):
            make(EXT, cmd, key)
    return lib


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--lab", action="store_true")
    ap.add_argument("--variant", metavar="TAG")
    ap.add_argument("--all", metavar="FLAGS", default="", help="extra flags for every unit")
    ap.add_argument("--unit", metavar="NAME=FLAGS", action="append", default=[], help="extra flags for one unit")
    # "--all -DX": glued to its option, or argparse would take a value that starts with "-" for an option of its own
    argv, it = [], iter(sys.argv[1:])
    for arg in it:
        argv.append(arg + "=" + next(it, "") if arg in ("--all", "--unit") else arg)
    a = ap.parse_args(argv)
    extra = {u: shlex.split(a.all) for l in ([False, True] if a.lab else [False]) for u in units(l)} if a.all else {}
    for spec in a.unit:
        name, eq, flags = spec.partition("=")
        if not eq:
            ap.error(f"--unit {spec}: expected NAME=FLAGS")
        extra[name] = extra.get(name, []) + shlex.split(flags)
    try:
        print(build(a.force, a.verbose, a.lab, a.variant, extra))
    except ValueError as e:
        ap.error(str(e))
