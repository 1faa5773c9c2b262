"""MI355X-native counterparts of the reference code on either side of the rasterizer:

    losses.py             L1, SSIMLoss / ssimLoss, the fused PhotometricLoss, DepthNormalLoss (the producer of dL_dout_depth / dL_dout_normal), and the
                          two auxiliary image losses DoGLoss / SmoothnessLoss (weight 0 in every shipped configuration; trainer_utils.py:105-201)
                          (reference: src/diff_recon/trainers/trainer_utils.py:9-103, 323-324, 349;
                           combined as in src/diff_recon/trainers/VanillaTS_trainer.py:80-81,111)
    triangle_renderer.py  TriangleRenderer (reference: src/diff_recon/renderer/triangle_renderer.py:15-95)
    model_update.py       DensificationStats (the per-iteration `_training_statistic` as one fused kernel) and the periodic rules
                          prune_points / densification / opacity_pruning / opacity_clipping / scale_pruning / scale_clipping /
                          opacity_reset / contribution_pruning with their Adam-state surgery on native row operators
                          (reference: src/diff_recon/models/VanillaTS_model.py:194-201, 214-345, 347-537)
    schedulers.py         exponential_scheduler / step_scheduler / exponential_step_scheduler, gamma_at, sh_degree_at
                          (reference: src/diff_recon/utils/scheduler.py:5-45, VanillaTS_model.py:548-565; pinned by tests/golden/schedules.npz)
    raw_triangle.py       RawTriangle with loadPLY / savePLY / saveGLB / loadGLB: the on-disk formats of a triangle model, numpy only, and its set
                          operations += / -= / - / reduce / replace (the set difference by centre distance searches on the device)
                          (reference: src/diff_recon/models/raw_triangle.py:12-223)
    optim.py              FusedAdam (the reference's torch.optim.Adam(l, lr=0.0, eps=1e-15) as ONE fused launch, same param_groups / state) and
                          ShardedAdam (reduce-scatter of the gradient bucket -> Adam on the rank's slice -> all-gather of the parameters)
                          (reference: src/diff_recon/models/VanillaTS_model.py:108-124, src/diff_recon/trainers/VanillaTS_trainer.py:119-122)
    model_forward.py      render_view = the argument construction of VanillaTSModel.forward
                          (reference: src/diff_recon/models/VanillaTS_model.py:585-694)
    model_init.py         create_from_pcd (point cloud -> distCUDA2 -> equilateral triangles, back-face twins), grid / random / direct sampling
                          (reference: src/diff_recon/models/VanillaTS_model.py:761-804, 830-917; model_utils.py:34-57, 95-149)
    regularizers.py       triangle_regularization (scaling / opacity / vertex regularisers fused, one pass each way), prepare_nearest, TrainerRegularizers
                          (the regularisation schedule of _get_loss with affine_reg), ColorAffine (the per-view colour affine and its optimizer groups)
                          (reference: src/diff_recon/trainers/VanillaTS_trainer.py:86-116, trainer_utils.py:339-346,
                           src/diff_recon/models/VanillaTS_model.py:72-76, 86-94, 118-121, 146-152, 678-684)
    multirank.py          ImageParallelLoop (image-parallel training end to end: shard the views, exchange gradients and statistics, replicated Adam and
                          structural rules), ReplicaGuard / ReplicaDivergence and state_digest (one-launch 64-bit digests of device state that prove the
                          replicas bit-identical) -- no counterpart in the reference, which has no distributed path
    mesh_renderer.py      MeshRenderer (the opaque z-buffer look at an exported mesh: constructor, `render` signature and results of KaolinRenderer,
                          plus depth and face_idx) and mesh_from_triangles (the mesh saveGLB would write, on the device)
                          (reference: src/diff_recon/renderer/kaolin_renderer.py:8-72, src/diff_recon/models/raw_triangle.py:183-209)
    mesh_census.py        MeshCensus (per-face pixel counts and fixed-point colour sums over the face_idx images of many views, in integers:
                          bit-identical in any view order), bake_face_colors (every face takes the mean of the target pixels it wins) and
                          visible_triangle_mask (multi-view visibility pruning of an exported mesh) -- no counterpart in the reference
    mesh_weld.py          weld_mesh (all vertices within eps of each other merged transitively: renumbered vertices, remapped faces, collapsed
                          faces dropped; a pure function of the input) and mesh_topology (boundary / manifold / non-manifold edges, pieces, Euler
                          characteristic) -- the counterpart of saveGLB(..., process=True)
                          (reference: src/diff_recon/models/raw_triangle.py:183-207, trimesh's vertex merging)
    mesh_distance.py      nearest_points (exact nearest neighbour between two point sets), sample_mesh_surface (deterministic area-weighted
                          surface samples), point_cloud_distance / mesh_distance (accuracy, completeness, Chamfer, Hausdorff, precision / recall /
                          F-score) -- the geometric scores of an exported mesh; the search stands in for scipy's KDTree in RawTriangle's `-=`
                          (reference: src/diff_recon/models/raw_triangle.py:79-87)
    mesh_surface.py       MeshBVH (a bounding-volume hierarchy over the triangles of a mesh; .closest: the exact nearest face, squared distance
                          and closest point of every query, float64), point_to_mesh_distance, mesh_surface_distance (the scores of
                          mesh_distance measured sample to SURFACE: identical surfaces score 0, not the sample spacing)
    mesh_ray.py           ray_cast (the exact first hit of every ray on a MeshBVH: face, t, barycentric weights, side; watertight, equal to brute
                          force bit for bit), camera_rays (the pixel-centre rays of a view; t is MeshRenderer's depth), point_visibility (how many
                          centres see a point past the mesh; behind mesh_surface_distance(visible_from=...)) -- loaded on first use
    volume.py             TSDFVolume (per-view depth fused into a truncated signed distance volume held in integers: bit-identical in any view
                          order, volumes add), extract_isosurface (marching tetrahedra on any fp32 grid: an oriented soup that weld_mesh(eps=0)
                          closes) and fuse_mesh (MeshRenderer depth of many views -> one connected, closed mesh) -- no counterpart in the
                          reference; loaded on first use
    color_volume.py       ColorTSDFVolume (colour fused beside the distances, in integers), sample_grid (trilinear over the samples that have
                          data: the colour of every extracted vertex, a function of its position alone), interpolate_vertex_attributes /
                          render_vertex_colors (vertex colours drawn over MeshRenderer's coverage), fuse_colored_mesh (fuse_mesh with colour)
                          and save_glb_mesh (an indexed, vertex-coloured GLB) -- no counterpart in the reference; loaded on first use
    mesh_simplify.py      simplify_mesh (vertex clustering on a uniform grid with quadric error placement: every vertex stays in its cell, the
                          result is a pure function of the input and bit-equal to a float64 reference; attributes are averaged, duplicate
                          faces swept) and drop_small_pieces (connected pieces below a face count removed) -- the pass behind
                          extract_isosurface / fuse_mesh(simplify_cell=...); no counterpart in the reference; loaded on first use
    mesh_smooth.py        vertex_adjacency (the one-ring of every vertex as CSR, edge use counts, vertex classes), smooth_mesh / smooth_fused
                          (Taubin lambda|mu smoothing in float64, bounded per axis, bit-equal to a float64 reference), face_normals /
                          vertex_normals, mesh_normal_consistency (the score beside Chamfer and F-score) and save_glb_shaded_mesh (a GLB
                          with a NORMAL accessor) -- the pass between extraction and simplify_mesh; no counterpart in the reference;
                          loaded on first use
    mesh_holes.py         boundary_loops (every boundary loop of an indexed mesh, found by pointer doubling, ordered from its smallest
                          half-edge and numbered; pinch vertices open their chains), loop_vertices, fill_holes / fill_fused (a centroid fan
                          over every loop of at most max_loop_edges edges, orientation continued, attributes averaged; bit-equal to a float64
                          reference) -- the pass between extraction and smooth_mesh; no counterpart in the reference, which exports its
                          soup through trimesh; loaded on first use
    mesh_manifold.py      vertex_fans (the fan of every corner: the corners of a vertex joined through edges that exactly two faces use, found by
                          two sorts and a lock-free union-find; fans per vertex, non-manifold and same-direction edge counts),
                          split_nonmanifold / manifold_fused (every extra fan of a vertex gets a vertex of its own: the result is
                          edge-manifold and vertex-manifold, positions and attributes copied bit for bit; bit-equal to a numpy reference)
                          -- the pass between simplify_mesh and fill_holes; no counterpart in the reference; loaded on first use
    mesh_orient.py        orient_faces / orient_fused (every orientable piece of an indexed mesh made to wind one way: the faces linked through
                          edges that exactly two of them use, pieces and flip parities by a lock-free union-find over the doubled graph,
                          non-orientable pieces reported and left alone; the piece faces by its anchor, by majority or by the sign of its
                          quantised volume; bit-equal to a numpy reference) -- the pass between split_nonmanifold and fill_holes; no
                          counterpart in the reference; loaded on first use
    mesh_texture.py       atlas_layout / face_uvs (res x res half-cells, two faces to a cell: every face gets res (res + 1) / 2 texels of its own),
                          texel_index (the texel of every pixel, from interpolate_vertex_attributes' barycentrics), TextureAtlas (a MeshCensus
                          over the texels: bit-identical in any view order, atlases add; resolve falls back texel -> face -> caller -> fill),
                          render_textured, bake_texture, evaluate_textured and save_glb_textured_mesh (a GLB with TEXCOORD_0 and the atlas as
                          an embedded PNG, exact under NEAREST) -- colour resolution that does not depend on the face count; no counterpart
                          in the reference; loaded on first use
    mesh_inside.py        ray_crossings (ALL hits of every ray on a MeshBVH, counted in half crossings so that a ray through a shared edge
                          counts one crossing; equal to brute force bit for bit), winding_number / contains_points / signed_distance (the
                          first clean ray of three fixed directions decides), mesh_to_sdf (the signed distance on a grid: the way back from
                          a mesh to a volume), remesh (its level set: one uniform closed surface, or an offset surface) and mesh_volume_iou
                          -- the counterpart of trimesh's contains / signed_distance; loaded on first use
    mesh_winding.py       generalized_winding_number (the signed solid angle of the mesh seen from a point, over 4 pi, summed on the MeshBVH
                          with one far-field term per node; int64 sums of quantised terms, so a pure function of the input),
                          contains_points_winding / signed_distance_winding / mesh_to_sdf_winding / remesh_winding /
                          mesh_volume_iou_winding: the inside test of OPEN meshes, where a ray count is wrong behind every sheet; also
                          method="winding" of mesh_inside's contains_points, signed_distance and mesh_volume_iou -- the counterpart of
                          libigl's fast winding number; loaded on first use
    mesh_overlap.py       MeshBVH.overlap / self_intersections / mesh_intersections (the overlap query of the MeshBVH: which face pairs of
                          one mesh, or of two, cross, lie in one plane or are duplicates; equal to a float64 brute force bit for bit),
                          intersecting_face_mask, drop_intersecting_faces and self_intersection_report: whether a surface passes through
                          itself after clustering, hole filling or smoothing -- the counterpart of a collision query's face-pair list;
                          loaded on first use
    mesh_subdivide.py     mesh_edges (the unique undirected edges of an indexed mesh with their use counts and float64 lengths, and the edge
                          of every half-edge), split_edges / split_long_edges / subdivide_mesh / split_fused (one new vertex at the midpoint
                          of every marked edge, every face cut into 1 to 4 pieces so that neighbours agree: no T-junction, attributes
                          interpolated, faces traced back to their parents; bit-equal to a numpy reference) and view_edge_limit (the world
                          length of max_pixels pixels in the nearest view, per vertex) -- the pass that makes a mesh FINER where
                          bake_face_colors or vertex colours need resolution; no counterpart in the reference; loaded on first use
    mesh_flip.py          flip_edges / delaunay_flips / nondelaunay_edges / flip_fused (rounds of edge flips toward the Delaunay condition:
                          an interior edge whose two opposite angles sum to more than pi is replaced by the other diagonal of its quad, an
                          independent set per round chosen by integer priorities; no vertex moves, V, E and F stay, creases and folds are
                          guarded; bit-equal to a numpy reference) and triangle_quality -- the pass that improves the SHAPE of the faces
                          that split_edges, fill_holes and extract_isosurface leave; no counterpart in the reference; loaded on first use
    mesh_collapse.py      collapse_edges / short_edges / collapse_short_edges / collapse_fused (rounds of half-edge collapses of short edges:
                          an interior edge shorter than a limit loses one end, which every face around it hands over to the other end, and
                          its two faces; an independent set at distance two per round, shortest first; no vertex moves, boundaries and
                          pinned vertices are held, link, length and normal guards keep the topology, the upper edge bound and the
                          creases; bit-equal to a numpy reference) and isotropic_remesh (split, collapse, flip and smooth, repeated) --
                          the pass that makes a mesh COARSER along its own connectivity and removes the needles that extract_isosurface
                          leaves; no counterpart in the reference; loaded on first use
    mesh_decimate.py      vertex_quadrics / decimate_round / cheapest_edges / decimate_mesh / decimate_fused (decimation to a face budget or
                          an error bound: rounds of the same half-edge collapses ordered by quadric error, the cheapest first, at most a
                          budget of them per round; the quadrics follow the collapses, so the error is measured against the original
                          surface; same classes, guards and independent set as mesh_collapse.py; bit-equal to a numpy reference) -- the
                          pass that answers "this surface in N faces"; no counterpart in the reference; loaded on first use
    mesh_contract.py      contract_round / placed_edges / contract_mesh / contract_fused (the same decimation by edge CONTRACTION:
                          where both ends of an edge are free the survivor moves to the regularised minimum of the edge's quadric,
                          rounded to fp32 first and judged there over the rings of both ends; attributes blend by how far it went;
                          bit-equal to a numpy reference) -- the pass that answers "this surface in N faces" with vertices where the
                          planes say the surface is; no counterpart in the reference; loaded on first use
    metrics.py           psnr, ssim (= 1 - SSIMLoss), evaluate_mesh and evaluate_vertex_colors: PSNR / SSIM of a mesh's opaque render (one
                          colour per face, or per vertex) against each view's gt_image
                          (reference: src/diff_recon/trainers/trainer_utils.py:331-336, VanillaTS_trainer.py:156-190)
    graphed.py            GraphedStep: a whole training step (sync-free forward, loss, backward, optimizer) captured once into a HIP graph and
                          replayed with one launch -- no counterpart in the reference, whose forward reads num_rendered back every step

Native code: libts2d.so (include/ts_loss.h, include/ts_model.h, include/ts_optim.h, include/ts2d.h, include/ts_mesh.h, include/ts_weld.h) and, for
mesh_distance.py, libts_geom.so beside this file (include/ts_geom.h), for mesh_surface.py, libts_bvh.so (include/ts_bvh.h), for mesh_ray.py, libts_ray.so (include/ts_ray.h), for volume.py, libts_volume.so (include/ts_volume.h), for color_volume.py, libts_color.so (include/ts_color.h), for mesh_simplify.py, libts_simplify.so (include/ts_simplify.h), for mesh_smooth.py, libts_smooth.so (include/ts_smooth.h), for mesh_holes.py, libts_holes.so (include/ts_holes.h), for mesh_manifold.py, libts_manifold.so (include/ts_manifold.h), for mesh_orient.py, libts_orient.so (include/ts_orient.h), for mesh_texture.py, libts_atlas.so (include/ts_atlas.h), for mesh_inside.py, libts_inside.so (include/ts_inside.h), for mesh_winding.py, libts_winding.so (include/ts_winding.h), for mesh_overlap.py, libts_overlap.so (include/ts_overlap.h), for mesh_subdivide.py, libts_subdivide.so (include/ts_subdivide.h), for mesh_flip.py, libts_flip.so (include/ts_flip.h), for mesh_collapse.py, libts_collapse.so (include/ts_collapse.h), for mesh_decimate.py, libts_decimate.so (include/ts_decimate.h), for mesh_contract.py, libts_contract.so (include/ts_contract.h).  No CPU / eager fallback anywhere.
"""
from .losses import L1, SSIMLoss, ssimLoss, PhotometricLoss, photometric_loss, DepthNormalLoss, DoGLoss, SmoothnessLoss, dogLoss, smoothnessLoss, downsample_bilinear, downsample_bilinear_many  # noqa: F401
from .triangle_renderer import TriangleRenderer  # noqa: F401
from .model_forward import background_depth, gamma_rescale_ratio, rescale_triangles, ste_opacity, render_view  # noqa: F401
from .model_update import (DensificationStats, prune_points, densification, opacity_pruning, opacity_clipping, scale_pruning,  # noqa: F401
                           scale_clipping, opacity_reset, contribution_pruning, set_gamma, set_sh_degree, run_model_update)
from . import schedulers  # noqa: F401
from .raw_triangle import RawTriangle  # noqa: F401
from .optim import FusedAdam, ShardedAdam, ShFactors  # noqa: F401
from .graphed import GraphedStep  # noqa: F401
from .regularizers import triangle_regularization, prepare_nearest, PreparedNearest, TrainerRegularizers, ColorAffine, AffineReg, affine_reg  # noqa: F401
from .model_init import create_from_pcd, grid_sampling, grid_size_search, get_inside_mask, inter_point_distance, sample_points  # noqa: F401
from .multirank import (ImageParallelLoop, ReplicaGuard, ReplicaDivergence, state_digest, state_digest_reference, digest_segments,  # noqa: F401
                        replicated_state, MAX_DIGEST_SEGMENTS)
from .mesh_renderer import MeshRenderer, mesh_from_triangles  # noqa: F401
from .mesh_census import MeshCensus, bake_face_colors, visible_triangle_mask  # noqa: F401
from .mesh_weld import WeldedMesh, weld_mesh, mesh_topology  # noqa: F401
from .mesh_distance import SurfaceSamples, nearest_points, face_areas, sample_mesh_surface, point_cloud_distance, mesh_distance  # noqa: F401
from .mesh_surface import MeshBVH, point_to_mesh_distance, mesh_surface_distance  # noqa: F401
from .metrics import psnr, ssim, evaluate_mesh, evaluate_vertex_colors  # noqa: F401

_RAY_NAMES = ("RayHits", "ray_cast", "camera_rays", "point_visibility")
_VOLUME_NAMES = ("TSDFVolume", "extract_isosurface", "fuse_mesh")
_COLOR_NAMES = ("ColorTSDFVolume", "ColoredMesh", "sample_grid", "interpolate_vertex_attributes", "render_vertex_colors", "fuse_colored_mesh",
                "save_glb_mesh")
_SIMPLIFY_NAMES = ("SimplifiedMesh", "simplify_mesh", "drop_small_pieces", "simplify_fused", "cluster_labels", "place_clusters", "unique_faces")
_SMOOTH_NAMES = ("MeshAdjacency", "SmoothedMesh", "vertex_adjacency", "smooth_mesh", "face_normals", "vertex_normals", "smooth_fused",
                 "mesh_normal_consistency", "save_glb_shaded_mesh")
_HOLES_NAMES = ("BoundaryLoops", "FilledMesh", "boundary_loops", "loop_vertices", "fill_holes", "fill_fused")
_MANIFOLD_NAMES = ("VertexFans", "ManifoldMesh", "vertex_fans", "split_nonmanifold", "manifold_fused")
_ORIENT_NAMES = ("OrientedMesh", "orient_faces", "orient_fused")
_TEXTURE_NAMES = ("AtlasLayout", "BakedTexture", "TextureAtlas", "atlas_layout", "face_uvs", "texel_index", "render_textured", "bake_texture",
                  "evaluate_textured", "encode_png", "save_glb_textured_mesh")
_INSIDE_NAMES = ("INSIDE_DIRECTIONS", "RayCrossings", "ray_crossings", "winding_number", "contains_points", "signed_distance", "mesh_to_sdf",
                 "remesh", "mesh_volume_iou")
_WINDING_NAMES = ("UNITS_PER_TURN", "winding_moments", "leaf_faces", "generalized_winding_number", "contains_points_winding",
                  "signed_distance_winding", "mesh_to_sdf_winding", "remesh_winding", "mesh_volume_iou_winding", "threshold_units")
_OVERLAP_NAMES = ("KIND_CROSSING", "KIND_COPLANAR", "KIND_DUPLICATE", "MeshOverlap", "CleanedMesh", "self_intersections", "mesh_intersections",
                  "intersecting_face_mask", "drop_intersecting_faces", "self_intersection_report")
_SUBDIVIDE_NAMES = ("MARK_ALL", "MARK_LONGER", "MARK_VERTEX_LIMIT", "MeshEdges", "SplitMesh", "mesh_edges", "split_edges", "split_long_edges",
                    "subdivide_mesh", "view_edge_limit", "split_fused")
_FLIP_NAMES = ("EDGE_STATES", "FlippedMesh", "DelaunayMesh", "flip_edges", "delaunay_flips", "nondelaunay_edges", "triangle_quality", "flip_fused")
_COLLAPSE_NAMES = ("COLLAPSE_STATES", "COLLAPSE_GUARDS", "CollapsedMesh", "CoarsenedMesh", "RemeshedMesh", "collapse_edges", "short_edges",
                   "collapse_short_edges", "collapse_fused", "isotropic_remesh")
_DECIMATE_NAMES = ("DECIMATE_STATES", "DecimatedRound", "DecimatedMesh", "vertex_quadrics", "decimate_round", "cheapest_edges", "decimate_mesh",
                   "decimate_fused")
_CONTRACT_NAMES = ("CONTRACT_STATES", "CONTRACT_GUARDS", "ContractedRound", "ContractedMesh", "contract_round", "placed_edges", "contract_mesh",
                   "contract_fused")


def __getattr__(name):
    # mesh_ray.py and its library (libts_ray.so) are loaded on first use: without that library everything else here, MeshBVH.closest included, still works
    if name in _RAY_NAMES or name == "mesh_ray":
        import importlib
        module = importlib.import_module(".mesh_ray", __name__)
        return module if name == "mesh_ray" else getattr(module, name)
    if name in _VOLUME_NAMES or name == "volume":  # volume.py and libts_volume.so likewise
        import importlib
        module = importlib.import_module(".volume", __name__)
        return module if name == "volume" else getattr(module, name)
    if name in _COLOR_NAMES or name == "color_volume":  # color_volume.py and libts_color.so likewise
        import importlib
        module = importlib.import_module(".color_volume", __name__)
        return module if name == "color_volume" else getattr(module, name)
    if name in _SIMPLIFY_NAMES or name == "mesh_simplify":  # mesh_simplify.py and libts_simplify.so likewise
        import importlib
        module = importlib.import_module(".mesh_simplify", __name__)
        return module if name == "mesh_simplify" else getattr(module, name)
    if name in _SMOOTH_NAMES or name == "mesh_smooth":  # mesh_smooth.py and libts_smooth.so likewise
        import importlib
        module = importlib.import_module(".mesh_smooth", __name__)
        return module if name == "mesh_smooth" else getattr(module, name)
    if name in _HOLES_NAMES or name == "mesh_holes":  # mesh_holes.py and libts_holes.so likewise
        import importlib
        module = importlib.import_module(".mesh_holes", __name__)
        return module if name == "mesh_holes" else getattr(module, name)
    if name in _MANIFOLD_NAMES or name == "mesh_manifold":  # mesh_manifold.py and libts_manifold.so likewise
        import importlib
        module = importlib.import_module(".mesh_manifold", __name__)
        return module if name == "mesh_manifold" else getattr(module, name)
    if name in _ORIENT_NAMES or name == "mesh_orient":  # mesh_orient.py and libts_orient.so likewise
        import importlib
        module = importlib.import_module(".mesh_orient", __name__)
        return module if name == "mesh_orient" else getattr(module, name)
    if name in _TEXTURE_NAMES or name == "mesh_texture":  # mesh_texture.py and libts_atlas.so likewise
        import importlib
        module = importlib.import_module(".mesh_texture", __name__)
        return module if name == "mesh_texture" else getattr(module, name)
    if name in _INSIDE_NAMES or name == "mesh_inside":  # mesh_inside.py and libts_inside.so likewise
        import importlib
        module = importlib.import_module(".mesh_inside", __name__)
        return module if name == "mesh_inside" else getattr(module, name)
    if name in _WINDING_NAMES or name == "mesh_winding":  # mesh_winding.py and libts_winding.so likewise
        import importlib
        module = importlib.import_module(".mesh_winding", __name__)
        return module if name == "mesh_winding" else getattr(module, name)
    if name in _OVERLAP_NAMES or name == "mesh_overlap":  # mesh_overlap.py and libts_overlap.so likewise
        import importlib
        module = importlib.import_module(".mesh_overlap", __name__)
        return module if name == "mesh_overlap" else getattr(module, name)
    if name in _SUBDIVIDE_NAMES or name == "mesh_subdivide":  # mesh_subdivide.py and libts_subdivide.so likewise
        import importlib
        module = importlib.import_module(".mesh_subdivide", __name__)
        return module if name == "mesh_subdivide" else getattr(module, name)
    if name in _FLIP_NAMES or name == "mesh_flip":  # mesh_flip.py and libts_flip.so likewise
        import importlib
        module = importlib.import_module(".mesh_flip", __name__)
        return module if name == "mesh_flip" else getattr(module, name)
    if name in _COLLAPSE_NAMES or name == "mesh_collapse":  # mesh_collapse.py and libts_collapse.so likewise
        import importlib
        module = importlib.import_module(".mesh_collapse", __name__)
        return module if name == "mesh_collapse" else getattr(module, name)
    if name in _DECIMATE_NAMES or name == "mesh_decimate":  # mesh_decimate.py and libts_decimate.so likewise
        import importlib
        module = importlib.import_module(".mesh_decimate", __name__)
        return module if name == "mesh_decimate" else getattr(module, name)
    if name in _CONTRACT_NAMES or name == "mesh_contract":  # mesh_contract.py and libts_contract.so likewise
        import importlib
        module = importlib.import_module(".mesh_contract", __name__)
        return module if name == "mesh_contract" else getattr(module, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
