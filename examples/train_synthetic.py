"""End-to-end training loop on a synthetic multi-view target, using only this repository's drop-in pieces the way the reference's
trainer + model use their own (src/diff_recon/trainers/VanillaTS_trainer.py:60-130, src/diff_recon/models/VanillaTS_model.py:560-694):

    render_view (argument construction of VanillaTSModel.forward)  ->  TriangleRenderer  ->  2D or 3D HIP rasterizer
    photometric_loss (fused L1 + SSIM)  ->  backward through the rasterizer  ->  Adam (diff_recon_hip.FusedAdam: one fused launch)
    model_update(iteration) in the reference's order (:560-575): training statistic, densification, opacity pruning / clipping,
    scale pruning / clipping, contribution pruning, opacity reset, gamma schedule, SH-degree schedule
    -- every structural update through the native row operators of include/ts_model.h (diff_recon_hip/model_update.py).

`views_per_step` views are rendered per optimisation step and their gradients summed, which is what one step of image-parallel
training computes across ranks (BASELINE.json configs[3]: 8 views per step over 8 GPUs; here the views run one after the other
on one GPU).  With --world N the same step runs image-parallel instead: N processes, each rendering views_per_step / N of the step's views,
gradients and statistics exchanged, the model replicated (diff_recon_hip.ImageParallelLoop), and a ReplicaGuard that proves every
--check-every iterations, and after every structural update, that the replicas still hold the same bits.

A "ground truth" is rendered from a hidden set of triangles from several cameras; a perturbed, sparser copy is optimised.
    python examples/train_synthetic.py [--rasterizer 2D|3D] [--iters 400] [--triangles 20000] [--views 4]
    python examples/train_synthetic.py --world 2 [--exchange dense|factored_sh] [--check-every 50]
    python examples/train_synthetic.py --eval-mesh      after training, score the OPAQUE mesh of the model (what saveGLB would export, rendered
                                                        by diff_recon_hip.MeshRenderer) on the training views: PSNR / SSIM per view and their means
    python examples/train_synthetic.py --eval-mesh --refine-mesh
                                                        then census that mesh over the same views (diff_recon_hip.MeshCensus), drop the triangles
                                                        that win no pixel, bake every face's colour from the pixels it wins, and score it again
    python examples/train_synthetic.py --eval-mesh --weld-mesh EPS
                                                        then weld the front faces of that mesh (diff_recon_hip.weld_mesh), print V -> V', the faces
                                                        dropped, the topology and the largest cluster, and score the welded mesh beside the soup
    python examples/train_synthetic.py --eval-mesh --weld-mesh EPS --split-edges L
                                                        then split the welded mesh until no edge is longer than L (diff_recon_hip.split_fused), start
                                                        the pieces from their parents' colours, bake the face colours again (bake_face_colors) and
                                                        print the face count and PSNR / SSIM before and after
    python examples/train_synthetic.py --eval-mesh (--weld-mesh EPS | --extract-mesh RES [--remesh RES]) --decimate-faces N
                                                        decimate the mesh behind the other steps to N faces by quadric-error collapses
                                                        (diff_recon_hip.decimate_fused / decimate_mesh) and print faces before and after, rounds,
                                                        whether N was reached and triangle quality; the welded mesh's face colours are baked again;
                                                        --decimate-placement optimal contracts edges instead and moves every survivor to the
                                                        quadric's minimum (diff_recon_hip.contract_fused / contract_mesh)
    python examples/train_synthetic.py --eval-mesh --weld-mesh EPS [--split-edges L] [--flip-edges] --collapse-edges L
                                                        collapse the edges shorter than L behind the other steps (diff_recon_hip.collapse_fused),
                                                        bake the face colours again and print rounds, collapses, vertices and faces, triangle
                                                        quality and PSNR / SSIM beside the mesh before
    python examples/train_synthetic.py --eval-mesh --weld-mesh EPS --split-edges L --flip-edges
                                                        then flip the edges of the split mesh toward the Delaunay condition
                                                        (diff_recon_hip.flip_fused), bake the face colours again and print rounds, flips, the
                                                        smallest and median triangle quality before and after, and PSNR / SSIM beside the unflipped
    python examples/train_synthetic.py --eval-mesh --eval-geometry N
                                                        then compare N surface samples of the model's front faces with N of the hidden target
                                                        triangles (diff_recon_hip.mesh_distance): accuracy, completeness, Chamfer, F-score
    python examples/train_synthetic.py --eval-mesh --eval-surface N
                                                        the same scores measured sample to SURFACE (diff_recon_hip.mesh_surface_distance): N samples
                                                        of each mesh against the triangles of the other, free of the sampling spacing
    python examples/train_synthetic.py --eval-mesh --extract-mesh RES
                                                        fuse the training views' depth of that mesh into a TSDF volume of RES samples a side and
                                                        extract one closed surface (diff_recon_hip.fuse_mesh); prints the topology of the soup
                                                        against the fused mesh's and the surface distance between the two and to the target
    python examples/train_synthetic.py --eval-mesh --extract-mesh RES --extract-color
                                                        fuse the training targets' colour in the same volume (diff_recon_hip.fuse_colored_mesh) and
                                                        print the PSNR / SSIM of the vertex-coloured fused mesh beside the soup's own
    python examples/train_synthetic.py --eval-mesh --extract-mesh RES --bake-texture R [--out PATH]
                                                        bake a texture atlas of R texels per face edge for the fused mesh from the training targets
                                                        (diff_recon_hip.bake_texture) and print the PSNR / SSIM of the textured fused mesh beside the
                                                        vertex-coloured one; with --out, write it as a GLB with the atlas as an embedded PNG
    python examples/train_synthetic.py --eval-mesh --extract-mesh RES [--fill-holes N ...] --remesh RES2
                                                        turn the finished fused mesh into a signed distance volume of RES2 samples along its longest
                                                        side (crossing counts on the mesh's own index decide the sign) and extract it again
                                                        (diff_recon_hip.remesh); print its faces, pieces, boundary edges, Euler characteristic, the
                                                        undecided samples and the surface distance to the mesh it came from.  The sign means
                                                        something on a closed mesh: an open sheet shadows what lies behind it.  With
                                                        --remesh-method winding the generalised winding number decides the sign instead
                                                        (diff_recon_hip.remesh_winding), which holds for a mesh with holes too
    python examples/train_synthetic.py --eval-mesh [--weld-mesh EPS] [--extract-mesh RES [...] [--remesh RES2]] --check-intersections
                                                        print, for every indexed mesh produced (welded, the finished fused one, remeshed), how many
                                                        face pairs cross, lie in one plane or are duplicates and how many faces take part in a
                                                        crossing (diff_recon_hip.self_intersection_report: the overlap query of the mesh's own index)
    python examples/train_synthetic.py --eval-mesh --extract-mesh RES --fill-holes N
                                                        close the boundary loops of the fused mesh of at most N edges with centroid fans before anything
                                                        smooths or simplifies it (diff_recon_hip.fill_fused); prints the loops, the filled ones, the open
                                                        half-edges and boundary edges / pieces / Euler characteristic before -> after
    python examples/train_synthetic.py --eval-mesh --extract-mesh RES --smooth-mesh N
                                                        smooth the fused mesh with N Taubin iterations before anything simplifies it, every vertex within
                                                        one voxel of its level set (diff_recon_hip.smooth_fused); prints its largest displacement in
                                                        voxels, its surface distance and normal consistency to the soup, and its topology (unchanged)
    python examples/train_synthetic.py --eval-mesh --extract-mesh RES --simplify-mesh K [--min-piece N]
                                                        simplify the fused mesh by vertex clustering in cells of K voxels with quadric placement
                                                        (diff_recon_hip.simplify_mesh) and drop the pieces below N faces (drop_small_pieces);
                                                        prints the simplified mesh's faces, topology and surface distance to the soup, and with
                                                        --extract-color its PSNR / SSIM
    python examples/train_synthetic.py --eval-mesh --extract-mesh RES [--simplify-mesh K] [--fill-holes N] --split-nonmanifold
                                                        give every extra fan of a vertex a vertex of its own (diff_recon_hip.manifold_fused), after
                                                        --simplify-mesh / --min-piece and before --fill-holes (which then closes the simplified, split
                                                        mesh); prints the fans, the split and new vertices, the non-manifold edges before -> after
                                                        and the same-direction edges
    python examples/train_synthetic.py --eval-mesh {--extract-mesh RES [--split-nonmanifold] [--fill-holes N] | --weld-mesh EPS} --orient-faces {anchor,majority,volume}
                                                        make every orientable piece of the mesh wind one way (diff_recon_hip.orient_fused): after
                                                        --split-nonmanifold and before --fill-holes, or on the welded mesh; prints the pieces, the
                                                        non-orientable ones, the same-direction edges before -> after and the faces flipped
    python examples/train_synthetic.py --eval-mesh --eval-surface N --eval-visible
                                                        those scores over the OBSERVED samples only: the ones that a training camera's centre sees
                                                        past their own mesh (ray casts, diff_recon_hip.point_visibility); prints the hidden counts
"""
import argparse
import math
import os
import sys
import time
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "triangle-splatting_amd")]

import numpy as np
import torch

import synthetic
import diff_recon_hip as D
from diff_recon_hip import DensificationStats, DepthNormalLoss, photometric_loss, render_view
from diff_triangle_rasterization_2D.parallel import ShGradSink, factored_sh_grads


class Camera:
    """The attributes of the reference's Camera that the renderer reads (src/diff_recon/utils/camera.py:70-117)."""

    def __init__(self, s, device, shift=(0.0, 0.0, 0.0)):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        view = s["viewmatrix"].copy()
        sh = np.asarray(shift, np.float32)
        view[3, :3] -= sh * np.array([-1, 1, -1], np.float32)  # translate the camera centre by `shift`
        proj = (view @ synthetic.projection_matrix(s["tanfovx"], s["tanfovy"]).T).astype(np.float32)
        self.image_width, self.image_height = s["image_width"], s["image_height"]
        self.tan_fovx, self.tan_fovy = s["tanfovx"], s["tanfovy"]
        self.world_view_transform, self.full_proj_transform = t(view), t(proj)
        self.camera_center = t(np.array([0, 0, synthetic.CAM_DIST], np.float32) + sh)
        self.device = device


from diff_recon_hip.schedulers import exponential_scheduler  # noqa: E402  (mirror of src/diff_recon/utils/scheduler.py)


class SyntheticModel(DensificationStats):
    """The state VanillaTSModel carries through training, under the reference's attribute names: four per-triangle parameters in
    named Adam groups (:119-135), the six statistics arrays (:196-201, inherited), gamma / active_sh_degree and the schedulers of
    _setup_model_update_utils (:150-194)."""

    def __init__(self, vertex, f_dc, f_rest, raw_opacity, iters, max_sh_degree, single_sh=False):
        super().__init__(vertex.shape[0], vertex.device)
        self._vertex, self._opacity = torch.nn.Parameter(vertex), torch.nn.Parameter(raw_opacity)
        groups = [{"params": [self._vertex], "lr": 0.03, "name": "vertex"}, {"params": [self._opacity], "lr": 0.05, "name": "opacity"}]
        if single_sh:
            # ONE (P, M, 3) colour tensor with the two learning rates of the reference's f_dc / f_rest groups inside it (FusedAdam: lr for the
            # first 3 floats of every triangle's 3 M, lr_tail for the rest): no torch.cat per forward, no split of its gradient per backward
            self._shs = torch.nn.Parameter(torch.cat([f_dc, f_rest], 1).contiguous())
            M = self._shs.shape[1]
            groups.append({"params": [self._shs], "lr": 0.01, "lr_tail": 0.0005, "tail_period": 3 * M, "tail_split": 3, "name": "shs"})
        else:
            self._f_dc, self._f_rest = torch.nn.Parameter(f_dc), torch.nn.Parameter(f_rest)
            groups += [{"params": [self._f_dc], "lr": 0.01, "name": "f_dc"}, {"params": [self._f_rest], "lr": 0.0005, "name": "f_rest"}]
        self.single_sh = single_sh
        # the reference's torch.optim.Adam(l, lr=0.0, eps=1e-15) (VanillaTS_model.py:108-124) as one fused launch per step (include/ts_optim.h)
        self.optimizer = D.FusedAdam(groups, lr=0.0, eps=1e-15)
        self.max_sh_degree, self.active_sh_degree, self.gamma = max_sh_degree, 0, 1.0
        self.scene_bbox, self.ste_threshold = None, None
        q = max(iters // 4, 1)
        every = lambda a, b, k, **kw: NS(start_iter=a, end_iter=b, hold_iter=b, interval_iter=k, **kw)
        self.config = NS(model_update=NS(
            statistic=NS(start_iter=0, end_iter=iters),  # the window in which _training_statistic accumulates (VanillaTS_model.py:348-350)
            densification=every(q // 2, 3 * q, max(q // 3, 1), min_view_count=8, split_num=2, split_scale_threshold=60.0),
            opacity_pruning=every(q, iters, max(q // 2, 1)), opacity_clipping=every(q, iters, max(q // 2, 1)),
            scale_pruning=every(q, iters, q, radii_threshold=200.0, scale_threshold=200.0), scale_clipping=every(q, iters, max(q // 2, 1)),
            contribution_pruning=every(2 * q, iters, q, min_view_count=8, target_point_num=int(0.8 * vertex.shape[0]), prune_ratio=0.3,
                                       max_prune_ratio=0.3, contrib_max_ratio=0.5, sparsity_retain_ratio=0.2, downsample_iteration=[],
                                       downsample_point_num=[]),
            opacity_reset=every(2 * q, 2 * q + 1, 2 * q + 1, reset_value=0.7),
            gamma_schedule=NS(start_iter=q, end_iter=iters), sh_schedule=NS(one_up_iters=[q, 2 * q, 3 * q])))
        self.grad_threshold_scheduler = exponential_scheduler(1.2e-5, 8e-6, 3 * q)
        self.opacity_pruning_scheduler = exponential_scheduler(0.02, 0.05, iters - q)
        self.opacity_clipping_scheduler = exponential_scheduler(0.999, 0.99, iters - q)
        self.scale_max_scheduler = exponential_scheduler(120.0, 100.0, iters - q)  # world units: the scene's mean side is ~55
        self.gamma_scheduler = exponential_scheduler(1.0, 4.0, iters - q)  # the reference's configs go 1 -> 50 over 30 k iterations
        self.log = []

    def model_update(self, iteration, render_pkgs, **kw):
        """VanillaTSModel.model_update (:567-581), same order (diff_recon_hip.model_update.run_model_update).  Returns the rules that fired."""
        fired = D.run_model_update(self, iteration, render_pkgs, **kw)
        for name, res in fired:
            self.log.append((iteration, name, res, self._vertex.shape[0]))
        return fired


def _setup(rasterizer, iters, triangles, width, height, seed, views, w_geometry, single_sh, init_from_pcd):
    """Scene, cameras, hidden targets and the model to optimise, on the current HIP device: the same numbers in every process that calls it with
    the same arguments (every draw comes from a seeded generator), which is what makes the ranks of --world N start as replicas."""
    dev = torch.device("cuda")
    geometry_loss = DepthNormalLoss(scale_factor=0.5) if w_geometry > 0 else None
    g_start_iter = iters // 2  # the reference's configs start it at half of the schedule (15 000 of 30 000)
    D_sh = 2
    s = synthetic.scene(triangles, width, height, D_sh, seed=seed, edge_px=10.0)
    cams = [Camera(s, dev, (6.0 * v, -3.0 * v, 0.0)) for v in range(views)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    bg = torch.zeros(3)
    kw = dict(bg_color=bg, max_sh_degree=D_sh, rasterizer_type=rasterizer)
    with torch.no_grad():  # hidden targets
        gts = [render_view(c, t(s["vertex"]), t(s["shs"][:, :1]), t(s["shs"][:, 1:]), torch.logit(t(s["opacity"]).clamp(0.05, 0.95)), is_training=False,
                           gamma=1.0, active_sh_degree=D_sh, **kw)["render"].clamp(0, 1) for c in cams]
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    keep = torch.rand(triangles, device=dev, generator=g) < 0.7  # start sparser than the target: densification has work to do
    vertex = (t(s["vertex"]) + 1.5 * torch.randn(s["vertex"].shape, device=dev, generator=g))[keep].contiguous()
    n0 = vertex.shape[0]
    if init_from_pcd:
        # the way the reference's trainer starts (VanillaTSModel.create_from_pcd, VanillaTS_model.py:830-917): a point cloud -- here the perturbed
        # centroids with grey colours and no normals, like a COLMAP cloud without them -- becomes equilateral triangles sized by the distance to the
        # three nearest neighbours (simple_knn.distCUDA2)
        init = D.create_from_pcd(vertex.mean(dim=1), torch.full((n0, 3), 0.5, device=dev), None, max_sh_degree=D_sh, init_opacity=0.5)
        m = SyntheticModel(init["_vertex"], init["_f_dc"], init["_f_rest"], init["_opacity"], iters, D_sh, single_sh=single_sh)
    else:
        m = SyntheticModel(vertex, torch.full((n0, 1, 3), 0.5, device=dev), torch.zeros((n0, (D_sh + 1) ** 2 - 1, 3), device=dev),
                           torch.zeros((n0, 1), device=dev), iters, D_sh, single_sh=single_sh)
    return dev, m, cams, gts, kw, geometry_loss, g_start_iter


def train(rasterizer="2D", iters=200, triangles=20000, width=256, height=192, seed=0, views=2, views_per_step=2, log=print, updates=True,
          w_geometry=0.0, single_sh=False, init_from_pcd=False, factored_sh=False, world=None, exchange="dense", check_every=50, on_iteration=None,
          collect=False):
    """w_geometry > 0 adds the depth / normal consistency term of the *_VanillaTS_mesh.yaml configurations (geometry_loss: w_geometry 0.05,
    scale_factor 0.5, from iteration start_iter on; VanillaTS_trainer.py:30-31,64-65,84,111) -- the producer of dL_dout_depth / dL_dout_normal.
    factored_sh: the backward passes hand the optimizer (dL_dRGB, camera centre) per view instead of writing the dense dL_dshs, and FusedAdam
    steps the colour parameters from those (include/ts_optim.h: tso_adam_step_sh_factored) -- the same numbers, 12 M bytes per triangle less
    written and as many less read.
    world = N: image-parallel over N fresh processes (train_ranks below; exchange, check_every, on_iteration and collect belong to it).  The
    default, None, is the one-process loop."""
    if world is not None:
        cfg = dict(rasterizer=rasterizer, iters=iters, triangles=triangles, width=width, height=height, seed=seed, views=views,
                   views_per_step=views_per_step, updates=updates, w_geometry=w_geometry, single_sh=single_sh, init_from_pcd=init_from_pcd)
        return train_ranks(world, cfg, exchange=exchange, check_every=check_every, on_iteration=on_iteration, collect=collect, log=log)
    dev, m, cams, gts, kw, geometry_loss, g_start_iter = _setup(rasterizer, iters, triangles, width, height, seed, views, w_geometry, single_sh,
                                                                init_from_pcd)
    losses, t0 = [], time.perf_counter()
    for it in range(1, iters + 1):
        m.optimizer.zero_grad(set_to_none=True)
        pkgs, total = [], torch.zeros((), device=dev)  # the loss stays on the device: no host synchronisation inside an iteration
        sink = ShGradSink()
        for k in range(views_per_step):  # the views of one step: gradients are summed, like ranks' gradients in image-parallel training
            v = (it * views_per_step + k) % views
            colour = dict(shs=m._shs) if m.single_sh else {}
            pkg = render_view(cams[v], m._vertex, None if m.single_sh else m._f_dc, None if m.single_sh else m._f_rest, m._opacity, is_training=True,
                              gamma=m.gamma, active_sh_degree=m.active_sh_degree, **colour, **kw)
            loss = photometric_loss(pkg["render"], gts[v], 0.8, 0.2)  # w_L1 = 1 - w_ssim, VanillaTS_trainer.py:72,111
            if geometry_loss is not None and it > g_start_iter:
                loss = loss + w_geometry * geometry_loss(pkg["depth"], pkg["normal"], cams[v].tan_fovx, cams[v].tan_fovy)
            with factored_sh_grads(sink, enabled=factored_sh):
                loss.backward()
            pkgs.append(pkg)
            total += loss.detach()
        if factored_sh:
            colour = dict(shs=m._shs) if m.single_sh else dict(f_dc=m._f_dc, f_rest=m._f_rest)
            m.optimizer.step(sh_factors=D.ShFactors(sink, m._vertex, m.active_sh_degree, **colour))
        else:
            m.optimizer.step()
        if updates:
            m.model_update(it, pkgs)
        else:
            for pkg in pkgs:
                m.update(pkg)
        losses.append(total / views_per_step)
        if log and (it % 50 == 0 or it == 1 or it == iters):
            log(f"iter {it:4d}  loss {float(losses[-1]):.5f}  triangles {m._vertex.shape[0]}  gamma {m.gamma:.2f}  sh {m.active_sh_degree}")
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / iters
    return [float(x) for x in torch.stack(losses).cpu()], m, sec


def mesh_scores(m, rasterizer="2D", iters=200, triangles=20000, width=256, height=192, seed=0, views=2, refine=False, weld=None, geometry=None, surface=None,
                visible=False, extract=None, extract_color=False, simplify=None, min_piece=0, smooth=None, fill=None, split=False, orient=None, texture=None,
                out=None, remesh=None, remesh_method="rays", check_intersections=False, split_edges=None, flip_edges=False, collapse_edges=None, decimate_faces=None, decimate_placement="vertex"):
    """PSNR / SSIM of the model's opaque mesh -- mesh_from_triangles: one colour per face from the DC coefficients, back faces as reversed
    twins, the soup saveGLB writes -- against the hidden targets of train() called with the same arguments (diff_recon_hip.evaluate_mesh).
    refine: the result also holds "refined", the same scores (plus "kept" and "triangles") of the mesh after a census over these views
    (diff_recon_hip.MeshCensus): the triangles that win no pixel from any view dropped (visible_triangle_mask), every remaining triangle
    coloured with the mean of the target pixels it wins (bake_face_colors).  The views are the training views: a fit, not a generalisation.
    weld = EPS: the result also holds "welded": the front faces of the mesh scored last (the refined one with `refine`) welded with
    diff_recon_hip.weld_mesh(eps=EPS) -- its scores, the weld's "stats", the "topology" of the welded front faces and "soup", the scores of the
    mesh it was welded from.  The renderer culls nothing, so the front faces alone draw what the soup with its back twins draws.
    geometry = N: the result also holds "geometry": diff_recon_hip.mesh_distance between N surface samples of the model's front faces and N of
    the hidden target triangles (the scene of train() called with the same arguments) -- accuracy, completeness, Chamfer and the F-score at
    0.5, 1 and 2 times the target's median edge length ("median_edge").
    surface = N: the result also holds "surface": the same dictionary from diff_recon_hip.mesh_surface_distance, every sample measured against
    the other mesh's TRIANGLES instead of its samples.
    visible (with surface): only the samples that at least one training camera's centre sees past their own mesh are scored
    (mesh_surface_distance(visible_from=...), ray casts on the mesh's own index); "a_hidden" / "b_hidden" count the samples left out.
    extract = RES: the result also holds "fused": diff_recon_hip.fuse_mesh of the front faces over these views at resolution RES -- the
    "topology" of the fused mesh and of the "soup" (the front faces welded with eps = 0), "to_soup" = mesh_surface_distance between the two and
    "to_target" = the same against the hidden target triangles (None for a fused mesh without faces).
    extract_color (with extract): the views' targets are fused as colour in the same volume (diff_recon_hip.fuse_colored_mesh; the mesh is the
    same) and "fused" also holds "color": diff_recon_hip.evaluate_vertex_colors of the vertex-coloured fused mesh on these views, "vertices"
    and "coloured", the number of vertices that found a colour.
    texture = R (with extract): "fused" also holds "texture": diff_recon_hip.evaluate_textured of the fused mesh with an atlas of R texels per face
    edge baked from these views' targets (diff_recon_hip.bake_texture), the atlas' "width" and "height", "texels" and "observed", the texels that
    a pixel of some view fell into; the others take their face's mean.  out (with texture): the path of the GLB that save_glb_textured_mesh writes.
    simplify = K and / or min_piece = N (with extract): "fused" also holds "simplified": the fused mesh after diff_recon_hip.simplify_mesh on the
    volume's grid in cells of K voxels and drop_small_pieces(N) (diff_recon_hip.simplify_fused) -- its "topology", "to_soup", the "stats" of the two steps and, with
    extract_color, "color" (the vertex colours averaged per cluster).
    smooth = N (with extract): the fused mesh is smoothed with N Taubin iterations, every vertex kept within one voxel of its level set
    (diff_recon_hip.smooth_fused), BEFORE it is simplified, and "fused" also holds "smoothed": "iterations", "moved", "max_displacement_voxels", its
    "topology", "to_soup" and "normals" = diff_recon_hip.mesh_normal_consistency to the soup, with "normals_before", the same of the mesh as fused.
    fill = N (with extract): the boundary loops of the fused mesh of at most N edges are closed with centroid fans (diff_recon_hip.fill_fused)
    BEFORE it is smoothed or simplified, and "fused" also holds "filled": fill_holes' stats and the "topology" of the filled mesh; "topology",
    "to_soup" and "to_target" stay those of the mesh as fused.
    split (with extract): every extra fan of a vertex gets a vertex of its own (diff_recon_hip.manifold_fused), on the simplified mesh when
    simplify / min_piece is given and on the fused mesh otherwise, and "fused" also holds "manifold": split_nonmanifold's stats, the "topology"
    of the split mesh and "before", the topology of the mesh it split.  It runs BEFORE the fill: with simplify / min_piece the fill moves behind
    the split, onto the simplified mesh, and "filled" then holds its own "before".
    orient = "anchor" / "majority" / "volume": the faces of every orientable piece are made to wind one way (diff_recon_hip.orient_fused).  With
    extract it runs where the fill runs, behind the split and before the fill, and "fused" also holds "oriented": orient_faces' stats; with weld
    it runs on the welded mesh and "welded" also holds "oriented".  No other entry changes.
    remesh = RES (with extract): the finished fused mesh, behind every step above, is turned into a signed distance volume of RES samples along
    its longest side and extracted again (diff_recon_hip.remesh: crossing counts on the mesh's own index decide the sign), and "fused" also holds
    "remeshed": the grid's "dims", "voxel_size", "samples", "undecided" and "inside", the "topology" of the new mesh and "to_fused" =
    mesh_surface_distance to the mesh it came from (None for a fused mesh without faces).  remesh_method = "winding": the generalised
    winding number decides the sign instead (diff_recon_hip.remesh_winding), which also holds for a fused mesh with holes; "remeshed" then
    also holds "method".
    check_intersections: every indexed mesh above -- "welded", "fused" (the finished fused mesh, behind every step asked for) and
    "fused"["remeshed"] -- also holds "intersections": diff_recon_hip.self_intersection_report of it, whether the surface passes through
    itself.  No other entry changes.
    split_edges = L (with weld): "welded" also holds "split": the welded mesh split until no edge exceeds L (diff_recon_hip.split_fused), its
    face colours started from faces_color[face_parent] and baked again from these views (bake_face_colors) -- its scores, "faces", "vertices",
    "rounds", "converged" and "before": the scores and "faces" of the welded mesh with ITS face colours baked the same way, so that the two
    differ in resolution alone.  No other entry changes.
    flip_edges (with split_edges): "split" also holds "flipped": the split mesh after diff_recon_hip.flip_fused, baked the same way -- its
    scores, "rounds", "flips", "guarded", "converged", "slots" (the face slots rewritten) and "quality" / "quality_before": the smallest and
    the median diff_recon_hip.triangle_quality.  No other entry changes.
    decimate_faces = N: with weld, "welded" also holds "decimated": the mesh behind the other steps (the collapse included) decimated to N faces
    by quadric-error collapses (diff_recon_hip.decimate_fused), baked again -- its scores, "faces", "vertices", "rounds", "collapses",
    "reached", "quality" / "quality_before" and "before".  A welded soup has only boundary edges: nothing collapses there and "reached" is
    False.  With extract, "fused" also holds "decimated": the same of the finished fused mesh (the remeshed one with remesh; "of" says which)
    through diff_recon_hip.decimate_mesh, with "to_source" = mesh_surface_distance to the mesh it came from instead of image scores (None for
    a mesh without faces).  decimate_placement = "optimal": the same through diff_recon_hip.contract_fused / contract_mesh, the survivors placed at
    the quadric's minimum; the entry then also holds "placement": "optimal".  No other entry changes."""
    _, _, cams, gts, kw, _, _ = _setup(rasterizer, iters, triangles, width, height, seed, views, 0.0, False, False)
    for cam, gt in zip(cams, gts):
        cam.gt_image = gt
    shs = m._shs if m.single_sh else m._f_dc
    res = D.evaluate_mesh(cams, *D.mesh_from_triangles(m._vertex, shs), bg_color=kw["bg_color"])
    if refine:
        keep = D.visible_triangle_mask(cams, m._vertex, shs)
        vertices, faces, color = D.mesh_from_triangles(m._vertex[keep], shs[keep])
        color = D.bake_face_colors(cams, vertices, faces, color, twin_period=int(keep.sum()))
        res["refined"] = dict(D.evaluate_mesh(cams, vertices, faces, color, bg_color=kw["bg_color"]), kept=int(keep.sum()), triangles=int(keep.numel()))
    if weld is not None:
        soup = res["refined"] if refine else res
        if not refine:
            vertices, faces, color = D.mesh_from_triangles(m._vertex, shs)
        front = faces.shape[0] // 2  # mesh_from_triangles: the back twins follow the front faces
        w = D.weld_mesh(vertices, faces[:front], color[:front], eps=weld)
        res["welded"] = dict(D.evaluate_mesh(cams, w.vertices, w.faces, w.faces_color, bg_color=kw["bg_color"]), stats=w.stats,
                             topology=D.mesh_topology(w.stats["num_vertices"], w.faces), eps=float(weld),
                             soup={k: soup[k] for k in ("mean_psnr", "mean_ssim")})
        if orient is not None:
            res["welded"]["oriented"] = D.orient_fused(w, orient).stats["orient"]
        if check_intersections:
            res["welded"]["intersections"] = D.self_intersection_report((w.vertices, w.faces))
        score = lambda mesh: D.evaluate_mesh(cams, mesh.vertices, mesh.faces, D.bake_face_colors(cams, mesh.vertices, mesh.faces, mesh.faces_color),
                                             bg_color=kw["bg_color"])

        def quality(mesh):  # [smallest, median]; a face that takes no part counts as degenerate
            q = D.triangle_quality(mesh.vertices, mesh.faces).nan_to_num(0.0)
            return [float(q.min()), float(q.median())]
        last = w  # the mesh behind the steps so far
        if split_edges is not None:
            fine = last = D.split_fused(w, split_edges)
            res["welded"]["split"] = dict(score(fine), max_edge=float(split_edges), faces=int(fine.faces.shape[0]), vertices=int(fine.vertices.shape[0]),
                                          rounds=fine.stats["split"]["rounds"], converged=fine.stats["split"]["converged"],
                                          before=dict(score(w), faces=int(w.faces.shape[0])))
            if flip_edges:
                flat = last = D.flip_fused(fine)
                t = flat.stats["flip"]
                res["welded"]["split"]["flipped"] = dict(score(flat), rounds=t["rounds"], flips=t["flipped"], guarded=t["guarded"],
                                                         converged=t["converged"], slots=int(t["face_flipped"].sum()),
                                                         quality=quality(flat), quality_before=quality(fine))
        if collapse_edges is not None:
            coarse = D.collapse_fused(last, collapse_edges)
            t = coarse.stats["collapse"]
            res["welded"]["collapsed"] = dict(score(coarse), min_edge=float(collapse_edges), rounds=t["rounds"], collapses=t["collapsed"],
                                              guarded=t["guarded"], converged=t["converged"], faces=int(coarse.faces.shape[0]),
                                              vertices=int(coarse.vertices.shape[0]), quality=quality(coarse), quality_before=quality(last),
                                              before=dict(score(last), faces=int(last.faces.shape[0]), vertices=int(last.vertices.shape[0])))
            last = coarse
        if decimate_faces is not None:
            if decimate_placement == "optimal":  # edge contraction: the survivors move to the quadric's minimum (diff_recon_hip.contract_fused)
                small = D.contract_fused(last, target_faces=int(decimate_faces))
                t = small.stats["contract"]
            else:
                small = D.decimate_fused(last, target_faces=int(decimate_faces))
                t = small.stats["decimate"]
            res["welded"]["decimated"] = dict(score(small), target_faces=int(decimate_faces), rounds=t["rounds"], collapses=t["collapsed"],
                                              reached=t["reached"], faces=int(small.faces.shape[0]), vertices=int(small.vertices.shape[0]),
                                              quality=quality(small), quality_before=quality(last), of="welded",
                                              before=dict(score(last), faces=int(last.faces.shape[0]), vertices=int(last.vertices.shape[0])))
            if decimate_placement == "optimal":
                res["welded"]["decimated"]["placement"] = "optimal"
    if geometry is not None or surface is not None:
        target = torch.from_numpy(np.ascontiguousarray(synthetic.scene(triangles, width, height, 2, seed=seed, edge_px=10.0)["vertex"])).to(m._vertex.device)
        edges = (target - target.roll(1, dims=1)).norm(dim=2)  # the hidden scene of _setup: every draw comes from the seeded generator
        median_edge = float(edges.median())
        soup_of = lambda tri: (tri.detach().reshape(-1, 3), torch.arange(3 * tri.shape[0], device=tri.device, dtype=torch.int32).reshape(-1, 3))
        thresholds = [0.5 * median_edge, median_edge, 2.0 * median_edge]
        if geometry is not None:
            res["geometry"] = dict(D.mesh_distance(soup_of(m._vertex), soup_of(target), int(geometry), seed=seed, thresholds=thresholds),
                                   median_edge=median_edge)
        if surface is not None:
            centres = torch.stack([cam.camera_center.reshape(3) for cam in cams]).to(m._vertex.device) if visible else None
            res["surface"] = dict(D.mesh_surface_distance(soup_of(m._vertex), soup_of(target), int(surface), seed=seed, thresholds=thresholds,
                                                          visible_from=centres), median_edge=median_edge)
    if extract is not None:
        soup_v, soup_f = m._vertex.detach().reshape(-1, 3), torch.arange(3 * m._vertex.shape[0], device=m._vertex.device, dtype=torch.int32).reshape(-1, 3)
        target = torch.from_numpy(np.ascontiguousarray(synthetic.scene(triangles, width, height, 2, seed=seed, edge_px=10.0)["vertex"])).to(soup_v.device)
        target_f = torch.arange(3 * target.shape[0], device=soup_v.device, dtype=torch.int32).reshape(-1, 3)
        simplified = simplify is not None or int(min_piece) > 0
        post = simplified or smooth is not None
        if extract_color:
            fused = D.fuse_colored_mesh(cams, soup_v, soup_f, D.mesh_from_triangles(m._vertex, shs, save_back=False)[2], int(extract), images=gts,
                                        return_volume=post)
        else:
            fused = D.fuse_mesh(cams, soup_v, soup_f, int(extract), return_volume=post)
        if post:
            fused, volume = fused
        welded = D.weld_mesh(soup_v, soup_f, eps=0.0)
        samples = int(surface) if surface is not None else 20000
        some = fused.faces.shape[0] > 0
        res["fused"] = dict(resolution=int(extract), topology=D.mesh_topology(fused.stats["num_vertices"], fused.faces),
                            soup=D.mesh_topology(welded.stats["num_vertices"], welded.faces),
                            to_soup=D.mesh_surface_distance((fused.vertices, fused.faces), (soup_v, soup_f), samples, seed=seed) if some else None,
                            to_target=D.mesh_surface_distance((fused.vertices, fused.faces), (target.reshape(-1, 3), target_f), samples, seed=seed) if some else None)
        if extract_color:
            res["fused"]["color"] = dict(D.evaluate_vertex_colors(cams, fused.vertices, fused.faces, fused.vertex_color, bg_color=kw["bg_color"]),
                                         vertices=int(fused.vertices.shape[0]), coloured=int(fused.color_valid.sum()),
                                         soup={k: res[k] for k in ("mean_psnr", "mean_ssim")})
        if texture is not None:
            baked = D.bake_texture(cams, fused.vertices, fused.faces, int(texture))
            res["fused"]["texture"] = dict(D.evaluate_textured(cams, fused.vertices, fused.faces, baked, bg_color=kw["bg_color"]), res=int(texture),
                                           width=baked.layout.width, height=baked.layout.height, faces=int(fused.faces.shape[0]),
                                           texels=int(fused.faces.shape[0]) * baked.layout.texels_per_face, observed=int((baked.state == 3).sum()))
            if out is not None:
                D.save_glb_textured_mesh(out, fused.vertices, fused.faces, baked)
                res["fused"]["texture"]["out"] = str(out)
        topology_of = lambda mesh: D.mesh_topology(mesh.vertices.shape[0], mesh.faces)
        if split and not simplified:
            before = res["fused"]["topology"]
            fused = D.manifold_fused(fused)
            res["fused"]["manifold"] = dict(fused.stats["manifold"], before=before, topology=topology_of(fused))
        if orient is not None and not (split and simplified):
            fused = D.orient_fused(fused, orient)
            res["fused"]["oriented"] = fused.stats["orient"]
        if fill is not None and not (split and simplified):
            fused = D.fill_fused(fused, int(fill))
            res["fused"]["filled"] = dict(fused.stats["fill"], max_loop_edges=int(fill), topology=D.mesh_topology(fused.vertices.shape[0], fused.faces))
            if split:
                res["fused"]["filled"]["before"] = res["fused"]["manifold"]["topology"]
        if smooth is not None:
            plain = fused
            fused = D.smooth_fused(plain, volume, iterations=int(smooth))
            both = lambda mesh: D.mesh_normal_consistency((mesh.vertices, mesh.faces), (soup_v, soup_f), samples, seed=seed) if some else None
            res["fused"]["smoothed"] = dict(fused.stats["smooth"], topology=D.mesh_topology(fused.vertices.shape[0], fused.faces),
                                            to_soup=D.mesh_surface_distance((fused.vertices, fused.faces), (soup_v, soup_f), samples, seed=seed) if some else None,
                                            normals=both(fused), normals_before=both(plain))
        if simplified:
            small = D.simplify_fused(fused, volume, simplify, int(min_piece))
            sv, sf, stats = small.vertices, small.faces, small.stats
            res["fused"]["simplified"] = dict(cell=simplify, min_piece=int(min_piece), faces_in=int(fused.faces.shape[0]), stats=stats,
                                              topology=D.mesh_topology(sv.shape[0], sf),
                                              to_soup=D.mesh_surface_distance((sv, sf), (soup_v, soup_f), samples, seed=seed) if sf.shape[0] else None)
            if extract_color:
                res["fused"]["simplified"]["color"] = dict(D.evaluate_vertex_colors(cams, sv, sf, small.vertex_color, bg_color=kw["bg_color"]),
                                                           vertices=int(sv.shape[0]), coloured=int(small.color_valid.sum()))
            if split:
                small = D.manifold_fused(small)
                res["fused"]["manifold"] = dict(small.stats["manifold"], before=res["fused"]["simplified"]["topology"], topology=topology_of(small))
                if orient is not None:
                    small = D.orient_fused(small, orient)
                    res["fused"]["oriented"] = small.stats["orient"]
                if fill is not None:
                    small = D.fill_fused(small, int(fill))
                    res["fused"]["filled"] = dict(small.stats["fill"], max_loop_edges=int(fill), before=res["fused"]["manifold"]["topology"],
                                                  topology=topology_of(small))
        done = small if simplified else fused  # the finished mesh: behind every step asked for above
        if check_intersections:
            res["fused"]["intersections"] = D.self_intersection_report((done.vertices, done.faces))
        if remesh is not None:
            if done.faces.shape[0]:
                if remesh_method not in ("rays", "winding"):
                    raise ValueError(f"remesh_method must be 'rays' or 'winding', not {remesh_method!r}")
                again = (D.remesh_winding if remesh_method == "winding" else D.remesh)((done.vertices, done.faces), int(remesh))
                grid = {k: again.stats[k] for k in ("dims", "voxel_size", "samples", "undecided", "inside")}
                if remesh_method == "winding":
                    grid["method"] = "winding"
                res["fused"]["remeshed"] = dict(grid, resolution=int(remesh), topology=topology_of(again),
                                                to_fused=D.mesh_surface_distance((again.vertices, again.faces), (done.vertices, done.faces), samples, seed=seed)
                                                if again.faces.shape[0] else None)
                if check_intersections:
                    res["fused"]["remeshed"]["intersections"] = D.self_intersection_report((again.vertices, again.faces))
            else:
                res["fused"]["remeshed"] = None
        if decimate_faces is not None:
            source, of = (again, "remeshed") if remesh is not None and done.faces.shape[0] else (done, "fused")
            if source.faces.shape[0]:
                small = (D.contract_mesh if decimate_placement == "optimal" else D.decimate_mesh)(source.vertices, source.faces,
                                                                                                  target_faces=int(decimate_faces))
                def shape(mesh):  # [smallest, median] triangle quality; a face that takes no part counts as degenerate
                    q = D.triangle_quality(mesh.vertices, mesh.faces).nan_to_num(0.0)
                    return [float(q.min()), float(q.median())]
                res["fused"]["decimated"] = dict(target_faces=int(decimate_faces), rounds=small.stats["rounds"], collapses=small.stats["collapsed"],
                                                 reached=small.reached, faces=int(small.faces.shape[0]), vertices=int(small.vertices.shape[0]),
                                                 quality=shape(small), quality_before=shape(source), of=of,
                                                 before=dict(faces=int(source.faces.shape[0]), vertices=int(source.vertices.shape[0])),
                                                 to_source=D.mesh_surface_distance((small.vertices, small.faces), (source.vertices, source.faces), samples,
                                                                                   seed=seed) if small.faces.shape[0] else None)
                if decimate_placement == "optimal":
                    res["fused"]["decimated"]["placement"] = "optimal"
            else:
                res["fused"]["decimated"] = None
    return res


def remeshed_report(r):
    """The lines --remesh prints for mesh_scores(...)["fused"]["remeshed"]."""
    if r is None:
        return ["remeshed mesh: no surface was extracted, nothing to remesh"]
    t, g = r["topology"], r["to_fused"]
    dist = (f"accuracy {g['accuracy']:.4g}, completeness {g['completeness']:.4g}, Chamfer {g['chamfer']:.4g}, Hausdorff {g['hausdorff']:.4g}"
            if g is not None else "no surface was extracted")
    how = ", signed by the generalised winding number" if r.get("method") == "winding" else ""
    return [f"remeshed mesh{how}, resolution {r['resolution']} ({r['dims'][0]} x {r['dims'][1]} x {r['dims'][2]} samples, {r['inside']} inside, "
            f"{r['undecided']} undecided): {t['faces']} faces, {t['pieces']} pieces, {t['boundary']} boundary edges, Euler characteristic {t['euler']}",
            f"remeshed mesh against the mesh it came from: {dist}"]


def intersections_report(r, which):
    """The line --check-intersections prints for an "intersections" entry of mesh_scores(...): of "welded", of "fused", of "remeshed"."""
    return [f"{which} mesh, self-intersections: {r['crossing_pairs']} crossing face pairs on {r['crossing_faces']} of {r['faces']} faces, "
            f"{r['coplanar_pairs']} coplanar candidate pairs, {r['duplicate_pairs']} duplicate pairs, {r['degenerate_faces']} degenerate faces"]


def smoothed_report(f):
    """The line --smooth-mesh prints for mesh_scores(...)["fused"]: the smoothed mesh of ["smoothed"] beside the fused one."""
    s, t = f["smoothed"], f["smoothed"]["topology"]
    late = "manifold" in f and "simplified" in f  # the split and the fill then follow the simplification: neither comes before the smoothing
    ahead = f["topology"] if late else f.get("filled", f.get("manifold", f))["topology"]
    same = "unchanged" if t == ahead else "CHANGED"
    if s["to_soup"] is None:
        return [f"smoothed mesh, {s['iterations']} Taubin iterations: no surface was extracted"]
    g, n, b = s["to_soup"], s["normals"], s["normals_before"]
    return [f"smoothed mesh, {s['iterations']} Taubin iterations: {s['moved']} vertices moved, largest displacement {s['max_displacement_voxels']:.3f} voxels; against the "
            f"soup: accuracy {g['accuracy']:.4g}, completeness {g['completeness']:.4g}, Chamfer {g['chamfer']:.4g}, normal consistency "
            f"{n['abs_normal_consistency']:.4f} (as fused: {b['abs_normal_consistency']:.4f}); topology {same} ({t['faces']} faces, {t['boundary']} boundary edges, "
            f"{t['pieces']} pieces, Euler characteristic {t['euler']})"]


def filled_report(f):
    """The line --fill-holes prints for mesh_scores(...)["fused"]: the filled mesh of ["filled"] beside the fused one."""
    s, b, a = f["filled"], f["filled"].get("before", f["topology"]), f["filled"]["topology"]
    return [f"filled mesh, loops of up to {s['max_loop_edges']} edges: {s['loops']} loops, {s['filled_loops']} filled ({s['new_vertices']} vertices and "
            f"{s['new_faces']} faces added), {s['open_half_edges']} open half-edges; {b['boundary']} -> {a['boundary']} boundary edges, "
            f"{b['pieces']} -> {a['pieces']} pieces, Euler characteristic {b['euler']} -> {a['euler']}"]


def manifold_report(f):
    """The line --split-nonmanifold prints for mesh_scores(...)["fused"]: the split mesh of ["manifold"] beside the mesh it split."""
    s, b, a = f["manifold"], f["manifold"]["before"], f["manifold"]["topology"]
    return [f"manifold mesh: {s['fans']} fans, {s['split_vertices']} vertices split, {s['new_vertices']} new vertices; {b['nonmanifold']} -> "
            f"{a['nonmanifold']} non-manifold edges, {s['same_direction_edges']} same-direction edges"]


def oriented_report(s, what="fused"):
    """The line --orient-faces prints for mesh_scores(...)["fused"]["oriented"] or ["welded"]["oriented"]."""
    return [f"oriented {what} mesh, outward by {s['outward']}: {s['pieces']} pieces, {s['nonorientable_pieces']} non-orientable; "
            f"{s['same_direction_before']} -> {s['same_direction_after']} same-direction edges, {s['faces_flipped']} of {s['faces']} faces flipped"]


def simplified_report(f):
    """The lines --simplify-mesh / --min-piece print for mesh_scores(...)["fused"]["simplified"]."""
    t, st = f["topology"], f["stats"]
    how = [] if f["cell"] is None else [f"cells of {f['cell']:g} voxels"]
    how += [f"pieces below {f['min_piece']} faces dropped"] if f["min_piece"] > 0 else []
    simp = st.get("simplify")
    swept = f"; {simp['collapsed']} faces collapsed, {simp['duplicates']} duplicates removed, {simp['flaps']} flaps, largest cluster {simp['largest_cluster']}" if simp else ""
    g = f["to_soup"]
    lines = [f"simplified mesh, {', '.join(how)}: {t['faces']} of {f['faces_in']} faces, {t['boundary']} boundary edges, {t['nonmanifold']} non-manifold edges, "
             f"{t['pieces']} pieces, Euler characteristic {t['euler']}{swept}",
             "simplified mesh against the soup: " + (f"accuracy {g['accuracy']:.4g}, completeness {g['completeness']:.4g}, Chamfer {g['chamfer']:.4g}, "
                                                     f"Hausdorff {g['hausdorff']:.4g}" if g is not None else "no surface is left")]
    if "color" in f:
        c = f["color"]
        lines.append(f"simplified mesh, colours averaged per cluster ({c['coloured']} of {c['vertices']} vertices coloured): "
                     f"mean PSNR {c['mean_psnr']:.2f} dB, mean SSIM {c['mean_ssim']:.4f}")
    return lines


def fused_report(f):
    """The three lines --extract-mesh prints for mesh_scores(...)["fused"]."""
    t, s = f["topology"], f["soup"]
    dist = lambda g: (f"accuracy {g['accuracy']:.4g}, completeness {g['completeness']:.4g}, Chamfer {g['chamfer']:.4g}, Hausdorff {g['hausdorff']:.4g}"
                      if g is not None else "no surface was extracted")
    return [f"fused mesh, resolution {f['resolution']}: {t['faces']} faces, {t['boundary']} boundary edges, {t['pieces']} pieces, Euler characteristic {t['euler']} "
            f"(the soup: {s['faces']} faces, {s['boundary']} boundary edges, {s['pieces']} pieces, Euler characteristic {s['euler']})",
            f"fused mesh against the soup: {dist(f['to_soup'])}",
            f"fused mesh against the target: {dist(f['to_target'])}"]


def fused_color_report(c):
    """The two lines --extract-color prints for mesh_scores(...)["fused"]["color"]."""
    return [f"fused mesh, colours fused from the {len(c['psnr'])} training views ({c['coloured']} of {c['vertices']} vertices coloured): "
            f"mean PSNR {c['mean_psnr']:.2f} dB, mean SSIM {c['mean_ssim']:.4f}",
            f"the soup, one colour per face: mean PSNR {c['soup']['mean_psnr']:.2f} dB, mean SSIM {c['soup']['mean_ssim']:.4f}"]


def fused_texture_report(t):
    """The lines --bake-texture prints for mesh_scores(...)["fused"]["texture"]."""
    lines = [f"fused mesh, a {t['width']} x {t['height']} atlas of {t['res']} texels per face edge baked from the {len(t['psnr'])} training views "
             f"({t['observed']} of {t['texels']} texels observed): mean PSNR {t['mean_psnr']:.2f} dB, mean SSIM {t['mean_ssim']:.4f}"]
    return lines + ([f"textured mesh written to {t['out']}"] if "out" in t else [])


def geometry_report(g, title="mesh geometry"):
    """The lines --eval-geometry prints for mesh_scores(...)["geometry"]; --eval-surface prints the same for ["surface"] under its own title, and
    with --eval-visible one more: the samples no camera sees."""
    hidden = [f"{title}, hidden from every camera centre and left out: {g['a_hidden']} samples of the model, {g['b_hidden']} of the target"] if "a_hidden" in g else []
    return [f"{title}, {g['a_count']} + {g['b_count']} surface samples (areas: model {g['area_a']:.4g}, target {g['area_b']:.4g}): accuracy {g['accuracy']:.4g}, "
            f"completeness {g['completeness']:.4g}, Chamfer {g['chamfer']:.4g}, Hausdorff {g['hausdorff']:.4g}",
            f"{title}, target's median edge {g['median_edge']:.4g}: F-score " +
            ", ".join(f"{f:.4f} at {k:g} edges" for k, f in zip((0.5, 1, 2), g["fscore"])),
            f"{title}, precision / recall: " + ", ".join(f"{p:.4f} / {r:.4f} at {k:g} edges" for k, p, r in zip((0.5, 1, 2), g["precision"], g["recall"]))] + hidden


def split_edges_report(s):
    """The lines --split-edges prints for mesh_scores(...)["welded"]["split"]."""
    b = s["before"]
    return [f"split mesh, no edge above {s['max_edge']:g}: faces {b['faces']} -> {s['faces']} in {s['rounds']} rounds"
            + ("" if s["converged"] else " (not converged)") + f", {s['vertices']} vertices",
            f"split mesh, face colours baked again: mean PSNR {b['mean_psnr']:.2f} -> {s['mean_psnr']:.2f} dB, mean SSIM {b['mean_ssim']:.4f} -> "
            f"{s['mean_ssim']:.4f} (before: the welded mesh baked the same way; a fit to the training views)"]


def collapse_edges_report(t):
    """The lines --collapse-edges prints for mesh_scores(...)["welded"]["collapsed"]: the collapsed mesh beside the one it was made from."""
    b = t["before"]
    return [f"collapsed mesh: {t['collapses']} collapses of edges below {t['min_edge']:g} in {t['rounds']} rounds" + ("" if t["converged"] else " (not converged)")
            + f", {t['guarded']} short edges guarded; {b['vertices']} -> {t['vertices']} vertices, {b['faces']} -> {t['faces']} faces",
            f"collapsed mesh, triangle quality: smallest {t['quality_before'][0]:.4f} -> {t['quality'][0]:.4f}, median {t['quality_before'][1]:.4f} -> "
            f"{t['quality'][1]:.4f}",
            f"collapsed mesh, face colours baked again: mean PSNR {b['mean_psnr']:.2f} -> {t['mean_psnr']:.2f} dB, mean SSIM {b['mean_ssim']:.4f} -> "
            f"{t['mean_ssim']:.4f} (before: the mesh behind the other steps)"]


def decimate_faces_report(t):
    """The lines --decimate-faces prints for a "decimated" entry of mesh_scores(...): of "welded" (with image scores) or of "fused"."""
    if t is None:
        return ["decimated mesh: no surface was extracted, nothing to decimate"]
    b = t["before"]
    how = f"reached {t['target_faces']} faces" if t["reached"] else f"did NOT reach {t['target_faces']} faces"
    why = " (every edge of a soup is a boundary edge: all vertices are held, nothing collapses)" if t["collapses"] == 0 and not t["reached"] else ""
    what = "quadric-error contractions, survivors placed at the quadric's minimum," if t.get("placement") == "optimal" else "quadric-error collapses"
    lines = [f"decimated {t['of']} mesh: {t['collapses']} {what} in {t['rounds']} rounds, {how}{why}; "
             f"{b['vertices']} -> {t['vertices']} vertices, {b['faces']} -> {t['faces']} faces",
             f"decimated {t['of']} mesh, triangle quality: smallest {t['quality_before'][0]:.4f} -> {t['quality'][0]:.4f}, median "
             f"{t['quality_before'][1]:.4f} -> {t['quality'][1]:.4f}"]
    if "mean_psnr" in t:
        lines.append(f"decimated {t['of']} mesh, face colours baked again: mean PSNR {b['mean_psnr']:.2f} -> {t['mean_psnr']:.2f} dB, mean SSIM "
                     f"{b['mean_ssim']:.4f} -> {t['mean_ssim']:.4f} (before: the mesh behind the other steps)")
    else:
        g = t["to_source"]
        lines.append(f"decimated {t['of']} mesh against the mesh it came from: " +
                     (f"accuracy {g['accuracy']:.4g}, completeness {g['completeness']:.4g}, Chamfer {g['chamfer']:.4g}, Hausdorff {g['hausdorff']:.4g}"
                      if g is not None else "no face is left"))
    return lines


def flip_edges_report(s):
    """The lines --flip-edges prints for mesh_scores(...)["welded"]["split"]: s["flipped"] beside the unflipped split mesh."""
    t = s["flipped"]
    return [f"flipped mesh: {t['flips']} flips in {t['rounds']} rounds" + ("" if t["converged"] else " (not converged)")
            + f", {t['slots']} of {s['faces']} face slots rewritten, {t['guarded']} non-Delaunay edges left guarded",
            f"flipped mesh, triangle quality: smallest {t['quality_before'][0]:.4f} -> {t['quality'][0]:.4f}, median {t['quality_before'][1]:.4f} -> "
            f"{t['quality'][1]:.4f}",
            f"flipped mesh, face colours baked again: mean PSNR {s['mean_psnr']:.2f} -> {t['mean_psnr']:.2f} dB, mean SSIM {s['mean_ssim']:.4f} -> "
            f"{t['mean_ssim']:.4f} (before: the split mesh, unflipped)"]


def weld_report(welded):
    """The lines --weld-mesh prints for mesh_scores(...)["welded"]."""
    s, t = welded["stats"], welded["topology"]
    return [f"welded mesh, eps {welded['eps']:g}: vertices {s['num_vertices_in']} -> {s['num_vertices']}, "
            f"{s['num_faces_in'] - s['num_faces']} of {s['num_faces_in']} faces dropped",
            f"welded mesh topology: {t['edges']} edges ({t['boundary']} boundary, {t['manifold']} manifold, {t['nonmanifold']} non-manifold), "
            f"{t['pieces']} pieces, Euler characteristic {t['euler']}",
            f"welded mesh, largest cluster: {s['largest_cluster']} vertices, largest displacement {s['max_displacement']:.3g}",
            f"welded mesh: mean PSNR {welded['mean_psnr']:.2f} dB, mean SSIM {welded['mean_ssim']:.4f} "
            f"(the soup: {welded['soup']['mean_psnr']:.2f} dB, {welded['soup']['mean_ssim']:.4f})"]


# ---- image-parallel: the same training over N processes (diff_recon_hip/multirank.py) ------------------------------------------------------
def _rank_state(m):
    """The replicated state of a rank as host arrays (collect=True: what the tests compare between the ranks, bit for bit)."""
    return {k: v.detach().cpu().numpy() for k, v in D.replicated_state(m).items()}


def _train_rank(rank, world, cfg, exchange, check_every, on_iteration, collect, log):
    """What one rank runs: train()'s loop with the step handed to ImageParallelLoop.  The process group is initialised by the caller."""
    iters, views, views_per_step, updates, w_geometry = cfg["iters"], cfg["views"], cfg["views_per_step"], cfg["updates"], cfg["w_geometry"]
    dev, m, cams, gts, kw, geometry_loss, g_start_iter = _setup(cfg["rasterizer"], iters, cfg["triangles"], cfg["width"], cfg["height"], cfg["seed"],
                                                                views, w_geometry, cfg["single_sh"], cfg["init_from_pcd"])
    it_now = [0]

    def render_and_loss(v):
        colour = dict(shs=m._shs) if m.single_sh else {}
        pkg = render_view(cams[v], m._vertex, None if m.single_sh else m._f_dc, None if m.single_sh else m._f_rest, m._opacity, is_training=True,
                          gamma=m.gamma, active_sh_degree=m.active_sh_degree, **colour, **kw)
        loss = photometric_loss(pkg["render"], gts[v], 0.8, 0.2)
        if geometry_loss is not None and it_now[0] > g_start_iter:
            loss = loss + w_geometry * geometry_loss(pkg["depth"], pkg["normal"], cams[v].tan_fovx, cams[v].tan_fovy)
        return loss, pkg

    def statistics_only(iteration, pkgs):  # train(updates=False): the statistics of all views, no rule
        for pkg in pkgs:
            m.update(pkg, all_views=True)
        return []

    guard = D.ReplicaGuard(every=check_every)
    loop = D.ImageParallelLoop(m, render_and_loss, exchange=exchange, guard=guard,
                               model_update=(lambda iteration, pkgs: m.model_update(iteration, pkgs, all_views=True)) if updates else statistics_only)
    losses, rows, t0 = [], [], time.perf_counter()
    for it in range(1, iters + 1):
        it_now[0] = it
        total = loop.step(it, [(it * views_per_step + k) % views for k in range(views_per_step)])
        losses.append(total / views_per_step)
        rows.append(m._vertex.shape[0])
        if on_iteration is not None:
            on_iteration(it, m, rank)
        if log and rank == 0 and (it % 50 == 0 or it == 1 or it == iters):
            log(f"iter {it:4d}  loss {float(losses[-1]):.5f}  triangles {m._vertex.shape[0]}  gamma {m.gamma:.2f}  sh {m.active_sh_degree}  ranks {world}")
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / iters
    out = dict(losses=[float(x) for x in torch.stack(losses).cpu()], log=list(m.log), sec=sec, rows=rows, gamma=m.gamma,
               active_sh_degree=m.active_sh_degree, guard_checks=guard.checks)
    if collect:
        out["state"] = _rank_state(m)
    return out


def _rank_main(rank, world, port, backend, cfg, exchange, check_every, on_iteration, collect, verbose, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(rank % torch.cuda.device_count())
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        try:
            q.put((rank, _train_rank(rank, world, cfg, exchange, check_every, on_iteration, collect, print if verbose else None)))
        except D.ReplicaDivergence as e:  # every rank raises it: each reports what it saw and ends in an orderly way
            q.put((rank, dict(divergence=(e.iteration, e.names, e.ranks))))
    finally:
        dist.destroy_process_group()


def train_ranks(world, cfg, exchange="dense", check_every=50, on_iteration=None, collect=False, log=print, timeout=1800.0):
    """train(world=N): N fresh child processes (spawn: never a fork or an exec of a process that has opened the GPU), rank r on GPU
    r % device_count; RCCL ("nccl") when every rank has a GPU of its own, gloo otherwise (several ranks sharing a card: a functional run).
    Returns (losses, summary, seconds per iteration) of rank 0; summary.ranks holds every rank's report (collect=True: with its final state as
    host arrays).  A ReplicaDivergence of the ranks is raised here again, with every rank's report in `.reports`."""
    import multiprocessing
    import queue as queue_mod
    import socket
    if exchange not in ("dense", "factored_sh"):
        raise ValueError(f"exchange must be 'dense' or 'factored_sh', not {exchange!r}")
    if world < 1 or cfg["views_per_step"] % world:
        raise ValueError(f"views_per_step ({cfg['views_per_step']}) must be a multiple of the number of ranks ({world})")
    backend = "nccl" if torch.cuda.device_count() >= world else "gloo"  # device_count() opens no device
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, backend, cfg, exchange, check_every, on_iteration, collect, log is print, q))
             for r in range(world)]
    for p in procs:
        p.start()
    reports, deadline = {}, time.monotonic() + timeout
    try:
        while len(reports) < world:  # the reports are read BEFORE the join: a child cannot end while its report sits in the pipe
            try:
                rank, rep = q.get(timeout=1.0)
                reports[rank] = rep
            except queue_mod.Empty:
                dead = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode not in (None, 0)]
                if dead:
                    raise RuntimeError(f"rank(s) ended abnormally (rank, exit code): {dead}")
                if all(p.exitcode == 0 for p in procs) and q.empty():
                    raise RuntimeError(f"ranks ended without a report: got {sorted(reports)} of {world}")
                if time.monotonic() > deadline:
                    raise RuntimeError(f"no report from every rank within {timeout:.0f} s")
        for p in procs:
            p.join(120)
    finally:
        for p in procs:  # first failure: nothing is left running
            if p.is_alive():
                p.terminate()
                p.join(30)
    codes = [p.exitcode for p in procs]
    if any(c != 0 for c in codes):
        raise RuntimeError(f"exit codes of the ranks: {codes}")
    ranks = [reports[r] for r in range(world)]
    diverged = {r: rep["divergence"] for r, rep in enumerate(ranks) if "divergence" in rep}
    if diverged:
        err = D.ReplicaDivergence(*diverged[min(diverged)])
        err.reports, err.exitcodes = diverged, codes
        raise err
    head = ranks[0]
    summary = NS(log=head["log"], ranks=ranks, world=world, backend=backend, exchange=exchange, gamma=head["gamma"],
                 active_sh_degree=head["active_sh_degree"], num_triangles=head["rows"][-1] if head["rows"] else None)
    if log and log is not print:
        log(f"{world} ranks over {backend}: {head['guard_checks']} guard checks passed")
    return head["losses"], summary, head["sec"]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rasterizer", default="2D", choices=["2D", "3D"])
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--triangles", type=int, default=20000)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--single-sh-tensor", action="store_true", help="one (P, M, 3) colour parameter with two learning rates instead of f_dc + f_rest")
    ap.add_argument("--init-from-pcd", action="store_true", help="start from diff_recon_hip.create_from_pcd (point cloud -> distCUDA2 -> equilateral triangles) like the reference's trainer")
    ap.add_argument("--factored-sh", action="store_true", help="Adam on the SH coefficients from the factored gradient (dL_dRGB per view) instead of the dense dL_dshs")
    ap.add_argument("--w-geometry", type=float, default=0.0, help="weight of the depth / normal consistency loss (0.05 in the *_VanillaTS_mesh configs)")
    ap.add_argument("--world", type=int, default=None, help="image-parallel over this many processes (rank r on GPU r %% device_count); views per step = 2, or N when N > 2")
    ap.add_argument("--exchange", default="dense", choices=["dense", "factored_sh"], help="--world: how the colour gradients travel between the ranks")
    ap.add_argument("--check-every", type=int, default=50, help="--world: iterations between two replica-guard checks (one is forced after every structural update)")
    ap.add_argument("--eval-mesh", action="store_true", help="after training, render the model as an opaque mesh (diff_recon_hip.MeshRenderer) from the training views and print PSNR / SSIM")
    ap.add_argument("--refine-mesh", action="store_true", help="with --eval-mesh: drop the triangles that win no pixel from any view and give every face the mean colour of the "
                                                               "pixels it wins (diff_recon_hip.MeshCensus), then print the triangles kept and the PSNR / SSIM of that mesh. The views "
                                                               "are the training views, so the figure is a fit and not a generalisation")
    ap.add_argument("--weld-mesh", type=float, default=None, metavar="EPS", help="with --eval-mesh: weld the front faces of the mesh scored last (diff_recon_hip.weld_mesh: "
                                                                                 "vertices within EPS of each other merge, transitively) and print V -> V', the faces dropped, "
                                                                                 "the topology, the largest cluster and the welded mesh's PSNR / SSIM beside the soup's")
    ap.add_argument("--split-edges", type=float, default=None, metavar="L", help="with --weld-mesh: split the welded mesh until no edge is longer than L "
                                                                                 "(diff_recon_hip.split_fused), bake the face colours again and print the face "
                                                                                 "count and PSNR / SSIM before and after")
    ap.add_argument("--collapse-edges", type=float, default=None, metavar="L",
                    help="with --weld-mesh: collapse the edges shorter than L of the welded mesh, behind --split-edges and --flip-edges where they "
                         "are given (diff_recon_hip.collapse_fused), bake the face colours again and print rounds, collapses, triangle quality "
                         "and PSNR / SSIM beside the mesh before")
    ap.add_argument("--decimate-faces", type=int, default=None, metavar="N",
                    help="with --weld-mesh: decimate the welded mesh, behind --split-edges, --flip-edges and --collapse-edges where they are given, to "
                         "N faces by quadric-error collapses (diff_recon_hip.decimate_fused) and bake the face colours again; with --extract-mesh: the "
                         "same of the finished fused mesh, behind --remesh where it is given (diff_recon_hip.decimate_mesh); print faces before and "
                         "after, rounds, whether N was reached, triangle quality and PSNR / SSIM or the distance to the mesh before")
    ap.add_argument("--decimate-placement", choices=("vertex", "optimal"), default="vertex",
                    help="with --decimate-faces: vertex (the default) keeps the survivor of every collapse where it was (decimate_fused / "
                         "decimate_mesh); optimal contracts edges and places the survivor at the regularised minimum of the edge's quadric "
                         "(diff_recon_hip.contract_fused / contract_mesh), blending vertex colours by how far it went")
    ap.add_argument("--flip-edges", action="store_true", help="with --split-edges: flip the edges of the split mesh toward the Delaunay condition "
                                                              "(diff_recon_hip.flip_fused), bake the face colours again and print rounds, flips, "
                                                              "triangle quality and PSNR / SSIM beside the unflipped mesh")
    ap.add_argument("--eval-geometry", type=int, default=None, metavar="N", help="with --eval-mesh: compare N surface samples of the model's front faces with N of the hidden "
                                                                                   "target triangles (diff_recon_hip.mesh_distance) and print accuracy, completeness, "
                                                                                   "Chamfer and the F-score at 0.5, 1 and 2 times the target's median edge length")
    ap.add_argument("--eval-surface", type=int, default=None, metavar="N", help="with --eval-mesh: measure N surface samples of the model's front faces against the TRIANGLES "
                                                                                  "of the hidden target and N of the target against the model's "
                                                                                  "(diff_recon_hip.mesh_surface_distance) and print the scores of --eval-geometry")
    ap.add_argument("--eval-visible", action="store_true", help="with --eval-surface: score only the samples that at least one training camera's centre sees past their own "
                                                                "mesh (ray casts, diff_recon_hip.point_visibility) and print how many were hidden")
    ap.add_argument("--extract-mesh", type=int, default=None, metavar="RES", help="with --eval-mesh: fuse the training views' depth of the mesh into a TSDF volume of RES samples "
                                                                                    "along its longest side and extract one surface (diff_recon_hip.fuse_mesh); print its "
                                                                                    "topology beside the soup's and its surface distance to the soup and to the target")
    ap.add_argument("--extract-color", action="store_true", help="with --extract-mesh: fuse the training targets' colour in the same volume (diff_recon_hip.fuse_colored_mesh) "
                                                                 "and print the PSNR / SSIM of the vertex-coloured fused mesh beside the soup's own")
    ap.add_argument("--simplify-mesh", type=float, default=None, metavar="K", help="with --extract-mesh: simplify the fused mesh by vertex clustering in cells of K voxels with "
                                                                                   "quadric placement (diff_recon_hip.simplify_mesh) and print its faces, topology and "
                                                                                   "surface distance to the soup (with --extract-color: its PSNR / SSIM)")
    ap.add_argument("--min-piece", type=int, default=0, metavar="N", help="with --extract-mesh: drop the connected pieces of the (simplified) fused mesh below N faces "
                                                                         "(diff_recon_hip.drop_small_pieces)")
    ap.add_argument("--smooth-mesh", type=int, default=None, metavar="N", help="with --extract-mesh: smooth the fused mesh with N Taubin iterations before it is simplified, every "
                                                                               "vertex within one voxel of its level set (diff_recon_hip.smooth_fused), and print its "
                                                                               "displacement, surface distance and normal consistency to the soup, and its topology")
    ap.add_argument("--fill-holes", type=int, default=None, metavar="N", help="with --extract-mesh: close the boundary loops of the fused mesh of at most N edges with centroid "
                                                                              "fans (diff_recon_hip.fill_fused) before it is smoothed or simplified, and print the loops, "
                                                                              "the filled ones, the open half-edges and the topology before and after")
    ap.add_argument("--split-nonmanifold", action="store_true", help="with --extract-mesh: give every extra fan of a vertex a vertex of its own "
                                                                     "(diff_recon_hip.manifold_fused) after --simplify-mesh / --min-piece and before --fill-holes, "
                                                                     "and print the fans, the split and new vertices, the non-manifold edges before and after and the "
                                                                     "same-direction edges")
    ap.add_argument("--orient-faces", choices=("anchor", "majority", "volume"), default=None,
                    help="with --extract-mesh: make every orientable piece of the mesh wind one way (diff_recon_hip.orient_fused) after --split-nonmanifold "
                         "and before --fill-holes; with --weld-mesh: the same on the welded mesh; print the pieces, the non-orientable ones, the "
                         "same-direction edges before and after and the faces flipped")
    ap.add_argument("--bake-texture", type=int, default=None, metavar="R", help="with --extract-mesh: bake a texture atlas of R texels per face edge (1 .. 64) for the fused "
                                                                                "mesh from the training targets (diff_recon_hip.bake_texture) and print the PSNR / SSIM "
                                                                                "of the textured mesh")
    ap.add_argument("--remesh", type=int, default=None, metavar="RES", help="with --extract-mesh: turn the finished fused mesh into a signed distance volume of RES samples along "
                                                                            "its longest side and extract it again (diff_recon_hip.remesh); print faces, pieces, boundary "
                                                                            "edges, Euler characteristic, undecided samples and the surface distance to the mesh it came from")
    ap.add_argument("--remesh-method", choices=("rays", "winding"), default="rays", help="with --remesh: what decides the sign of the distance volume: crossing counts of rays "
                                                                                          "(closed meshes) or the generalised winding number (diff_recon_hip.remesh_winding: "
                                                                                          "open meshes too)")
    ap.add_argument("--check-intersections", action="store_true", help="with --weld-mesh and / or --extract-mesh: print, for every indexed mesh produced (welded, fused, "
                                                                       "remeshed), how many face pairs cross, lie in one plane or are duplicates "
                                                                       "(diff_recon_hip.self_intersection_report)")
    ap.add_argument("--out", default=None, metavar="PATH", help="with --bake-texture: write the textured fused mesh as a GLB (diff_recon_hip.save_glb_textured_mesh)")
    a = ap.parse_args()
    if a.split_edges is not None and a.weld_mesh is None:
        ap.error("--split-edges splits the welded mesh of --weld-mesh")
    if a.collapse_edges is not None and a.weld_mesh is None:
        ap.error("--collapse-edges collapses the welded mesh of --weld-mesh")
    if a.decimate_faces is not None and a.weld_mesh is None and a.extract_mesh is None:
        ap.error("--decimate-faces decimates the mesh of --weld-mesh or of --extract-mesh")
    if a.decimate_placement != "vertex" and a.decimate_faces is None:
        ap.error("--decimate-placement chooses how --decimate-faces places the survivors")
    if a.decimate_faces is not None and a.decimate_faces < 0:
        ap.error("--decimate-faces needs a face count >= 0")
    if a.flip_edges and a.split_edges is None:
        ap.error("--flip-edges flips the split mesh of --split-edges")
    if a.split_edges is not None and not (a.split_edges > 0 and math.isfinite(a.split_edges)):
        ap.error("--split-edges needs a positive edge length")
    if a.check_intersections and a.extract_mesh is None and a.weld_mesh is None:
        ap.error("--check-intersections checks the mesh of --weld-mesh or of --extract-mesh")
    if a.remesh is not None and a.extract_mesh is None:
        ap.error("--remesh remeshes the mesh of --extract-mesh")
    if a.remesh is not None and a.remesh < 8:
        ap.error("--remesh needs a resolution of at least 8 (two voxels of padding either side)")
    if a.bake_texture is not None and a.extract_mesh is None:
        ap.error("--bake-texture textures the mesh of --extract-mesh")
    if a.bake_texture is not None and not 1 <= a.bake_texture <= 64:
        ap.error("--bake-texture needs 1 .. 64 texels per face edge")
    if a.out is not None and a.bake_texture is None:
        ap.error("--out writes the mesh of --bake-texture")
    if a.orient_faces is not None and a.extract_mesh is None and a.weld_mesh is None:
        ap.error("--orient-faces orients the mesh of --extract-mesh or of --weld-mesh")
    if a.split_nonmanifold and a.extract_mesh is None:
        ap.error("--split-nonmanifold splits the vertices of the mesh of --extract-mesh")
    if a.fill_holes is not None and a.extract_mesh is None:
        ap.error("--fill-holes fills the holes of the mesh of --extract-mesh")
    if a.fill_holes is not None and a.fill_holes < 0:
        ap.error("--fill-holes needs a number of edges >= 0")
    if a.smooth_mesh is not None and a.extract_mesh is None:
        ap.error("--smooth-mesh smooths the mesh of --extract-mesh")
    if a.smooth_mesh is not None and a.smooth_mesh < 0:
        ap.error("--smooth-mesh needs a number of iterations >= 0")
    if a.simplify_mesh is not None and a.extract_mesh is None:
        ap.error("--simplify-mesh simplifies the mesh of --extract-mesh")
    if a.min_piece and a.extract_mesh is None:
        ap.error("--min-piece filters the mesh of --extract-mesh")
    if a.simplify_mesh is not None and not (a.simplify_mesh > 0 and math.isfinite(a.simplify_mesh)):
        ap.error("--simplify-mesh needs a positive cell size in voxels")
    if a.min_piece < 0:
        ap.error("--min-piece needs a face count >= 0")
    if a.extract_color and a.extract_mesh is None:
        ap.error("--extract-color colours the mesh of --extract-mesh")
    if a.extract_mesh is not None and not a.eval_mesh:
        ap.error("--extract-mesh fuses the mesh of --eval-mesh")
    if a.extract_mesh is not None and a.extract_mesh < 10:
        ap.error("--extract-mesh needs a resolution of at least 10 (four voxels of padding either side)")
    if a.eval_visible and a.eval_surface is None:
        ap.error("--eval-visible restricts the scores of --eval-surface")
    if a.eval_surface is not None and not a.eval_mesh:
        ap.error("--eval-surface measures the mesh that --eval-mesh scores")
    if a.eval_surface is not None and a.eval_surface < 1:
        ap.error("--eval-surface needs at least one sample")
    if a.eval_geometry is not None and not a.eval_mesh:
        ap.error("--eval-geometry measures the mesh that --eval-mesh scores")
    if a.eval_geometry is not None and a.eval_geometry < 1:
        ap.error("--eval-geometry needs at least one sample")
    if a.weld_mesh is not None and not a.eval_mesh:
        ap.error("--weld-mesh welds the mesh that --eval-mesh scores")
    if a.refine_mesh and not a.eval_mesh:
        ap.error("--refine-mesh refines the mesh that --eval-mesh scores")
    if a.eval_mesh and a.world is not None:
        ap.error("--eval-mesh scores the model of the one-process loop (with --world the trained replicas live in the rank processes)")
    parallel = {} if a.world is None else dict(world=a.world, exchange=a.exchange, check_every=a.check_every,
                                               views_per_step=2 if 2 % a.world == 0 else a.world)
    losses, m, sec = train(a.rasterizer, a.iters, a.triangles, views=a.views, w_geometry=a.w_geometry, single_sh=a.single_sh_tensor, init_from_pcd=a.init_from_pcd,
                           factored_sh=a.factored_sh, **parallel)
    for row in m.log:
        print("  update", row)
    print(f"{a.rasterizer}: loss {losses[0]:.5f} -> {losses[-1]:.5f} in {a.iters} iterations, {sec * 1e3:.2f} ms/iteration (incl. Python)")
    if a.eval_mesh:
        res = mesh_scores(m, a.rasterizer, a.iters, a.triangles, views=a.views, refine=a.refine_mesh, weld=a.weld_mesh, geometry=a.eval_geometry,
                          surface=a.eval_surface, visible=a.eval_visible, extract=a.extract_mesh, extract_color=a.extract_color, simplify=a.simplify_mesh,
                          min_piece=a.min_piece, smooth=a.smooth_mesh, fill=a.fill_holes, split=a.split_nonmanifold, orient=a.orient_faces,
                          texture=a.bake_texture, out=a.out, remesh=a.remesh, remesh_method=a.remesh_method,
                          check_intersections=a.check_intersections, split_edges=a.split_edges, flip_edges=a.flip_edges, collapse_edges=a.collapse_edges,
                          decimate_faces=a.decimate_faces, decimate_placement=a.decimate_placement)
        for v, (p_, s_) in enumerate(zip(res["psnr"], res["ssim"])):
            print(f"  opaque mesh, view {v}: PSNR {p_:.2f} dB  SSIM {s_:.4f}")
        print(f"opaque mesh of {m._vertex.shape[0]} triangles: mean PSNR {res['mean_psnr']:.2f} dB, mean SSIM {res['mean_ssim']:.4f} over {len(res['psnr'])} views")
        if a.refine_mesh:
            r = res["refined"]
            print(f"refined mesh: {r['kept']} of {r['triangles']} triangles win a pixel from one of the {len(r['psnr'])} training views and are kept")
            print(f"refined mesh, colours baked from those views: mean PSNR {r['mean_psnr']:.2f} dB, mean SSIM {r['mean_ssim']:.4f} (a fit to the training views)")
        if a.weld_mesh is not None:
            for line in weld_report(res["welded"]):
                print(line)
            if "oriented" in res["welded"]:
                for line in oriented_report(res["welded"]["oriented"], "welded"):
                    print(line)
            if a.check_intersections:
                for line in intersections_report(res["welded"]["intersections"], "welded"):
                    print(line)
            if a.split_edges is not None:
                for line in split_edges_report(res["welded"]["split"]) + (flip_edges_report(res["welded"]["split"]) if a.flip_edges else []):
                    print(line)
            if a.collapse_edges is not None:
                for line in collapse_edges_report(res["welded"]["collapsed"]):
                    print(line)
            if a.decimate_faces is not None:
                for line in decimate_faces_report(res["welded"]["decimated"]):
                    print(line)
        if a.eval_geometry is not None:
            for line in geometry_report(res["geometry"]):
                print(line)
        if a.eval_surface is not None:
            for line in geometry_report(res["surface"], title="mesh surface"):
                print(line)
        if a.extract_mesh is not None:
            for line in fused_report(res["fused"]):
                print(line)
            if a.extract_color:
                for line in fused_color_report(res["fused"]["color"]):
                    print(line)
            if a.bake_texture is not None:
                for line in fused_texture_report(res["fused"]["texture"]):
                    print(line)
            late = "manifold" in res["fused"] and "simplified" in res["fused"]  # the split, and the fill behind it, follow the simplification
            if "manifold" in res["fused"] and not late:
                for line in manifold_report(res["fused"]):
                    print(line)
            if "oriented" in res["fused"] and not late:
                for line in oriented_report(res["fused"]["oriented"]):
                    print(line)
            if "filled" in res["fused"] and not late:
                for line in filled_report(res["fused"]):
                    print(line)
            if "smoothed" in res["fused"]:
                for line in smoothed_report(res["fused"]):
                    print(line)
            if "simplified" in res["fused"]:
                for line in simplified_report(res["fused"]["simplified"]):
                    print(line)
            if late:
                for line in manifold_report(res["fused"]):
                    print(line)
                if "oriented" in res["fused"]:
                    for line in oriented_report(res["fused"]["oriented"]):
                        print(line)
                if "filled" in res["fused"]:
                    for line in filled_report(res["fused"]):
                        print(line)
            if a.check_intersections:
                for line in intersections_report(res["fused"]["intersections"], "fused"):
                    print(line)
            if a.remesh is not None:
                for line in remeshed_report(res["fused"]["remeshed"]):
                    print(line)
                if a.check_intersections and res["fused"]["remeshed"] is not None:
                    for line in intersections_report(res["fused"]["remeshed"]["intersections"], "remeshed"):
                        print(line)
            if a.decimate_faces is not None:
                for line in decimate_faces_report(res["fused"]["decimated"]):
                    print(line)
