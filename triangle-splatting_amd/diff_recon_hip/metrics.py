"""Evaluation helpers: the numbers the reference's trainer reports for a view (src/diff_recon/trainers/VanillaTS_trainer.py:156-190).

    psnr(img1, img2, mask=None)   trainer_utils.py:331-336, both formulas with their 1e-10 terms
    ssim(img1, img2)              1 - SSIMLoss, as VanillaTS_trainer.py:169-170 reports it, through the fused photometric kernel
    evaluate_mesh(views, ...)     PSNR / SSIM of the opaque render of a mesh (MeshRenderer) against each view's gt_image

LPIPS is not offered: its network weights are not part of this tree."""
from __future__ import annotations

from typing import Dict, Iterable

import torch

from .losses import PhotometricLoss
from .mesh_renderer import MeshRenderer


def psnr(img1: torch.Tensor, img2: torch.Tensor, mask: torch.Tensor = None) -> torch.Tensor:
    err = (img1 - img2) ** 2
    if mask is None:
        mse = err.mean() + 1e-10
    else:  # the error summed over the channels, averaged over the masked PIXELS, like the reference
        mse = (err * mask).sum() / (mask.sum() + 1e-10) + 1e-10
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


_ssim_loss = PhotometricLoss(w_L1=0.0, w_ssim=1.0)


def ssim(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    return 1.0 - _ssim_loss(img1, img2)


def evaluate_mesh(views: Iterable, vertices: torch.Tensor, faces: torch.Tensor, faces_color: torch.Tensor,
                  bg_color: torch.Tensor = torch.Tensor([0, 0, 0])) -> Dict[str, object]:
    """Renders the mesh opaquely from every view (a camera as MeshRenderer takes it, with `gt_image` (3, H, W) and optionally `alpha_mask`)
    and scores it as the trainer's `_evaluate` scores a model: PSNR under the view's alpha mask when it has one, SSIM = 1 - SSIMLoss.
    Returns {"psnr": [...], "ssim": [...], "mean_psnr": float, "mean_ssim": float} (NaN means for no views)."""
    psnrs, ssims = [], []
    for view in views:
        image = MeshRenderer(view, bg_color).render(vertices, faces, faces_color)["render"]
        gt = view.gt_image.to(image.device)
        alpha = getattr(view, "alpha_mask", None)
        psnrs.append(float(psnr(image, gt, alpha.to(image.device) if alpha is not None else None).item()))
        ssims.append(float(ssim(image, gt.contiguous()).item()))
    n = len(psnrs)
    return {"psnr": psnrs, "ssim": ssims, "mean_psnr": sum(psnrs) / n if n else float("nan"), "mean_ssim": sum(ssims) / n if n else float("nan")}


def evaluate_vertex_colors(views: Iterable, vertices: torch.Tensor, faces: torch.Tensor, vertex_color: torch.Tensor,
                           bg_color: torch.Tensor = torch.Tensor([0, 0, 0])) -> Dict[str, object]:
    """evaluate_mesh for a mesh with one colour per VERTEX (V, 3), drawn by color_volume.render_vertex_colors: the same loop, the same keys."""
    from .color_volume import render_vertex_colors  # libts_color.so is loaded on first use
    psnrs, ssims = [], []
    for view in views:
        image = render_vertex_colors(view, vertices, faces, vertex_color, bg_color)["render"]
        gt = view.gt_image.to(image.device)
        alpha = getattr(view, "alpha_mask", None)
        psnrs.append(float(psnr(image, gt, alpha.to(image.device) if alpha is not None else None).item()))
        ssims.append(float(ssim(image, gt.contiguous()).item()))
    n = len(psnrs)
    return {"psnr": psnrs, "ssim": ssims, "mean_psnr": sum(psnrs) / n if n else float("nan"), "mean_ssim": sum(ssims) / n if n else float("nan")}
