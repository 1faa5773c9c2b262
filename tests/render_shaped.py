"""Shared by tests/test_loss_render_shaped_cpu.py and tests/test_loss_render_shaped_gpu.py: the render-shaped fixtures
(tests/golden/render_shaped_losses.npz, generator tests/golden/make_golden_render_shaped.py), the float64 oracle evaluated ONCE per case, the pixel
classes and the tie bands.  Nothing here touches the GPU or the kernels under test.

Pixel classes: dL/dnormal -- zero-normal pixels (the background of a render; |dL/dn| ~ 1e4 there, F.normalize's eps branch) and all others (~1e-4);
dL/ddepth and the image gradients -- background and foreground (`cover`).  A whole-array norm is decided by one class alone.
Tie band: pixels whose G / U / normalised DoG lies within 1e-4 (relative) of its hard threshold may fall on either side in a float32 pipeline; they
are set aside, and their number is capped (TIE_CAP) before anything is compared.  dL/ddepth of a pixel collects terms from the pixels whose
up-sampling, Scharr and down-sampling footprints reach it, so there the band is widened by that reach."""
import functools
import os

import numpy as np

from oracle import ts_loss_oracle as O

Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_shaped_losses.npz"))
W_L1, W_SSIM = (float(v) for v in Z["weights"])
N_CASES = len(Z["cases"])
IMAGE_CASES = [i for i in range(N_CASES) if Z["cases"][i][6] > 0]
EMPTY_DN_CASE = 4
NF_NAMES = [str(n) for n in Z["nf_names"]]


def case(i):
    H, W, s, q, qs, C, aux = Z["cases"][i]
    H, W = int(H), int(W)
    tx = float(Z["tan_fovx"])
    return dict(H=H, W=W, s=None if s < 0 else float(s), q=float(q), qs=None if qs < 0 else float(qs), C=int(C), tx=tx, ty=tx * H / W)


def tie_cap(H, W):
    return max(2, int(1e-3 * H * W))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def dilate(m, r):
    out = m.copy()
    H, W = m.shape
    for y, x in zip(*np.nonzero(m)):
        out[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
    return out


@functools.lru_cache(maxsize=None)
def dn_oracle(i):
    """float64 oracle of the depth / normal loss on finite case i, its tie band and the pixel classes."""
    c = case(i)
    aux = {}
    loss, dd, dn = O.depth_normal_loss(Z[f"depth{i}"], Z[f"normal{i}"], c["tx"], c["ty"], c["s"], c["q"], aux=aux)
    tie = np.abs(aux["G"] - aux["threshold"]) < 1e-4 * aux["threshold"]
    reach = 2 + int(np.ceil(2.5 / (c["s"] or 1.0)))  # Scharr (1 low-resolution pixel) + the two bilinear footprints, in full-resolution pixels
    cover = Z[f"cover{i}"].astype(bool)
    zero_n = np.abs(Z[f"normal{i}"]).sum(0) == 0
    return dict(loss=loss, ddepth=dd, dnormal=dn, G=aux["G"], thr=aux["threshold"], tie=tie, tie_wide=dilate(tie, reach), cover=cover, zero_n=zero_n)


@functools.lru_cache(maxsize=None)
def image_oracle(i):
    """float64 oracles of the three image losses on finite case i, each loss ON THE REFERENCE'S MASK (the differentiable part), + the oracle's masks."""
    c = case(i)
    img, gt = Z[f"img{i}"], Z[f"gt{i}"]
    a1, a2 = {}, {}
    dog_m = O.dog_mask(gt, 90, c["s"], a1)
    sm_m = O.smoothness_mask(gt, c["qs"], c["s"], a2)
    dog_loss, dog_grad = O.dog_loss(img, gt, 90, c["s"], mask=Z[f"dog_mask{i}"].astype(np.float64))
    sm_loss, sm_grad = O.smoothness_loss(img, gt, c["qs"], c["s"], mask=Z[f"smooth_mask{i}"].astype(np.float64))
    ph_loss, l1, sl, ph_grad = O.photometric_loss(img, gt, W_L1, W_SSIM)
    _, _, _, ssim_grad = O.photometric_loss(img, gt, 0.0, W_SSIM)  # the SSIM term alone: what remains where image == target bit for bit
    return dict(dog_mask=dog_m, dog_tie=np.abs(a1["normalized"] - 0.5) < 1e-4 * 0.5, smooth_mask=sm_m, smooth_thr=a2["threshold"],
                smooth_tie=np.abs(a2["U"] - a2["threshold"]) < 1e-4 * a2["threshold"], dog_loss=dog_loss, dog_grad=dog_grad, smooth_loss=sm_loss,
                smooth_grad=sm_grad, photo_loss=ph_loss, photo_grad=ph_grad, ssim_grad=ssim_grad, cover=Z[f"cover{i}"].astype(bool))


def classes(mask_a, name_a, name_b):
    return ((name_a, mask_a), (name_b, ~mask_a))


def bar(rho):
    """The suite's gradient bar, 1e-4 relative L2 against the reference's float32 result; where a class is ill-conditioned in float32 -- the
    reference's own float32 gradient is `rho` away from the float64 oracle -- twice that distance, because two independent float32 evaluations can
    err to opposite sides."""
    return max(1e-4, 2.0 * rho)


def nonfinite_inputs(name):
    """Case 0 with the one value of non-finite case `name` changed: (depth, normal, img, gt)."""
    t = {k: Z[f"{k}0"].copy() for k in ("depth", "normal", "img")}
    ch, y, x = (int(v) for v in Z[f"nf_index_{name}"])
    which = str(Z["nf_tensor"][NF_NAMES.index(name)])
    if which == "depth":
        t["depth"][y, x] = Z[f"nf_value_{name}"]
    else:
        t[which][ch, y, x] = Z[f"nf_value_{name}"]
    return t["depth"], t["normal"], t["img"], Z["gt0"]


def verdict(v):
    v = float(v)
    return "nan" if v != v else ("+inf" if v == float("inf") else ("-inf" if v == float("-inf") else "finite"))
