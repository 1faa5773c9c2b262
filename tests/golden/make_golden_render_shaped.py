"""Generates tests/golden/render_shaped_losses.npz from the REFERENCE's own loss classes (build container only; the reference never travels):

    python tests/golden/make_golden_render_shaped.py

The inputs look like what the rasterizer hands the losses every training step, which the smooth fields of depth_normal.npz / aux_losses.npz do not:
  depth   a constant background (37.5) under three overlapping planar patches a + b x + c y with hard silhouettes, the nearest one winning;
  normal  the patch's unit normal + 0.02 noise on covered pixels, scaled by 0.3 on ~5 % of them (partly covered rims), EXACTLY 0 on the background;
  target  a background of exactly 0.0 or exactly 1.0 around a smooth texture + noise;
  render  the target + 0.05 noise on the foreground, bit-equal to the target on the background.
Everything is built in numpy from a seed; the rasterizer is not called.  Values are rounded to short dyadic fractions (target k / 256 like an 8-bit
dataset image, render and normal to 2^-12 / 2^-11, plane coefficients to 2^-10) -- still float32 images of the same structure, but the file deflates
to a fraction of what full-mantissa noise would take.

What runs is the reference's DepthNormalLoss, DoGLoss, SmoothnessLoss, SSIMLoss and L1 (src/diff_recon/trainers/trainer_utils.py, through
make_golden.load_trainer_utils) under torch autograd in float32.  Stored per finite case i: the inputs, the loss, every input gradient, the masks
(the classes' own depth_to_normal / _dog_mask / _low_grad_mask) and the thresholds (what torch.quantile returned inside the class).  The image
losses run on cases 0-3; case 4 is a depth / normal case whose share of G == 0 pixels exceeds the quantile (threshold 0, empty mask); "smooth_empty"
is SmoothnessLoss(quantile = 0.3) on case 2's images, whose flat target background leaves the gradient map exactly 0 on more than 30 % of the
image (threshold 0, empty mask).

Non-finite cases derive from case 0 with ONE value changed (nf_names; nf_index_<name> = (channel, y, x), nf_value_<name>); stored per loss that
consumes the changed tensor: the reference's loss as a float (NaN / inf kept) and, per gradient tensor, whether it holds any non-finite value.

Tie band: a float32 pipeline may put a pixel within rounding of a hard threshold on the other side.  Per finite case the float64 oracle
(oracle/ts_loss_oracle.py) counts the pixels within 1e-4 of a threshold (relative; the band tests/test_loss_gpu.py sets aside); the generator refuses
to write unless every count is at most max(2, 1e-3 H W) -- change SEED then.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402  (the loader of the reference's trainer_utils)
from oracle import ts_loss_oracle as O  # noqa: E402

SEED = 30
W_L1, W_SSIM = 0.8, 0.2
TAN_FOVX = 0.31
# (H, W, scale_factor, depth_grad_filter_quantile, smoothness quantile, background share, target background, channels, runs the image losses)
CASES = [
    (47, 78, 0.5, 0.9, 0.6, 0.45, 0.0, 3, True),     # odd height, W % 4 != 0
    (64, 96, 0.5, 0.9, 0.6, 0.45, 1.0, 1, True),     # W % 4 == 0
    (61, 83, None, 0.9, 0.6, 0.45, 0.0, 1, True),    # no resampling
    (60, 100, 0.25, 0.7, 0.7, 0.45, 1.0, 1, True),
    (47, 78, 0.5, 0.5, None, 0.9, None, 0, False),   # G == 0 on more than the quantile's share: threshold 0, empty mask (the zero padding alone
                                                     # puts a ring of G > 0 on a fifth of an image this small, so the quantile is 0.5, not 0.9)
]


def tie_cap(H, W):
    return max(2, int(1e-3 * H * W))


def geometry(H, W, bg_share, rng):
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    # three discs that overlap; their common radius factor is bisected until the background share is the one asked for
    discs = [(rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W, rng.uniform(0.8, 1.2), np.round(rng.uniform(6, 12) * 16) / 16,
              np.round(rng.uniform(-0.02, 0.02) * 1024) / 1024, np.round(rng.uniform(-0.02, 0.02) * 1024) / 1024) for _ in range(3)]

    def place(f):
        depth = np.full((H, W), 37.5)
        normal = np.zeros((3, H, W))
        cover = np.zeros((H, W), bool)
        for cy, cx, rel, a, b, c in discs:
            inside = (yy - cy) ** 2 + (xx - cx) ** 2 < (f * rel) ** 2 * H * W
            plane = a + b * xx + c * yy
            n = np.array([b * 40, c * 40, -1.0])
            n /= np.linalg.norm(n)
            upd = inside & (plane < depth)  # the nearest patch wins
            depth = np.where(upd, plane, depth)
            cover |= upd
            for ch in range(3):
                normal[ch] = np.where(upd, n[ch], normal[ch])
        return depth, normal, cover

    lo, hi = 0.0, 1.0
    for _ in range(30):
        f = 0.5 * (lo + hi)
        depth, normal, cover = place(f)
        if 1 - cover.mean() > bg_share:
            lo = f
        else:
            hi = f
    rim = cover & (rng.random((H, W)) < 0.05)
    normal += cover * 0.02 * rng.standard_normal((3, H, W))
    normal[:, rim] *= 0.3
    normal = np.round(normal * 2 ** 11) / 2 ** 11
    normal[:, ~cover] = 0.0
    return depth.astype(np.float32), normal.astype(np.float32), cover


def images(cover, bg_value, C, rng):
    H, W = cover.shape
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    tex = 0.5 + 0.3 * np.sin(9 * xx + 3 * yy) * np.cos(7 * yy)
    gt = np.clip(tex[None] + 0.05 * rng.standard_normal((C, H, W)) + 0.08 * np.arange(C)[:, None, None], 0, 1)
    gt = np.round(gt * 256) / 256
    img = gt + np.round(0.05 * rng.standard_normal((C, H, W)) * 4096) / 4096
    gt[:, ~cover] = bg_value
    img[:, ~cover] = bg_value
    return gt.astype(np.float32), img.astype(np.float32)


class QuantileTap:
    """Records what torch.quantile returns inside the reference's classes (they keep the threshold to themselves)."""

    def __enter__(self):
        self.values, self.orig = [], torch.quantile

        def tapped(*a, **k):
            v = self.orig(*a, **k)
            self.values.append(float(v.detach()))
            return v
        torch.quantile = tapped
        return self

    def __exit__(self, *exc):
        torch.quantile = self.orig


def run_depth_normal(tu, depth, normal, s, q, tx, ty):
    d = torch.tensor(depth, requires_grad=True)
    n = torch.tensor(normal, requires_grad=True)
    mod = tu.DepthNormalLoss(scale_factor=s, depth_grad_filter_quantile=q)
    with QuantileTap() as tap:
        loss = mod(d, n, tx, ty)
    loss.backward()
    with torch.no_grad():
        mask = mod.depth_to_normal(d.detach(), tx, ty)[1].numpy()
    return float(loss), d.grad.numpy(), n.grad.numpy(), mask.astype(np.uint8), tap.values[0]


def run_image_losses(tu, img, gt, s, q, which=("dog", "smooth", "photo")):
    g = torch.tensor(gt)
    sf = 1.0 if s is None else s
    out = {}
    if "dog" in which:
        x = torch.tensor(img, requires_grad=True)
        mod = tu.DoGLoss(freq=90, scale_factor=sf)
        loss = mod(x, g)
        loss.backward()
        out["dog"] = (float(loss), x.grad.numpy(), mod._dog_mask(g[None])[0, 0].numpy().astype(np.uint8))
    if "smooth" in which:
        x = torch.tensor(img, requires_grad=True)
        mod = tu.SmoothnessLoss(quantile=q, scale_factor=sf)
        with QuantileTap() as tap:
            loss = mod(x, g)
        loss.backward()
        out["smooth"] = (float(loss), x.grad.numpy(), mod._low_grad_mask(g[None])[0, 0].numpy().astype(np.uint8), tap.values[0])
    if "photo" in which:
        x = torch.tensor(img, requires_grad=True)
        l1, sl = tu.L1(x, g), tu.SSIMLoss()(x, g)
        loss = W_L1 * l1 + W_SSIM * sl
        loss.backward()
        out["photo"] = (float(loss), x.grad.numpy(), float(l1), float(sl))
    return out


def bad(a):
    return bool(not np.isfinite(a).all())


def pick(cond, rng, reach=1):
    """One pixel (y, x), away from the border, whose (2 reach + 1)^2 neighbourhood satisfies `cond` (a Scharr response depends on the 3 x 3 one)."""
    ok = cond.copy()
    ok[:2] = ok[-2:] = False
    ok[:, :2] = ok[:, -2:] = False
    for dy in range(-reach, reach + 1):
        for dx in range(-reach, reach + 1):
            ok &= np.roll(np.roll(cond, dy, 0), dx, 1)
    ys, xs = np.nonzero(ok)
    k = int(rng.integers(len(ys)))
    return int(ys[k]), int(xs[k])


def main():
    tu = make_golden.load_trainer_utils()
    rng = np.random.default_rng(SEED)
    out = {"cases": np.array([[H, W, -1.0 if s is None else s, q, -1.0 if qs is None else qs, C, float(aux)] for H, W, s, q, qs, _, _, C, aux in CASES]),
           "weights": np.array([W_L1, W_SSIM]), "tan_fovx": np.float64(TAN_FOVX)}
    keep = {}
    for i, (H, W, s, q, qs, bg_share, bg_value, C, aux) in enumerate(CASES):
        tx, ty = TAN_FOVX, TAN_FOVX * H / W
        depth, normal, cover = geometry(H, W, bg_share, rng)
        loss, dd, dn, mask, thr = run_depth_normal(tu, depth, normal, s, q, tx, ty)
        oa = {}
        O.depth_normal_loss(depth, normal, tx, ty, s, q, need_grad=False, aux=oa)
        tie = int((np.abs(oa["G"] - oa["threshold"]) < 1e-4 * oa["threshold"]).sum())
        assert tie <= tie_cap(H, W), ("depth/normal tie band", i, tie)
        assert (thr == 0.0 and mask.sum() == 0 and loss == 0.0) if not aux else (thr > 0.0 and 0 < mask.mean() < 1), (i, thr, mask.mean())
        out.update({f"depth{i}": depth, f"normal{i}": normal, f"cover{i}": cover.astype(np.uint8), f"dn_loss{i}": np.float32(loss), f"ddepth{i}": dd,
                    f"dnormal{i}": dn, f"dn_mask{i}": mask, f"dn_thr{i}": np.float32(thr), f"dn_tie{i}": np.int64(tie)})
        print(f"case {i}: {H}x{W} background {1 - cover.mean():.3f} dn loss {loss:.6g} thr {thr:.6g} G==0 {np.mean(oa['G'] == 0):.3f} tie {tie}")
        if not aux:
            continue
        gt, img = images(cover, bg_value, C, rng)
        r = run_image_losses(tu, img, gt, s, qs)
        oa = {}
        O.dog_mask(gt, 90, s, oa)
        tie_dog = int((np.abs(oa["normalized"] - 0.5) < 1e-4 * 0.5).sum())
        oa = {}
        O.smoothness_mask(gt, qs, s, oa)
        tie_sm = int((np.abs(oa["U"] - oa["threshold"]) < 1e-4 * oa["threshold"]).sum())
        assert tie_dog <= tie_cap(H, W) and tie_sm <= tie_cap(H, W), ("image tie bands", i, tie_dog, tie_sm)
        assert r["smooth"][3] > 0.0 and 0 < r["smooth"][2].mean() < 1 and 0 < r["dog"][2].mean() < 1, i
        out.update({f"gt{i}": gt, f"img{i}": img,
                    f"dog_loss{i}": np.float32(r["dog"][0]), f"dog_grad{i}": r["dog"][1], f"dog_mask{i}": r["dog"][2], f"dog_tie{i}": np.int64(tie_dog),
                    f"smooth_loss{i}": np.float32(r["smooth"][0]), f"smooth_grad{i}": r["smooth"][1], f"smooth_mask{i}": r["smooth"][2],
                    f"smooth_thr{i}": np.float32(r["smooth"][3]), f"smooth_tie{i}": np.int64(tie_sm),
                    f"photo_loss{i}": np.float32(r["photo"][0]), f"photo_grad{i}": r["photo"][1], f"l1_{i}": np.float32(r["photo"][2]),
                    f"ssim_loss{i}": np.float32(r["photo"][3])})
        print(f"        dog {r['dog'][0]:.6g} (mask {r['dog'][2].mean():.3f}, tie {tie_dog}) smooth {r['smooth'][0]:.6g} (thr {r['smooth'][3]:.6g}, "
              f"mask {r['smooth'][2].mean():.3f}, U==0 {np.mean(oa['U'] == 0):.3f}, tie {tie_sm}) photo {r['photo'][0]:.6g}")
        if i == 0:
            keep = dict(depth=depth, normal=normal, cover=cover, gt=gt, img=img, dn_mask=mask.astype(bool), smooth_mask=r["smooth"][2].astype(bool))
        if i == 2:
            # the default quantile on a target whose flat background leaves U == 0 on more than 30 % of the image: threshold 0, nothing below it
            e = run_image_losses(tu, img, gt, s, 0.3, which=("smooth",))["smooth"]
            assert e[0] == 0.0 and e[3] == 0.0 and e[2].sum() == 0 and not e[1].any(), e[0]
            out.update(smooth_empty_case=np.int64(i), smooth_empty_q=np.float64(0.3), smooth_empty_loss=np.float32(e[0]), smooth_empty_grad=e[1],
                       smooth_empty_mask=e[2], smooth_empty_thr=np.float32(e[3]))
    # ---- non-finite cases: case 0 with one value changed ---------------------------------------------------------------------------------
    H, W, s, q, qs = CASES[0][:5]
    tx, ty = TAN_FOVX, TAN_FOVX * H / W
    nan, inf = float("nan"), float("inf")
    cov, dm, sm = keep["cover"], keep["dn_mask"], keep["smooth_mask"]
    changes = [("a", "normal", (1,) + pick(cov & ~dm, rng, 0), nan),    # a NaN normal component where G >= thr (masked out)
               ("b", "normal", (1,) + pick(cov & dm, rng, 0), nan),     # ... where G < thr
               ("c", "depth", (0,) + pick(cov, rng), nan),
               ("d", "depth", (0,) + pick(cov, rng), inf),
               ("e", "img", (1,) + pick(cov & ~sm, rng), nan),       # outside the smoothness mask, the 3 x 3 neighbourhood included
               ("f", "img", (1,) + pick(cov & sm, rng), nan),        # inside
               ("g", "img", (2,) + pick(cov, rng), nan)]             # the photometric loss's image
    out["nf_names"] = np.array([c[0] for c in changes])
    out["nf_tensor"] = np.array([c[1] for c in changes])
    for name, tensor, (ch, y, x), value in changes:
        out[f"nf_index_{name}"] = np.array([ch, y, x], np.int64)
        out[f"nf_value_{name}"] = np.float32(value)
        t = {k: keep[k].copy() for k in ("depth", "normal", "img")}
        if tensor == "depth":
            t["depth"][y, x] = value
        else:
            t[tensor][ch, y, x] = value
        if tensor in ("normal", "depth"):
            loss, dd, dn, _, thr = run_depth_normal(tu, t["depth"], t["normal"], s, q, tx, ty)
            out[f"nf_dn_loss_{name}"] = np.float32(loss)
            out[f"nf_dn_bad_{name}"] = np.array([bad(dd), bad(dn)])
            print(f"non-finite ({name}): {tensor}{(ch, y, x)} = {value}: dn loss {loss} thr {thr} bad gradients (depth, normal) {bad(dd), bad(dn)}")
        elif name in ("e", "f"):
            r = run_image_losses(tu, t["img"], keep["gt"], s, qs, which=("dog", "smooth"))
            out[f"nf_smooth_loss_{name}"], out[f"nf_smooth_bad_{name}"] = np.float32(r["smooth"][0]), np.array(bad(r["smooth"][1]))
            out[f"nf_dog_loss_{name}"], out[f"nf_dog_bad_{name}"] = np.float32(r["dog"][0]), np.array(bad(r["dog"][1]))
            print(f"non-finite ({name}): img{(ch, y, x)} = {value}: smooth {r['smooth'][0]} bad {bad(r['smooth'][1])}, dog {r['dog'][0]} bad {bad(r['dog'][1])}")
        else:
            r = run_image_losses(tu, t["img"], keep["gt"], s, qs, which=("photo",))
            out[f"nf_photo_loss_{name}"], out[f"nf_photo_bad_{name}"] = np.float32(r["photo"][0]), np.array(bad(r["photo"][1]))
            print(f"non-finite ({name}): img{(ch, y, x)} = {value}: photo {r['photo'][0]} bad {bad(r['photo'][1])}")
    path = os.path.join(HERE, "render_shaped_losses.npz")
    np.savez_compressed(path, **out)
    print("render_shaped_losses.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
