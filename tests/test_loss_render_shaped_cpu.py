"""CPU tests of the float64 loss oracle (oracle/ts_loss_oracle.py) on render-shaped inputs: tests/golden/render_shaped_losses.npz holds what the
REFERENCE's DepthNormalLoss, DoGLoss, SmoothnessLoss, SSIMLoss and L1 + torch autograd (float32) give on images with an exactly-zero-normal,
constant-depth, constant-colour background under hard-edged planar patches, and on the same images with one non-finite value
(generator: tests/golden/make_golden_render_shaped.py).  The GPU tests (test_loss_render_shaped_gpu.py) lean on this oracle for the tie bands, for
the conditioning of each pixel class and for the background of the photometric gradient, so it is pinned here first, class by class
(tests/render_shaped.py)."""
import numpy as np
import pytest

import render_shaped as R
from oracle import ts_loss_oracle as O

Z = R.Z
LOSS_TOL, GRAD_TOL = 1e-5, 1e-4   # the suite's bars: relative loss, relative L2 of a gradient
# The photometric gradient on a flat WHITE background is ill-conditioned in float32: sigma^2 = E[I^2] - mu^2 cancels two numbers near 1 against
# C2 = 9e-4, so a relative rounding error e of the 121-tap window sums arrives multiplied by mu^2 / C2 = 1111; the worst case of a 121-term float32
# accumulation is e = 121 * 2^-24.  (On a black background mu = 0 and nothing is amplified.)
FLAT_WHITE_TOL = (1.0 / O.C2) * 121 * 2.0 ** -24


@pytest.mark.parametrize("i", range(R.N_CASES))
def test_depth_normal_oracle_on_render_shaped_cases(i):
    c, o = R.case(i), R.dn_oracle(i)
    assert int(o["tie"].sum()) == int(Z[f"dn_tie{i}"]) <= R.tie_cap(c["H"], c["W"])
    ref_mask = Z[f"dn_mask{i}"].astype(bool)
    assert np.array_equal(ref_mask[~o["tie"]], (o["G"] < o["thr"])[~o["tie"]])
    if i == R.EMPTY_DN_CASE:
        # G == 0 on more than the quantile's share: threshold 0, nothing below it, loss and gradients exactly 0 -- in the reference and in the oracle
        assert float(Z[f"dn_thr{i}"]) == 0.0 and float(Z[f"dn_loss{i}"]) == 0.0 and not ref_mask.any()
        assert not Z[f"ddepth{i}"].any() and not Z[f"dnormal{i}"].any()
        assert (o["G"] == 0).mean() > c["q"] and o["thr"] == 0.0 and o["loss"] == 0.0 and not o["ddepth"].any() and not o["dnormal"].any()
        return
    assert abs(o["thr"] - float(Z[f"dn_thr{i}"])) <= 1e-6 * o["thr"]
    assert abs(o["loss"] - float(Z[f"dn_loss{i}"])) < LOSS_TOL * abs(o["loss"])
    assert o["zero_n"].mean() > 0.4 and np.array_equal(o["zero_n"], ~o["cover"])  # the background of a render: normal exactly 0
    for name, m in R.classes(o["zero_n"], "zero-normal", "other"):
        k = m & ~o["tie"]
        rho = R.rel(Z[f"dnormal{i}"][:, k], o["dnormal"][:, k])
        print(f"case {i} dL/dnormal {name}: {int(k.sum())} px, rho {rho:.3g}, max |g| {np.abs(o['dnormal'][:, k]).max():.3g}")
        assert rho < GRAD_TOL
    for name, m in R.classes(~o["cover"], "background", "foreground"):
        k = m & ~o["tie_wide"]
        rho = R.rel(Z[f"ddepth{i}"][k], o["ddepth"][k])
        print(f"case {i} dL/ddepth {name}: {int(k.sum())} px, rho {rho:.3g}")
        assert rho < GRAD_TOL


@pytest.mark.parametrize("i", R.IMAGE_CASES)
def test_image_loss_oracles_on_render_shaped_cases(i):
    c, o = R.case(i), R.image_oracle(i)
    cap = R.tie_cap(c["H"], c["W"])
    assert int(o["dog_tie"].sum()) == int(Z[f"dog_tie{i}"]) <= cap and int(o["smooth_tie"].sum()) == int(Z[f"smooth_tie{i}"]) <= cap
    assert np.array_equal(o["dog_mask"][~o["dog_tie"]], Z[f"dog_mask{i}"][~o["dog_tie"]])
    assert np.array_equal(o["smooth_mask"][~o["smooth_tie"]], Z[f"smooth_mask{i}"][~o["smooth_tie"]])
    assert abs(o["smooth_thr"] - float(Z[f"smooth_thr{i}"])) <= 1e-6 * o["smooth_thr"]
    bg = ~o["cover"]
    assert np.array_equal(Z[f"img{i}"][:, bg], Z[f"gt{i}"][:, bg]) and len(np.unique(Z[f"gt{i}"][:, bg])) == 1  # bit-equal, one colour
    white = float(Z[f"gt{i}"][0][bg][0]) == 1.0
    for g in ("dog", "smooth", "photo"):
        assert abs(o[f"{g}_loss"] - float(Z[f"{g}_loss{i}"])) < LOSS_TOL * o[f"{g}_loss"], g
        for name, m in R.classes(bg, "background", "foreground"):
            ref, ora = Z[f"{g}_grad{i}"][:, m], o[f"{g}_grad"].reshape(Z[f"{g}_grad{i}"].shape)[:, m]
            if not ora.any():
                assert not ref.any(), (g, name)  # (DoG: sign(0) = 0 where image == target; smoothness: the norm of an exact 0 has gradient 0)
                continue
            rho = R.rel(ref, ora)
            print(f"case {i} {g} {name}: rho {rho:.3g}")
            assert rho < (FLAT_WHITE_TOL if (g, name, white) == ("photo", "background", True) else GRAD_TOL), (g, name)
    # where the image equals the target bit for bit the L1 sign term is exactly 0: the photometric gradient there is the SSIM term alone
    assert np.array_equal(o["photo_grad"].reshape(Z[f"img{i}"].shape)[:, bg], o["ssim_grad"].reshape(Z[f"img{i}"].shape)[:, bg])


def test_smoothness_oracle_on_a_flat_target_background():
    """SmoothnessLoss(quantile = 0.3) on a target whose flat background leaves the gradient map exactly 0 on more than 30 % of the image:
    quantile(U, 0.3) = 0, U < 0 is empty, loss and gradient are exactly 0."""
    i = int(Z["smooth_empty_case"])
    c, q = R.case(i), float(Z["smooth_empty_q"])
    assert float(Z["smooth_empty_thr"]) == 0.0 and float(Z["smooth_empty_loss"]) == 0.0 and not Z["smooth_empty_mask"].any() and not Z["smooth_empty_grad"].any()
    aux = {}
    m = O.smoothness_mask(Z[f"gt{i}"], q, c["s"], aux)
    assert (aux["U"] == 0).mean() > q and aux["threshold"] == 0.0 and not m.any()
    loss, grad = O.smoothness_loss(Z[f"img{i}"], Z[f"gt{i}"], q, c["s"])
    assert loss == 0.0 and not grad.any()


@pytest.mark.parametrize("name", R.NF_NAMES)
def test_oracle_gives_the_reference_verdict_on_non_finite_inputs(name):
    """One NaN / inf value in case 0.  The reference multiplies by its masks (NaN * 0 = NaN) and torch.quantile is NaN as soon as one input is:
    the loss is non-finite wherever the value sits.  The oracle must say the same, loss and gradients."""
    c = R.case(0)
    depth, normal, img, gt = R.nonfinite_inputs(name)
    with np.errstate(all="ignore"):
        if f"nf_dn_loss_{name}" in Z:
            loss, dd, dn = O.depth_normal_loss(depth, normal, c["tx"], c["ty"], c["s"], c["q"])
            assert R.verdict(loss) == R.verdict(Z[f"nf_dn_loss_{name}"]) != "finite"
            assert [bool(not np.isfinite(g).all()) for g in (dd, dn)] == list(Z[f"nf_dn_bad_{name}"])
        if f"nf_smooth_loss_{name}" in Z:
            loss, grad = O.smoothness_loss(img, gt, c["qs"], c["s"])
            assert R.verdict(loss) == R.verdict(Z[f"nf_smooth_loss_{name}"]) != "finite"
            assert bool(not np.isfinite(grad).all()) == bool(Z[f"nf_smooth_bad_{name}"])
            loss, grad = O.dog_loss(img, gt, 90, c["s"])
            assert R.verdict(loss) == R.verdict(Z[f"nf_dog_loss_{name}"]) != "finite"
            assert bool(not np.isfinite(grad).all()) == bool(Z[f"nf_dog_bad_{name}"])
        if f"nf_photo_loss_{name}" in Z:
            loss, _, _, grad = O.photometric_loss(img, gt, R.W_L1, R.W_SSIM)
            assert R.verdict(loss) == R.verdict(Z[f"nf_photo_loss_{name}"]) != "finite"
            assert bool(not np.isfinite(grad).all()) == bool(Z[f"nf_photo_bad_{name}"])
