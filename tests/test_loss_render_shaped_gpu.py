"""The loss kernels (csrc/depth_normal.hip, aux_losses.hip, photometric.hip, select.hip through diff_recon_hip.losses) on what the rasterizer hands
them every training step -- a background with a normal of exactly (0, 0, 0), constant depth and one flat colour under hard-edged patches -- and on
the same images with ONE non-finite value, against the reference's own classes + torch autograd in float32
(tests/golden/render_shaped_losses.npz, generator tests/golden/make_golden_render_shaped.py).

Gradients are compared per pixel class, never over the whole array: |dL/dnormal| is ~1e4 on zero-normal pixels and ~1e-4 on covered ones, so a
whole-array norm would pass with every covered pixel wrong.  Bars: loss 1e-5 relative, gradients 1e-4 relative L2 against the reference's float32
result; where a class is ill-conditioned in float32 the bar is max(1e-4, 2 rho), rho = the distance between the reference's float32 gradient and the
float64 oracle on that class (tests/render_shaped.py; nothing from the kernels goes into it).  Pixels within 1e-4 of a hard threshold are set
aside, after their number has been checked against the generator's cap.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import render_shaped as R

pytestmark = pytest.mark.gpu

Z = R.Z
LOSS_TOL = 1e-5
GO = 2.5  # upstream gradient: the backward kernels' grad_out path


def _cuda(a, grad=False):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def _depth_normal(depth, normal, c):
    from diff_recon_hip import DepthNormalLoss
    d, n = _cuda(depth, True), _cuda(normal, True)
    loss = DepthNormalLoss(scale_factor=c["s"], depth_grad_filter_quantile=c["q"])(d, n, c["tx"], c["ty"])
    (GO * loss).backward()
    return float(loss), d.grad.cpu().numpy() / GO, n.grad.cpu().numpy() / GO


def _check_class(what, got, ref, ora):
    """One pixel class of one gradient: the kernel against the reference's float32 values, under max(1e-4, 2 rho)."""
    rho, dist = R.rel(ref, ora), R.rel(got, ref)
    print(f"{what}: {ref.size} values, rho {rho:.3g}, kernel vs reference {dist:.3g}, bar {R.bar(rho):.3g}")
    assert dist < R.bar(rho), what


@pytest.mark.parametrize("i", [i for i in range(R.N_CASES) if i != R.EMPTY_DN_CASE])
def test_depth_normal_loss_on_render_shaped_cases(i):
    """Zero normals on ~45 % of the image (dn_bwd_fullres_kernel's `len <= 1e-8` branch), G == 0 on the flat background, hard silhouettes."""
    c, o = R.case(i), R.dn_oracle(i)
    print(f"case {i}: tie band {int(o['tie'].sum())} px (cap {R.tie_cap(c['H'], c['W'])}), widened for dL/ddepth {int(o['tie_wide'].sum())} px")
    assert int(o["tie"].sum()) <= R.tie_cap(c["H"], c["W"])
    loss, dd, dn = _depth_normal(Z[f"depth{i}"], Z[f"normal{i}"], c)
    want = float(Z[f"dn_loss{i}"])
    print(f"case {i}: loss {loss!r} reference {want!r} relative {abs(loss - want) / want:.3g}")
    assert abs(loss - want) < LOSS_TOL * want
    for name, m in R.classes(o["zero_n"], "zero-normal", "other"):
        k = m & ~o["tie"]
        _check_class(f"case {i} dL/dnormal {name}", dn[:, k], Z[f"dnormal{i}"][:, k], o["dnormal"][:, k])
    for name, m in R.classes(~o["cover"], "background", "foreground"):
        k = m & ~o["tie_wide"]
        _check_class(f"case {i} dL/ddepth {name}", dd[k], Z[f"ddepth{i}"][k], o["ddepth"][k])


def test_depth_normal_loss_with_an_empty_mask():
    """G == 0 on more than the quantile's share of the image: quantile(G, q) = 0 sits on a run of duplicates, G < 0 is empty, and the loss and
    both gradients are exactly 0, as in the reference."""
    i = R.EMPTY_DN_CASE
    loss, dd, dn = _depth_normal(Z[f"depth{i}"], Z[f"normal{i}"], R.case(i))
    print(f"loss {loss!r}, max |dL/ddepth| {np.abs(dd).max()!r}, max |dL/dnormal| {np.abs(dn).max()!r}")
    assert loss == 0.0 and not dd.any() and not dn.any()


@pytest.mark.parametrize("i", R.IMAGE_CASES)
def test_image_losses_on_render_shaped_cases(i):
    """DoGLoss, SmoothnessLoss and the photometric loss on a target with a flat black / white background and a render that equals it there bit for
    bit: the masks pixel for pixel outside the tie band, then each loss and gradient ON the reference's mask, class by class."""
    import torch
    from diff_recon_hip import DoGLoss, SmoothnessLoss, photometric_loss
    from diff_recon_hip.losses import _MaskedL1, _ScharrSmoothness
    c, o = R.case(i), R.image_oracle(i)
    C, H, W = c["C"], c["H"], c["W"]
    cap, bg = R.tie_cap(H, W), ~o["cover"]
    gt = _cuda(Z[f"gt{i}"])
    for name, mod, fn in (("dog", DoGLoss(freq=90, scale_factor=c["s"]), _MaskedL1), ("smooth", SmoothnessLoss(quantile=c["qs"], scale_factor=c["s"]), _ScharrSmoothness)):
        tie = o[f"{name}_tie"]
        print(f"case {i} {name}: tie band {int(tie.sum())} px (cap {cap})")
        assert int(tie.sum()) <= cap
        m = mod.mask(gt).cpu().numpy()
        ref_m = Z[f"{name}_mask{i}"].astype(np.float32)
        print(f"case {i} {name}: mask differs on {int((m != ref_m)[~tie].sum())} px outside the tie band, {int((m != ref_m)[tie].sum())} inside")
        assert set(np.unique(m)) <= {0.0, 1.0} and np.array_equal(m[~tie], ref_m[~tie])
        x = _cuda(Z[f"img{i}"], True)
        ws, _ = mod._workspace(gt, C, H, W)
        rm = _cuda(ref_m)
        loss = fn.apply(x, gt, rm, C, H, W, ws) if name == "dog" else fn.apply(x, rm, C, H, W, ws)
        (GO * loss).backward()
        want, got = float(Z[f"{name}_loss{i}"]), x.grad.cpu().numpy() / GO
        print(f"case {i} {name}: loss {float(loss)!r} reference {want!r} relative {abs(float(loss) - want) / want:.3g}")
        assert abs(float(loss) - want) < LOSS_TOL * want
        for cname, k in R.classes(bg, "background", "foreground"):
            ref, ora = Z[f"{name}_grad{i}"][:, k], o[f"{name}_grad"][:, k]
            if not ref.any():
                # DoG: sign(0) = 0 where image == target; smoothness: a locally constant image has a Scharr norm of exactly 0, whose gradient is 0
                print(f"case {i} {name} {cname}: reference exactly 0, kernel max {np.abs(got[:, k]).max()!r}")
                assert not got[:, k].any(), (name, cname)
            else:
                _check_class(f"case {i} {name} {cname}", got[:, k], ref, ora)
        if np.array_equal(m, ref_m):  # the class end to end, on its own mask
            assert abs(float(mod(_cuda(Z[f"img{i}"]), gt)) - want) < LOSS_TOL * want
    x = _cuda(Z[f"img{i}"], True)
    loss = photometric_loss(x, gt, R.W_L1, R.W_SSIM)
    (GO * loss).backward()
    want, got = float(Z[f"photo_loss{i}"]), x.grad.cpu().numpy() / GO
    print(f"case {i} photometric: loss {float(loss)!r} reference {want!r} relative {abs(float(loss) - want) / want:.3g} (oracle {o['photo_loss']!r})")
    assert abs(float(loss) - want) < LOSS_TOL * want
    for cname, k in R.classes(bg, "background", "foreground"):
        _check_class(f"case {i} photometric {cname}", got[:, k], Z[f"photo_grad{i}"][:, k], o["photo_grad"][:, k])
    # Background: image == target bit for bit, the L1 sign term is exactly 0 and the gradient is the SSIM term alone -- against the oracle's.  The bar
    # is the same max(1e-4, 2 rho): the kernel's float32 evaluation and the reference's are each about rho from the float64 value.
    rho, dist = R.rel(Z[f"photo_grad{i}"][:, bg], o["ssim_grad"][:, bg]), R.rel(got[:, bg], o["ssim_grad"][:, bg])
    print(f"case {i} photometric background against the oracle's SSIM term: rho {rho:.3g}, kernel vs oracle {dist:.3g}, bar {R.bar(rho):.3g}")
    assert dist < R.bar(rho)
    # the masked L1 alone (what DoGLoss differentiates) with a mask of ones is the plain L1: exactly 0 gradient on the background
    x = _cuda(Z[f"img{i}"], True)
    ws, _ = DoGLoss()._workspace(gt, C, H, W)
    _MaskedL1.apply(x, gt, torch.ones((H, W), device="cuda"), C, H, W, ws).backward()
    g1 = x.grad.cpu().numpy()
    assert not g1[:, bg].any() and np.array_equal(g1[:, ~bg], (np.sign(Z[f"img{i}"] - Z[f"gt{i}"]) / np.float32(C * H * W)).astype(np.float32)[:, ~bg])


def test_smoothness_loss_with_an_empty_mask():
    """The default quantile 0.3 on a target whose flat background leaves U == 0 on more than 30 % of the image: threshold 0, mask all zeros, loss
    and every gradient element exactly 0."""
    from diff_recon_hip import SmoothnessLoss
    i = int(Z["smooth_empty_case"])
    mod = SmoothnessLoss(quantile=float(Z["smooth_empty_q"]), scale_factor=R.case(i)["s"])
    gt, x = _cuda(Z[f"gt{i}"]), _cuda(Z[f"img{i}"], True)
    m = mod.mask(gt).cpu().numpy()
    loss = mod(x, gt)
    loss.backward()
    print(f"mask sum {m.sum()!r}, loss {float(loss)!r}, max |gradient| {float(x.grad.abs().max())!r}")
    assert not m.any() and float(loss) == 0.0 and not x.grad.cpu().numpy().any()


def _same_verdict(what, got, want, bad_got, bad_want):
    print(f"{what}: loss {got!r}, reference {float(want)!r}; non-finite gradients {bad_got}, reference {[bool(b) for b in bad_want]}")
    assert R.verdict(got) == R.verdict(want), what
    if R.verdict(want) == "finite":
        assert abs(got - float(want)) < LOSS_TOL * abs(float(want)), what
    for g, w in zip(bad_got, bad_want):
        assert g or not w, what  # every gradient tensor that is non-finite in the reference holds a non-finite value here; the pattern is not compared


@pytest.mark.parametrize("name", R.NF_NAMES)
def test_non_finite_inputs_reach_the_loss(name):
    """One NaN / inf value in case 0.  (a) / (b) a NaN normal component where G >= thr / G < thr; (c) / (d) a NaN / +inf depth pixel; (e) / (f) a NaN
    render pixel outside / inside the smoothness mask, also fed to the DoG loss; (g) a NaN pixel in the photometric loss's image.  The reference
    multiplies by its masks and torch.quantile is NaN as soon as one input is, so its loss is non-finite in every case: a trainer's
    isfinite(loss) guard sees a diverged render wherever the value sits.  A kernel that SKIPS masked-out pixels, or orders a NaN above +inf and
    selects a finite threshold, hides it.
    Before the fix (dn_sum_kernel, the select's NaN flag, aux_smooth_sum_kernel) cases a, c, d and e returned a finite loss here, and in a and b
    dL/dnormal was finite: the normalisation's fmaxf(|n|, eps) dropped the NaN length and handed back eps."""
    from diff_recon_hip import DoGLoss, SmoothnessLoss, photometric_loss
    c = R.case(0)
    depth, normal, img, gt = R.nonfinite_inputs(name)
    bad = lambda t: bool(not np.isfinite(t).all())
    if f"nf_dn_loss_{name}" in Z:
        loss, dd, dn = _depth_normal(depth, normal, c)
        _same_verdict(f"({name}) depth / normal", loss, Z[f"nf_dn_loss_{name}"], [bad(dd), bad(dn)], Z[f"nf_dn_bad_{name}"])
    if f"nf_smooth_loss_{name}" in Z:
        for what, mod in (("smooth", SmoothnessLoss(quantile=c["qs"], scale_factor=c["s"])), ("dog", DoGLoss(freq=90, scale_factor=c["s"]))):
            x = _cuda(img, True)
            loss = mod(x, _cuda(gt))
            loss.backward()
            _same_verdict(f"({name}) {what}", float(loss), Z[f"nf_{what}_loss_{name}"], [bad(x.grad.cpu().numpy())], [Z[f"nf_{what}_bad_{name}"]])
    if f"nf_photo_loss_{name}" in Z:
        x = _cuda(img, True)
        loss = photometric_loss(x, _cuda(gt), R.W_L1, R.W_SSIM)
        loss.backward()
        _same_verdict(f"({name}) photometric", float(loss), Z[f"nf_photo_loss_{name}"], [bad(x.grad.cpu().numpy())], [Z[f"nf_photo_bad_{name}"]])


def test_photometric_loss_is_the_same_bits_from_misaligned_storage():
    """A W % 4 == 0 image pair whose storage starts 4 bytes off a 16-byte boundary (a slice of a larger buffer) goes through load_halo_tile's scalar
    loader, an aligned copy through its float4 loader: the same tile, so the same bits, loss and gradient."""
    import torch
    from diff_recon_hip import photometric_loss
    i = 1
    img, gt = Z[f"img{i}"], Z[f"gt{i}"]
    assert img.shape[-1] % 4 == 0
    n = img.size

    def shifted(a):
        buf = torch.zeros(n + 8, device="cuda")
        off = 1 + (-(buf.data_ptr() // 4) % 4)  # first element 4 bytes past a 16-byte boundary
        buf[off:off + n] = torch.from_numpy(a).cuda().reshape(-1)
        return buf[off:off + n].view(a.shape)

    out = []
    for x, g in ((_cuda(img), _cuda(gt)), (shifted(img), shifted(gt))):
        out.append((x.data_ptr() % 16, g.data_ptr() % 16))
        x = x.detach().requires_grad_(True)
        loss = photometric_loss(x, g, R.W_L1, R.W_SSIM)
        loss.backward()
        out.append((loss.detach().cpu().numpy(), x.grad.cpu().numpy()))
    assert out[0] == (0, 0) and out[2] == (4, 4), (out[0], out[2])
    assert out[1][0].tobytes() == out[3][0].tobytes() and out[1][1].tobytes() == out[3][1].tobytes()
