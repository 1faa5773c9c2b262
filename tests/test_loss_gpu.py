"""GPU parity of the fused photometric loss (csrc/photometric.hip through diff_recon_hip.losses -> ctypes -> C ABI)
against the float64 oracle and the committed golden vectors of the reference's SSIM / L1 classes."""
import os

import numpy as np
import pytest

import helpers
from oracle import ts_loss_oracle as LO

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "photometric.npz"))
VAL_TOL = 2e-6    # fp32 evaluation of a mean of O(1) terms
GRAD_TOL = 2e-5   # relative L2


def _run(img, gt, w1, ws):
    import torch
    from diff_recon_hip import photometric_loss
    x = torch.tensor(img, device="cuda", requires_grad=True)
    g = torch.tensor(gt, device="cuda")
    loss = photometric_loss(x, g, w1, ws)
    loss.backward()
    return float(loss), x.grad.cpu().numpy()


@pytest.mark.parametrize("i", range(int(GOLD["n"])))
def test_matches_reference_golden(i):
    w1, ws = (float(v) for v in GOLD[f"w{i}"])
    loss, grad = _run(GOLD[f"img{i}"], GOLD[f"gt{i}"], w1, ws)
    assert abs(loss - float(GOLD[f"loss_{i}"])) < VAL_TOL
    assert helpers.rel_l2(grad, GOLD[f"grad_{i}"]) < GRAD_TOL


@pytest.mark.parametrize("C,H,W", [(3, 1080, 1920), (3, 545, 977), (1, 16, 32), (3, 5, 7), (4, 33, 31)])
def test_matches_oracle(C, H, W):
    rng = np.random.default_rng(C * H + W)
    gt = rng.random((C, H, W), dtype=np.float32)
    img = np.clip(0.7 * gt + 0.3 * rng.random((C, H, W), dtype=np.float32), 0, 1).astype(np.float32)
    img[0, : min(H, 4), : min(W, 4)] = gt[0, : min(H, 4), : min(W, 4)]  # exact ties: sign(0) = 0 in the L1 term
    loss, grad = _run(img, gt, 0.8, 0.2)
    ol, _, _, og = LO.photometric_loss(img, gt, 0.8, 0.2)
    assert abs(loss - ol) < VAL_TOL
    assert helpers.rel_l2(grad, og) < GRAD_TOL


def test_reference_call_surface():
    import torch
    from diff_recon_hip import L1, PhotometricLoss, SSIMLoss, ssimLoss

    rng = np.random.default_rng(3)
    a = torch.tensor(rng.random((3, 40, 50), dtype=np.float32), device="cuda", requires_grad=True)
    b = torch.tensor(rng.random((3, 40, 50), dtype=np.float32), device="cuda")
    l1, sl = L1(a, b), ssimLoss(a, b)
    assert l1.dim() == 0 and sl.dim() == 0
    ol, o1, os_, _ = LO.photometric_loss(a.detach().cpu().numpy(), b.cpu().numpy(), 0.8, 0.2, need_grad=False)
    assert abs(float(l1) - o1) < VAL_TOL and abs(float(sl) - os_) < VAL_TOL
    # separate calls combined like VanillaTS_trainer.py:111 == the fused module, values and gradients
    (0.8 * l1 + 0.2 * sl).backward()
    g_sep = a.grad.clone()
    a.grad = None
    fused = PhotometricLoss(0.8, 0.2)(a, b)
    fused.backward()
    assert abs(float(fused) - ol) < VAL_TOL
    assert helpers.rel_l2(a.grad.cpu().numpy(), g_sep.cpu().numpy()) < 1e-6
    # 2-D and 4-D inputs (normalize_shape, trainer_utils.py:80-93); upstream gradient scaling
    a4 = a.detach().reshape(1, 3, 40, 50).clone().requires_grad_(True)
    (3.0 * SSIMLoss()(a4, b.reshape(1, 3, 40, 50))).backward()
    a.grad = None
    ssimLoss(a, b).backward()
    assert helpers.rel_l2(a4.grad.reshape(3, 40, 50).cpu().numpy(), 3.0 * a.grad.cpu().numpy()) < 1e-6
    # L1 with BOTH arguments requiring grad (the trainer's affine regulariser, VanillaTS_trainer.py:103) against torch autograd;
    # the SSIM term differentiates its first argument only and refuses a second argument that requires grad
    x = a.detach().clone().requires_grad_(True)
    y = b.detach().clone().requires_grad_(True)
    (2.0 * L1(x, y)).backward()
    xr = a.detach().clone().requires_grad_(True)
    yr = b.detach().clone().requires_grad_(True)
    (2.0 * torch.abs(xr - yr).mean()).backward()
    assert helpers.rel_l2(x.grad.cpu().numpy(), xr.grad.cpu().numpy()) < 1e-6
    assert helpers.rel_l2(y.grad.cpu().numpy(), yr.grad.cpu().numpy()) < 1e-6
    y.grad = None
    L1(a.detach(), y).backward()  # only the second argument requires grad
    assert helpers.rel_l2(y.grad.cpu().numpy(), 0.5 * yr.grad.cpu().numpy()) < 1e-6
    with pytest.raises(RuntimeError):
        ssimLoss(a, y)
    with pytest.raises(RuntimeError):
        PhotometricLoss(0.8, 0.2)(a, y)
    with pytest.raises(ValueError):
        L1(a, b[:, :10])
    with pytest.raises(RuntimeError):
        L1(a.detach().cpu(), b.cpu())


def test_triangle_renderer_shim():
    """diff_recon_hip.TriangleRenderer packs the same dict as the reference's (triangle_renderer.py:77-95), 2D and 3D."""
    import torch
    import synthetic
    from diff_recon_hip import TriangleRenderer

    s = synthetic.scene(800, 96, 64, 1, seed=4)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    class Cam:
        image_width, image_height = 96, 64
        tan_fovx, tan_fovy = s["tanfovx"], s["tanfovy"]
        world_view_transform, full_proj_transform, camera_center = t(s["viewmatrix"]), t(s["projmatrix"]), t(s["campos"])
        device = "cuda"

    for kind in ("2D", "3D"):
        r = TriangleRenderer(Cam, sh_degree=1, rich_info=True, rasterizer_type=kind)
        pkg = r.render(t(s["vertex"]).requires_grad_(True), t(s["shs"]), None, t(s["opacity"]))
        assert set(pkg) == {"render", "radii", "center2D", "depth", "normal", "contrib_sum", "contrib_max"}
        assert pkg["render"].shape == (3, 64, 96)
        pkg["render"].sum().backward()
        assert pkg["center2D"].grad is not None
        r2 = TriangleRenderer(Cam, sh_degree=1, rich_info=False, rasterizer_type=kind)
        assert set(r2.render(t(s["vertex"]), t(s["shs"]), None, t(s["opacity"]))) == {"render", "radii", "center2D"}
    with pytest.raises(ValueError):
        TriangleRenderer(Cam, rasterizer_type="4D")


def test_render_view_shim_matches_manual_pipeline():
    """diff_recon_hip.render_view (VanillaTS_model.py:585-694): up-scaled render + bilinear resize, gamma rescale, STE
    opacity and bg_depth must equal the same steps done by hand around the rasterizer package."""
    import copy
    import torch
    import torch.nn.functional as F
    import synthetic
    from diff_recon_hip import TriangleRenderer, gamma_rescale_ratio, render_view

    s = synthetic.scene(1500, 80, 48, 1, seed=12, max_degree=2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    class Cam:
        pass

    cam = Cam()
    cam.image_width, cam.image_height = 80, 48
    cam.tan_fovx, cam.tan_fovy = s["tanfovx"], s["tanfovy"]
    cam.world_view_transform, cam.full_proj_transform, cam.camera_center = t(s["viewmatrix"]), t(s["projmatrix"]), t(s["campos"])
    cam.device = "cuda"
    vertex = t(s["vertex"]).requires_grad_(True)
    shs = t(s["shs"])
    f_dc, f_rest = shs[:, :1].clone().requires_grad_(True), shs[:, 1:].clone().requires_grad_(True)
    raw_op = torch.logit(t(s["opacity"]).clamp(0.02, 0.98)).requires_grad_(True)
    bg = torch.tensor([0.1, 0.2, 0.3])
    kw = dict(bg_color=bg, gamma=2.0, active_sh_degree=1, max_sh_degree=2, gamma_rescale=True, ste_threshold=0.3,
              render_up_scale=2, rasterizer_type="2D")
    pkg = render_view(cam, vertex, f_dc, f_rest, raw_op, is_training=True, **kw)
    assert pkg["render"].shape == (3, 48, 80) and pkg["depth"].shape == (48, 80) and pkg["normal"].shape == (3, 48, 80)
    assert set(pkg) == {"render", "radii", "center2D", "contrib_sum", "contrib_max", "depth", "normal", "opacity", "vertex",
                        "visible_mask"}
    # by hand
    op = torch.sigmoid(raw_op)
    ratio = gamma_rescale_ratio(2.0)
    c = vertex.mean(1, keepdim=True)
    v2 = (vertex - c) * ratio + c
    o2 = ((op > 0.3).float() - op).detach() + op
    cam2 = copy.copy(cam)
    cam2.image_width, cam2.image_height = 160, 96
    bgd = (cam.camera_center.view(1, 1, 3) - vertex).norm(dim=-1).max()
    r = TriangleRenderer(cam2, bg_depth=bgd, bg_color=bg, sh_degree=1, gamma=2.0, rich_info=True, rasterizer_type="2D")
    out = r.render(v2, torch.cat((f_dc, f_rest), 1), None, o2)
    want = F.interpolate(out["render"].unsqueeze(0), size=(48, 80), mode="bilinear").squeeze(0)
    assert helpers.rel_l2(pkg["render"].detach().cpu().numpy(), want.detach().cpu().numpy()) < 1e-6
    assert torch.equal(pkg["radii"], out["radii"] // 2)
    # gradients flow to the model tensors through rescale / STE / sigmoid and to center2D
    pkg["render"].sum().backward()
    assert vertex.grad.abs().sum() > 0 and raw_op.grad.abs().sum() > 0 and f_dc.grad.abs().sum() > 0
    assert f_rest.grad[:, 3:].abs().sum() == 0  # coefficients above the active degree receive exact zeros
    assert pkg["center2D"].grad is not None
    # evaluation mode: 2-tuple path, only the image
    ev = render_view(cam, vertex, f_dc, f_rest, raw_op, is_training=False, **kw)
    assert set(ev) == {"render"}


@pytest.mark.parametrize("P", [0, 1, 85, 4099, 700001])
def test_background_depth_equals_the_torch_expression(P):
    """VanillaTS_model.py:623.  One kernel in place of subtract / norm / max; the sum of squares is formed in the order x, y, z without contraction, so
    the difference to torch's vector norm is at most the last bit of the square root."""
    import torch
    from diff_recon_hip import background_depth
    g = torch.Generator().manual_seed(P)
    vertex = (torch.randn(P, 3, 3, generator=g) * 7.0).cuda()
    campos = torch.tensor([0.3, -2.0, 11.0], device="cuda")
    got = background_depth(vertex, campos)
    assert got.shape == () and got.is_cuda and not got.requires_grad
    if P == 0:
        assert float(got) == 0.0
        return
    want = (campos.view(1, 1, 3) - vertex).norm(dim=-1).max()
    assert abs(float(got) - float(want)) <= 2.0 * np.spacing(np.float32(float(want)))
    # a vertex tensor that requires grad (the model's parameter) gives the same number and no graph
    assert float(background_depth(vertex.requires_grad_(True), campos)) == float(got)


@pytest.mark.parametrize("P", [85, 700001])
@pytest.mark.parametrize("bad", ["nan", "inf", "nan_and_inf"])
def test_background_depth_follows_the_torch_expression_through_non_finite_vertices(P, bad):
    """VanillaTS_model.py:623 on a diverged model: torch's max over the distances is NaN as soon as one distance is NaN, and inf when one
    coordinate is infinite.  The kernel's running maximum must not drop a NaN (fmaxf would, and the depth image would stay finite)."""
    import torch
    from diff_recon_hip import background_depth
    g = torch.Generator().manual_seed(P)
    vertex = (torch.randn(P, 3, 3, generator=g) * 7.0)
    if bad in ("nan", "nan_and_inf"):
        vertex[P // 3, 1, 2] = float("nan")  # one coordinate of one vertex, inside the range of some block other than the first
    if bad in ("inf", "nan_and_inf"):
        vertex[P - 1, 2, 0] = float("inf")  # the last vertex of the array
    vertex = vertex.cuda()
    campos = torch.tensor([0.3, -2.0, 11.0], device="cuda")
    got = float(background_depth(vertex, campos))
    want = float((campos.view(1, 1, 3) - vertex).norm(dim=-1).max())
    assert (want != want) == (bad != "inf") and (want == float("inf")) == (bad == "inf")  # the torch expression itself: NaN wins over inf
    if want != want:
        assert got != got, got
    else:
        assert got == want, (got, want)


def _dn_golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_normal.npz"))


@pytest.mark.parametrize("i", range(6))
def test_depth_normal_loss_matches_reference_golden(i):
    """The fused DepthNormalLoss (csrc/depth_normal.hip through include/ts_loss.h) against the reference's own class + autograd
    (tests/golden/depth_normal.npz): loss to 1e-5 relative, gradients to 1e-4 relative L2 (float32 on both sides)."""
    import torch
    from diff_recon_hip import DepthNormalLoss
    z = _dn_golden()
    H, W, s, q, tx, ty = z["cases"][i]
    d = torch.from_numpy(z[f"depth{i}"]).cuda().requires_grad_(True)
    n = torch.from_numpy(z[f"normal{i}"]).cuda().requires_grad_(True)
    loss = DepthNormalLoss(scale_factor=None if s < 0 else float(s), depth_grad_filter_quantile=float(q))(d, n, float(tx), float(ty))
    (2.5 * loss).backward()
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    assert abs(float(loss) - float(z[f"loss{i}"])) < 1e-5 * abs(float(z[f"loss{i}"]))
    assert rel(d.grad.cpu().numpy() / 2.5, z[f"ddepth{i}"]) < 1e-4
    assert rel(n.grad.cpu().numpy() / 2.5, z[f"dnormal{i}"]) < 1e-4


def test_depth_normal_loss_full_size_against_oracle_and_flags():
    """1080p (the BASELINE configs[4] image size) against the float64 oracle; depth_grad / normal_grad = False drop the respective
    gradient like the reference's detach(); CPU tensors are refused (no fallback)."""
    import torch
    from diff_recon_hip import DepthNormalLoss
    from oracle import ts_loss_oracle as O
    rng = np.random.default_rng(3)
    H, W = 1080, 1920
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    depth = (8.0 + 3.0 * np.sin(5 * xx) * np.cos(4 * yy) + 2.0 * (xx > 0.6) + 0.02 * rng.standard_normal((H, W))).astype(np.float32)
    normal = (rng.standard_normal((3, H, W)) * 0.2 + np.array([0.0, 0.1, -1.0])[:, None, None]).astype(np.float32)
    d = torch.from_numpy(depth).cuda().requires_grad_(True)
    n = torch.from_numpy(normal).cuda().requires_grad_(True)
    loss = DepthNormalLoss(scale_factor=0.5)(d, n, 0.3148, 0.3148 * H / W)
    loss.backward()
    aux = {}
    want, dd, dn = O.depth_normal_loss(depth, normal, 0.3148, 0.3148 * H / W, 0.5, 0.9, aux=aux)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    assert abs(float(loss) - want) < 1e-5 * abs(want)
    # The mask is a hard threshold (G < quantile(G, 0.9), trainer_utils.py:240-241): among two million pixels a few sit within float32
    # rounding of it and land on the other side in a float32 evaluation (the reference's own included); each carries its whole per-pixel
    # gradient (measured: 8 of 2 073 600 pixels, up to 1.7e-5 of the threshold away; without them the gradients agree to 1.6e-5).  Pixels
    # with |G - thr| < 1e-4 thr are set aside, everything else must agree.
    tie = np.abs(aux["G"] - aux["threshold"]) < 1e-4 * aux["threshold"]
    assert tie.sum() < 2000
    gn = n.grad.cpu().numpy()
    assert rel(gn[:, ~tie], dn[:, ~tie]) < 1e-4
    # dL/ddepth spreads every pixel's term over its neighbours (up-sampling, Scharr and down-sampling adjoints) and is a sum of differences
    # of nearly equal terms: float32 against the float64 oracle sits at ~5e-4 at this size (against the reference's own float32 autograd
    # the small cases above agree to 1e-4)
    assert rel(d.grad.cpu().numpy(), dd) < 1e-3
    d2 = torch.from_numpy(depth).cuda().requires_grad_(True)
    n2 = torch.from_numpy(normal).cuda().requires_grad_(True)
    DepthNormalLoss(depth_grad=False, scale_factor=0.5)(d2, n2, 0.3148, 0.3148 * H / W).backward()
    assert d2.grad is None and rel(n2.grad.cpu().numpy()[:, ~tie], dn[:, ~tie]) < 1e-4
    with pytest.raises(RuntimeError):
        DepthNormalLoss(scale_factor=0.5)(torch.from_numpy(depth), torch.from_numpy(normal), 0.3, 0.2)


@pytest.mark.parametrize("i", range(5))
def test_aux_losses_match_reference_golden(i):
    """DoGLoss / SmoothnessLoss (csrc/aux_losses.hip through include/ts_loss.h) against the reference's own classes + autograd
    (tests/golden/aux_losses.npz): the masks pixel for pixel except where a float32 pipeline may put a value on the other side of its
    threshold (a handful of pixels, counted), the losses and gradients ON the reference's mask to 1e-5 / 1e-4, and the classes end to end."""
    import torch
    from diff_recon_hip import DoGLoss, SmoothnessLoss
    from diff_recon_hip.losses import _MaskedL1, _ScharrSmoothness
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "aux_losses.npz"))
    C, H, W, s, freq, q = z["cases"][i]
    C, H, W, freq = int(C), int(H), int(W), int(freq)
    s = None if s < 0 else float(s)
    gt = torch.from_numpy(z[f"gt{i}"]).cuda()
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    dog, smo = DoGLoss(freq=freq, scale_factor=s), SmoothnessLoss(quantile=float(q), scale_factor=s)
    for name, mod, fn in (("dog", dog, _MaskedL1), ("smooth", smo, _ScharrSmoothness)):
        m = mod.mask(gt).cpu().numpy()
        ref_m = z[f"{name}_mask{i}"]
        assert set(np.unique(m)) <= {0.0, 1.0} and (m != ref_m).mean() < 3e-3, (name, float((m != ref_m).mean()))
        # loss and gradient on the reference's mask: the differentiable part alone
        x = torch.from_numpy(z[f"img{i}"]).cuda().requires_grad_(True)
        ws, _ = mod._workspace(gt, C, H, W)
        rm = torch.from_numpy(ref_m).cuda()
        loss = fn.apply(x, gt, rm, C, H, W, ws) if name == "dog" else fn.apply(x, rm, C, H, W, ws)
        (1.5 * loss).backward()
        want = float(z[f"{name}_loss{i}"])
        assert abs(float(loss) - want) < 1e-5 * want, (name, float(loss), want)
        assert rel(x.grad.cpu().numpy() / 1.5, z[f"{name}_grad{i}"]) < 1e-4, name
        # the class end to end (its own mask): within what the few differing mask pixels can move
        x2 = torch.from_numpy(z[f"img{i}"]).cuda().requires_grad_(True)
        l2 = mod(x2, gt)
        l2.backward()
        assert abs(float(l2) - want) < 5e-3 * want and rel(x2.grad.cpu().numpy(), z[f"{name}_grad{i}"]) < 8e-2, name


def test_aux_losses_full_size_against_oracle_and_surface():
    """1080p against the float64 oracle (on the kernels' own masks), the reference's call surface (batch dimension, module-level instances), and the
    refusals: CPU tensors, a target that requires grad, more than 8 folded channels."""
    import torch
    from diff_recon_hip import DoGLoss, SmoothnessLoss, dogLoss, smoothnessLoss
    rng = np.random.default_rng(5)
    H, W = 1080, 1920
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    gt = np.clip(0.5 + 0.3 * np.sin(40 * xx) * np.cos(25 * yy) + 0.05 * rng.standard_normal((3, H, W)), 0, 1).astype(np.float32)
    img = np.clip(gt + 0.05 * rng.standard_normal((3, H, W)), 0, 1).astype(np.float32)
    g = torch.from_numpy(gt).cuda()
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    for mod, ofn in ((dogLoss, LO.dog_loss), (smoothnessLoss, LO.smoothness_loss)):
        x = torch.from_numpy(img).cuda().requires_grad_(True)
        loss = mod(x[None], g[None])  # (B, C, H, W) like the trainer's call
        loss.backward()
        m = mod.mask(g).cpu().numpy().astype(np.float64)
        assert set(np.unique(m)) <= {0.0, 1.0} and 0.0 < m.mean() < 1.0  # (the DoG mask of a smooth image is mostly 1: the zero padding puts the extremes at the border)
        want, wgrad = ofn(img, gt, mask=m)
        assert abs(float(loss) - want) < 1e-5 * want and rel(x.grad.cpu().numpy(), wgrad) < 1e-4
    # a constant image: every Scharr response cancels to an exact 0 in the kernels' fixed summation order, the norm's gradient there is 0 (torch's
    # norm backward; the reference's own float32 convolution leaves rounding noise in such regions and differentiates THAT)
    flat = torch.full((3, 64, 96), 0.37, device="cuda", requires_grad=True)
    l = SmoothnessLoss()(flat, g[:, :64, :96].contiguous())
    l.backward()
    assert float(flat.grad[:, 3:-3, 3:-3].abs().max()) == 0.0  # (the zero padding gives the image's border a real gradient)
    with pytest.raises(RuntimeError, match="HIP device"):
        DoGLoss()(torch.zeros(3, 8, 8), torch.zeros(3, 8, 8))
    with pytest.raises(RuntimeError, match="must not require grad"):
        SmoothnessLoss()(torch.zeros(3, 8, 8, device="cuda"), torch.zeros(3, 8, 8, device="cuda", requires_grad=True))
    with pytest.raises(RuntimeError, match="at most 8 channels"):
        DoGLoss()(torch.zeros(3, 3, 8, 8, device="cuda"), torch.zeros(3, 3, 8, 8, device="cuda"))


@pytest.mark.parametrize("shape,factor", [((3, 64, 96), 2), ((1, 30, 45), 3), ((2, 3, 40, 56), 4), ((3, 1600, 1600), 2), ((16, 24), 2)])
def test_downsample_bilinear_equals_interpolate_and_its_autograd(shape, factor):
    """Round 6: the resize behind a render at render_up_scale x the resolution (VanillaTS_model.py:649-656, F.interpolate(..., mode="bilinear")) as
    one gather kernel each way (csrc/resample.hip) -- against torch's own kernels: forward to 1 ulp-ish, backward against autograd (whose
    upsample_bilinear2d_backward scatters with atomics)."""
    import torch
    import torch.nn.functional as F
    from diff_recon_hip import downsample_bilinear
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(shape, device="cuda", generator=g).requires_grad_(True)
    H, W = shape[-2:]
    h, w = H // factor, W // factor
    y = downsample_bilinear(x, (h, w))
    x4 = x.reshape((1, -1, H, W)) if x.dim() != 4 else x
    ref = F.interpolate(x4, size=(h, w), mode="bilinear").reshape(y.shape)
    assert y.shape == tuple(shape[:-2]) + (h, w)
    assert float((y - ref).abs().max()) < 2e-7
    up = torch.rand(y.shape, device="cuda", generator=g)
    (gx,) = torch.autograd.grad(y, x, up)
    (gr,) = torch.autograd.grad(ref, x, up)
    assert float((gx - gr).abs().max()) < 2e-7
    with pytest.raises(RuntimeError):
        downsample_bilinear(x, (h + 1, w))  # not an integer factor


@pytest.mark.parametrize("H,W,factor", [(96, 160, 2), (90, 150, 3), (94, 158, 2)])
def test_downsample_bilinear_many_is_the_single_tensor_kernel_on_every_tensor(H, W, factor):
    """Round 6: the render (3), depth (1) and normal (3) images of a step through ONE launch each way (tsl_downsample_*_planes; nine planes here:
    more than a launch holds) -- the same bits as downsample_bilinear on each tensor, gradients included; an output nobody differentiates hands
    its input None (the rasterizer's backward then takes its colour-only form), not zeros."""
    import torch
    from diff_recon_hip import downsample_bilinear, downsample_bilinear_many
    g = torch.Generator(device="cuda").manual_seed(H)
    buf = torch.rand(H * W + 1, device="cuda", generator=g)
    # three tensors that are not contiguous with each other; the second starts 4 bytes off an 8-byte boundary (the factor-2 kernel's float2 loads
    # need that alignment: the launch falls back to the general kernel, same bits)
    xs = [torch.rand((3, H, W), device="cuda", generator=g).requires_grad_(True), buf[1:].view(H, W).detach().requires_grad_(True),
          torch.rand((5, H, W), device="cuda", generator=g).requires_grad_(True)]
    h, w = H // factor, W // factor
    many = downsample_bilinear_many(xs, (h, w))
    single = [downsample_bilinear(x, (h, w)) for x in xs]
    assert [tuple(m.shape) for m in many] == [(3, h, w), (h, w), (5, h, w)]
    for m, s1 in zip(many, single):
        assert torch.equal(m, s1)
    ups = [torch.rand(m.shape, device="cuda", generator=g) for m in many]
    gm = torch.autograd.grad(many, xs, ups)
    gs = torch.autograd.grad(single, xs, ups)
    for a, b in zip(gm, gs):
        assert torch.equal(a, b)
    # only the first output is differentiated: the others' inputs get no gradient at all
    many = downsample_bilinear_many(xs, (h, w))
    got = torch.autograd.grad(many[0].sum(), xs, allow_unused=True)
    assert got[0] is not None and got[1] is None and got[2] is None
