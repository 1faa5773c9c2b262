"""GPU tests of the trainer's regularisers and the per-view colour affine (csrc/regularizers.hip, diff_recon_hip/regularizers.py): parity with
the reference's own outputs (tests/golden/regularizers.npz), with torch autograd in float64 at training sizes, run-to-run identity, the
schedule of TrainerRegularizers on the native calls, graph capture, and an end-to-end recovery of known per-view colour transforms."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regularizers.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _u32(idx):
    return torch.from_numpy(np.ascontiguousarray(idx.astype(np.int32))).to(DEV).view(torch.uint32)


def _schedule(cfg, it):
    w_s, q, l, qs, ls, wv, vs, vi = cfg
    mode, w_o = ("none", 0.0) if it <= qs else (("quad", q) if it <= ls else ("linear", l))
    return w_s, mode, w_o, (wv if it > vs else 0.0)


def _close_to_max(got, ref, rel):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(got - ref).max() / scale
    assert err <= rel, f"max error {err:.3e} of the largest element (limit {rel})"


# ---- torch float64 statement of the same expressions (VanillaTS_model.py:72-76, VanillaTS_trainer.py:87-97, trainer_utils.py:339-346) -------
def torch_reg(vertex, opacity, nearest_long, w_s, mode, w_o, w_v):
    l1 = (vertex[:, 2] - vertex[:, 1]).norm(dim=1)
    l2 = (vertex[:, 0] - vertex[:, 2]).norm(dim=1)
    l3 = (vertex[:, 1] - vertex[:, 0]).norm(dim=1)
    loss = w_s * torch.stack((l1, l2, l3), dim=1).mean(dim=1).mean()
    if mode == "quad":
        loss = loss + w_o * (0.25 - (opacity - 0.5) ** 2).mean()
    elif mode == "linear":
        loss = loss + w_o * (1 - opacity).mean()
    if w_v:
        pc = vertex.view(-1, 3)
        loss = loss + w_v * ((pc - pc[nearest_long]) ** 2).sum(dim=1).mean()
    return loss


# ---- fixture parity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(10))
def test_fixture_parity(gold, k):
    from diff_recon_hip import triangle_regularization
    name, cfg, it = str(gold["case_names"][k]), gold["case_cfg"][k], int(gold["case_iter"][k])
    w_s, mode, w_o, w_v = _schedule(cfg, it)
    v = _t(gold["vertex"]).requires_grad_(True)
    o = _t(gold["opacity"]).requires_grad_(True)
    total, parts = triangle_regularization(v, o, _u32(gold["nearest"]), w_scaling=w_s, w_opacity=w_o, opacity_mode=mode, w_vertex=w_v)
    total.backward()
    ref = float(gold[f"loss_{name}_f64"])
    assert abs(float(total.detach()) - ref) <= 1e-6 * abs(ref)
    vref = float(gold[f"vertex_loss_{name}_f64"])
    assert abs(float(parts[3]) - vref) <= 1e-6 * abs(vref)
    _close_to_max(v.grad.cpu().numpy(), gold[f"dvertex_{name}_f64"], 1e-5)
    if w_o:
        _close_to_max(o.grad.cpu().numpy(), gold[f"dopacity_{name}_f64"], 1e-5)
    else:
        assert torch.count_nonzero(o.grad) == 0


def test_fixture_parts_and_degenerate_sides(gold):
    from diff_recon_hip import triangle_regularization
    v = _t(gold["vertex"])
    o = _t(gold["opacity"])
    _, parts = triangle_regularization(v, o, _u32(gold["nearest"]), w_scaling=1.0, w_opacity=1.0, opacity_mode="quad", w_vertex=1.0)
    p = parts.cpu().numpy().astype(np.float64)
    assert abs(p[1] - gold["scaling_f64"].mean()) <= 1e-6 * gold["scaling_f64"].mean()
    assert abs(p[3] - gold["dist2_f64"].mean()) <= 1e-6 * gold["dist2_f64"].mean()
    # a triangle with all three vertices at one point and the fixture's zero-side triangle: exactly 0 through a zero side
    d = int(gold["degenerate"])
    vv = gold["vertex"].copy()
    vv[0] = vv[0, 0]
    vt = _t(vv).requires_grad_(True)
    total, _ = triangle_regularization(vt, None, None, w_scaling=1.0)
    total.backward()
    assert torch.count_nonzero(vt.grad[0]) == 0
    g = vt.grad[d].double().cpu().numpy()
    x = vv[d].astype(np.float64)
    e1, e2 = x[0] - x[2], x[1] - x[2]  # the sides that do not vanish; the zero side v2 - v1 adds nothing
    np.testing.assert_allclose(g[0], e1 / np.linalg.norm(e1) / (3 * len(vv)), rtol=1e-5)
    np.testing.assert_allclose(g[1], e2 / np.linalg.norm(e2) / (3 * len(vv)), rtol=1e-5)


@pytest.mark.parametrize("m", [0, 1])
def test_fixture_colour_affine(gold, m):
    from diff_recon_hip import ColorAffine, affine_reg
    uid = int(gold["uid"])
    ca = ColorAffine(gold["weight"].shape[0], device=DEV)
    with torch.no_grad():
        ca.weight.copy_(_t(gold["weight"]))
        ca.bias.copy_(_t(gold["bias"]))
    x = _t(gold[f"x{m}"]).requires_grad_(True)
    mask = _t(gold[f"mask{m}"]) if f"mask{m}" in gold else None
    y = ca(x, uid)
    np.testing.assert_allclose(y.detach().cpu().numpy(), gold[f"y{m}_f64"], rtol=0, atol=1e-6)
    areg = affine_reg(y, x, mask)
    assert abs(float(areg.detach()) - float(gold[f"affine_reg{m}_f64"])) <= 1e-6 * float(gold[f"affine_reg{m}_f64"])
    L = areg + (y * _t(gold[f"R{m}"])).sum()
    L.backward()
    _close_to_max(x.grad.cpu().numpy(), gold[f"dx{m}_f64"], 1e-5)
    _close_to_max(ca.weight.grad.cpu().numpy(), gold[f"dweight{m}_f64"], 1e-5)
    _close_to_max(ca.bias.grad.cpu().numpy(), gold[f"dbias{m}_f64"], 1e-5)
    others = [i for i in range(ca.weight.shape[0]) if i != uid]
    assert torch.count_nonzero(ca.weight.grad[others]) == 0 and torch.count_nonzero(ca.bias.grad[others]) == 0


# ---- training size ---------------------------------------------------------------------------------------------------------------------------
def _scene(P, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    c = torch.rand((P, 1, 3), device=DEV, generator=g) * 4 - 2
    v = c + 0.01 * torch.randn((P, 3, 3), device=DEV, generator=g)
    o = torch.rand((P, 1), device=DEV, generator=g)
    return v.contiguous(), o


@pytest.fixture(scope="module")
def big():
    from simple_knn import nearestNeighbor
    P = 1_000_000
    v, o = _scene(P, 5)
    v[1::97] = v[1::97][:, [0, 2, 1]].clone()  # some coincident vertices from twins of neighbours
    v[2::97] = v[1::97][: v[2::97].shape[0]]
    nearest = nearestNeighbor(v.view(-1, 3), 3)
    hub = nearest.view(torch.int32).clone()
    src = torch.arange(300, 300 + 3 * 250, 3, device=DEV)  # 250 vertices of 250 different triangles share one target (vertex 5)
    hub[src] = 5
    hub = hub.view(torch.uint32)
    torch.cuda.synchronize()
    return v, o, nearest, hub


@pytest.mark.parametrize("which", ["knn", "hub"])
@pytest.mark.parametrize("mode", ["quad", "linear"])
def test_training_size_matches_torch_float64(big, which, mode):
    from diff_recon_hip import triangle_regularization
    v, o, nearest, hub = big
    nn_idx = nearest if which == "knn" else hub
    if which == "hub":
        counts = torch.bincount(nn_idx.view(torch.int32).long(), minlength=v.numel() // 3)
        assert int(counts.max()) >= 100
    w_s, w_o, w_v = 0.3, 0.05, 5.0
    vg, og = v.clone().requires_grad_(True), o.clone().requires_grad_(True)
    total, parts = triangle_regularization(vg, og, nn_idx, w_scaling=w_s, w_opacity=w_o, opacity_mode=mode, w_vertex=w_v)
    total.backward()
    v64, o64 = v.double().requires_grad_(True), o.double().requires_grad_(True)
    ref = torch_reg(v64, o64, nn_idx.view(torch.int32).long(), w_s, mode, w_o, w_v)
    ref.backward()
    assert abs(float(total.detach()) - float(ref.detach())) <= 1e-6 * abs(float(ref.detach()))
    _close_to_max(vg.grad.cpu().numpy(), v64.grad.cpu().numpy(), 1e-5)
    _close_to_max(og.grad.cpu().numpy(), o64.grad.cpu().numpy(), 1e-5)
    pc = v64.detach().view(-1, 3)
    vr = float(((pc - pc[nn_idx.view(torch.int32).long()]) ** 2).sum(1).mean())
    assert abs(float(parts[3]) - vr) <= 1e-6 * vr


def test_nan_input_makes_the_loss_nan(big):
    from diff_recon_hip import triangle_regularization
    v, o, nearest, _ = big
    v2 = v.clone()
    v2[123, 1, 2] = float("nan")
    for kw in (dict(w_scaling=1.0), dict(w_vertex=1.0)):
        total, _ = triangle_regularization(v2, o, nearest, **kw)
        assert torch.isnan(total)
    o2 = o.clone()
    o2[7] = float("nan")
    total, _ = triangle_regularization(v, o2, None, w_opacity=1.0, opacity_mode="linear")
    assert torch.isnan(total)


# ---- determinism -----------------------------------------------------------------------------------------------------------------------------
def test_backward_is_run_to_run_identical(big):
    from diff_recon_hip import ColorAffine, prepare_nearest, triangle_regularization
    v, o, _, hub = big
    prep = prepare_nearest(hub)
    grads = []
    for _ in range(2):
        vg, og = v.clone().requires_grad_(True), o.clone().requires_grad_(True)
        total, _ = triangle_regularization(vg, og, hub, w_scaling=0.3, w_opacity=0.05, opacity_mode="quad", w_vertex=5.0, prepared=prep)
        total.backward()
        grads.append((total.detach().clone(), vg.grad, og.grad))
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    ca = ColorAffine(3, device=DEV)
    x = torch.rand((3, 1080, 1920), device=DEV) * 1.4 - 0.2
    R = torch.randn_like(x)
    res = []
    for _ in range(2):
        ca.zero_grad()
        xg = x.clone().requires_grad_(True)
        (ca(xg, 1) * R).sum().backward()
        res.append((xg.grad, ca.weight.grad.clone(), ca.bias.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ---- schedule on the native calls ------------------------------------------------------------------------------------------------------------
def test_schedule_switches_and_cache_refresh_on_the_gpu():
    from simple_knn import nearestNeighbor
    from diff_recon_hip import TrainerRegularizers
    calls = []

    def counting(pts, bs):
        calls.append(pts.shape[0])
        return nearestNeighbor(pts, bs)

    cfg = types.SimpleNamespace(w_scaling_reg=0.0, w_affine_reg=0.0,
                                w_opacity_reg=types.SimpleNamespace(quad_reg=0.01, linear_reg=0.02, quad_start_iter=6000, linear_start_iter=9000),
                                vertex_reg=types.SimpleNamespace(w_vertex_reg=0.5, start_iter=9001, interval_iter=10))
    reg = TrainerRegularizers(cfg, nearest_fn=counting)
    v, o = _scene(4000, 9)
    o64 = o.double()
    quad, lin = float(0.01 * (0.25 - (o64 - 0.5) ** 2).mean()), float(0.02 * (1 - o64).mean())
    pkg = {"vertex": v, "opacity": o}
    assert reg(6000, pkg) == 0.0
    for it, want in ((6001, quad), (9000, quad)):
        got = float(reg(it, pkg))
        assert abs(got - want) <= 1e-6 * want, it
    assert calls == [] and pkg["vertex_loss"] == 0
    got = reg(9001, pkg)
    assert abs(float(got) - lin) <= 1e-6 * lin and calls == []  # the vertex term starts AFTER start_iter
    refreshed = []
    for it in range(9002, 9025):
        n = len(calls)
        reg(it, pkg)
        if len(calls) > n:
            refreshed.append(it)
        assert float(pkg["vertex_loss"]) > 0
    assert refreshed == [9002, 9011, 9021]  # empty cache, then (iteration - 1) % 10 == 0
    v2, o2 = _scene(5000, 10)
    reg(9025, {"vertex": v2, "opacity": o2})  # P changed between refreshes
    assert calls[-1] == 15000 and len(calls) == 4


# ---- colour affine at image sizes ----------------------------------------------------------------------------------------------------------
def _torch_affine(x, W, b, uid):
    return (x.permute(1, 2, 0) @ W[uid] + b[uid]).permute(2, 0, 1).clamp(0, 1)


@pytest.mark.parametrize("hw", [(800, 800), (1080, 1920)])
def test_colour_affine_matches_torch(hw):
    from diff_recon_hip import ColorAffine
    H, W = hw
    V, uid = 5, 3
    torch.manual_seed(H)
    ca = ColorAffine(V, device=DEV)
    Wq = torch.tensor([[0.75, 0.125, -0.0625], [0.0625, 1.125, 0.0], [-0.125, 0.0625, 0.875]], device=DEV)
    with torch.no_grad():
        ca.weight.add_(0.05 * torch.randn_like(ca.weight))
        ca.weight[uid] = Wq
        ca.bias.copy_(0.03 * torch.randn_like(ca.bias))
        ca.bias[uid] = torch.tensor([0.0625, -0.0625, 0.125], device=DEV)
    x = torch.rand((3, H, W), device=DEV) * 1.4 - 0.2
    x[:, 0, :64] = torch.tensor([1.25, 0.0, 0.0], device=DEV)[:, None]   # channel 0 exactly 1
    x[:, 1, :64] = torch.tensor([-0.125, 0.5, 0.0], device=DEV)[:, None]  # channel 0 exactly 0
    R = torch.randn((3, H, W), device=DEV)
    xg = x.clone().requires_grad_(True)
    y = ca(xg, uid)
    (y * R).sum().backward()
    Wd, bd = ca.weight.detach(), ca.bias.detach()
    y32 = _torch_affine(x, Wd, bd, uid)
    assert (y - y32).abs().max() <= 1e-6
    x64 = x.double().requires_grad_(True)
    W64, b64 = Wd.double().requires_grad_(True), bd.double().requires_grad_(True)
    pre64 = (x64.permute(1, 2, 0) @ W64[uid] + b64[uid]).permute(2, 0, 1)
    _close_to_max(y.detach().cpu().numpy(), pre64.detach().clamp(0, 1).cpu().numpy(), 1e-6)
    # The clamp decision is the forward's: the pre-clamp value in float32, summed as the kernel sums it.  Among 6 M random pixels a few lie
    # within rounding of 0 or 1, where float32 and float64 may decide differently; the float64 autograd reference takes the forward's decision,
    # and every pixel where the two disagree must lie within 1e-6 of a bound.
    pre32 = torch.stack([((x[0] * Wd[uid, 0, c] + x[1] * Wd[uid, 1, c]) + x[2] * Wd[uid, 2, c]) + bd[uid, c] for c in range(3)])
    inside32 = (pre32 >= 0) & (pre32 <= 1)
    p64 = pre64.detach()
    differ = inside32 != ((p64 >= 0) & (p64 <= 1))
    assert bool((torch.minimum(p64[differ].abs(), (p64[differ] - 1).abs()) < 1e-6).all())
    y64 = torch.where(inside32, pre64, p64.clamp(0, 1))  # torch's clamp where the decisions agree, which is everywhere else
    (y64 * R.double()).sum().backward()
    _close_to_max(xg.grad.cpu().numpy(), x64.grad.cpu().numpy(), 1e-5)
    _close_to_max(ca.weight.grad.cpu().numpy(), W64.grad.cpu().numpy(), 1e-5)
    _close_to_max(ca.bias.grad.cpu().numpy(), b64.grad.cpu().numpy(), 1e-5)
    # boundary pixels take the inclusive clamp gradient: there dL/dx = W[uid] g with nothing masked
    gx_b = xg.grad[:, 0:2, :64]
    want = torch.einsum("kc,chw->khw", Wq, R[:, 0:2, :64])
    assert torch.allclose(gx_b, want, rtol=1e-6, atol=1e-6)
    others = [i for i in range(V) if i != uid]
    assert torch.count_nonzero(ca.weight.grad[others]) == 0 and torch.count_nonzero(ca.bias.grad[others]) == 0


def test_fused_adam_over_the_affine_groups_matches_torch_adam():
    from diff_recon_hip import ColorAffine, FusedAdam
    torch.manual_seed(3)
    a, b = ColorAffine(4, device=DEV), ColorAffine(4, device=DEV)
    x = torch.rand((3, 64, 96), device=DEV)
    R = torch.randn_like(x)
    fa = FusedAdam(a.param_groups(lr=1e-2), lr=0.0, eps=1e-15)
    ta = torch.optim.Adam(b.param_groups(lr=1e-2), lr=0.0, eps=1e-15)
    assert [g["name"] for g in fa.param_groups] == ["color_affine_weight", "color_affine_bias"]
    sched = ColorAffine.lr_schedulers(v_init=1e-2, v_final=1e-4, max_steps=30)
    for step in range(3):
        for opt, m in ((fa, a), (ta, b)):
            for g in opt.param_groups:
                g["lr"] = sched[g["name"]](step)
            (m(x, step % 4) * R).sum().backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
    assert torch.allclose(a.weight, b.weight, rtol=1e-6, atol=1e-7) and torch.allclose(a.bias, b.bias, rtol=1e-6, atol=1e-7)


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_bit_for_bit(big):
    from simple_knn import nearestNeighbor
    from diff_recon_hip import ColorAffine, prepare_nearest, triangle_regularization
    v, o, _, _ = big
    P = 200_000
    v, o = v[:P].clone(), o[:P].clone()
    nearest = nearestNeighbor(v.view(-1, 3), 3)
    prep = prepare_nearest(nearest)
    ca = ColorAffine(3, device=DEV)
    with torch.no_grad():
        ca.weight.add_(0.05)
        ca.bias.sub_(0.02)
    x = torch.rand((3, 256, 320), device=DEV) * 1.2 - 0.1
    R = torch.randn_like(x)
    vg, og, xg = v.clone().requires_grad_(True), o.clone().requires_grad_(True), x.clone().requires_grad_(True)

    def step():
        total, parts = triangle_regularization(vg, og, nearest, w_scaling=0.3, w_opacity=0.05, opacity_mode="quad", w_vertex=5.0, prepared=prep)
        L = total + (ca(xg, 2) * R).sum()
        return (parts,) + torch.autograd.grad(L, [vg, og, xg, ca.weight, ca.bias])

    eager = [t.clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, static):
            assert torch.equal(a, b)


# ---- end to end: recover known per-view colour transforms -----------------------------------------------------------------------------------
def test_colour_affine_recovers_known_per_view_transforms():
    import synthetic
    from diff_recon_hip import L1, ColorAffine, FusedAdam, render_view

    s = synthetic.scene(6000, 192, 128, 1, seed=21)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    cam = types.SimpleNamespace(image_width=192, image_height=128, tan_fovx=s["tanfovx"], tan_fovy=s["tanfovy"],
                                world_view_transform=t(s["viewmatrix"]), full_proj_transform=t(s["projmatrix"]), camera_center=t(s["campos"]),
                                device=DEV)
    vertex = t(s["vertex"])
    shs = t(s["shs"])
    raw_op = torch.logit(t(s["opacity"]).clamp(0.3, 0.98))
    bg = torch.tensor([0.2, 0.5, 0.8])
    V = 3
    rng = np.random.default_rng(4)
    Wstar = np.stack([np.diag(rng.uniform(0.7, 1.2, 3)) + (1 - np.eye(3)) * rng.uniform(-0.1, 0.1, (3, 3)) for _ in range(V)]).astype(np.float32)
    bstar = rng.uniform(-0.05, 0.05, (V, 3)).astype(np.float32)
    Wt, bt = t(Wstar), t(bstar)
    ca = ColorAffine(V, device=DEV)
    with torch.no_grad():
        plain = render_view(cam, vertex, None, None, raw_op, shs=shs, bg_color=bg, is_training=False, rasterizer_type="2D")["render"]
        targets = [_torch_affine(plain, Wt, bt, u) for u in range(V)]
    opt = FusedAdam(ca.param_groups(), lr=0.0, eps=1e-15)
    sched = ColorAffine.lr_schedulers(v_init=1e-2, v_final=1e-4, max_steps=4500)
    for it in range(4500):  # 1500 steps per view
        u = it % V
        for g in opt.param_groups:
            g["lr"] = sched[g["name"]](it)
        pkg = render_view(cam, vertex, None, None, raw_op, shs=shs, bg_color=bg, is_training=False, rasterizer_type="2D", color_affine=(ca, u))
        assert torch.equal(pkg["render_original"], plain)
        L1(pkg["render"], targets[u]).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    err_w = float((ca.weight.detach() - Wt).abs().max())
    err_b = float((ca.bias.detach() - bt).abs().max())
    assert err_w <= 0.02 and err_b <= 0.01, (err_w, err_b)
