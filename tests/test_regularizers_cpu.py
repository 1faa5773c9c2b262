"""CPU tests of the trainer's regularisers and the per-view colour affine (diff_recon_hip/regularizers.py, csrc/regularizers.hip):

  * a float64 numpy restatement of every term and gradient the kernels compute -- in the kernels' form: side-length gradients masked at length 0,
    the neighbour term's backward as a gather over the inverse of the nearest relation (stable sort on (nearest[k], k)) -- pinned against
    tests/golden/regularizers.npz, which the reference's own _get_loss / get_scaling / nearest_dist2 / L1 produced (make_golden_regularizers.py);
  * the schedule and nearest-cache logic of TrainerRegularizers, driven with injected stand-ins for the native calls.
"""
import os
import types

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regularizers.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


# ---- float64 restatement ------------------------------------------------------------------------------------------------------------------
SIDES = ((2, 1), (0, 2), (1, 0))  # get_scaling's sides v3 - v2, v1 - v3, v2 - v1 as (a, b) of e = a - b


def scaling(v):
    return np.mean([np.linalg.norm(v[:, a] - v[:, b], axis=1) for a, b in SIDES], axis=0)


def scaling_grad(v):
    P = v.shape[0]
    g = np.zeros_like(v)
    for a, b in SIDES:
        e = v[:, a] - v[:, b]
        l = np.linalg.norm(e, axis=1, keepdims=True)
        t = np.where(l > 0, e / np.where(l > 0, l, 1.0), 0.0) / (3 * P)  # torch's norm backward: 0 where the norm is 0
        g[:, a] += t
        g[:, b] -= t
    return g


def inverse(nearest):
    """tsl_reg_prepare: (sources in ascending order, run offsets) of the relation k -> nearest[k]."""
    n = nearest.size
    order = np.argsort(nearest, kind="stable")
    off = np.searchsorted(nearest[order], np.arange(n + 1), side="left")
    return order, off


def vertex_reg(v, nearest):
    p = v.reshape(-1, 3)
    return ((p - p[nearest]) ** 2).sum(1).mean()


def vertex_grad(v, nearest):
    p = v.reshape(-1, 3)
    n = p.shape[0]
    inv, off = inverse(nearest)
    g = np.empty_like(p)
    for j in range(n):
        acc = p[j] - p[nearest[j]]
        for k in inv[off[j]:off[j + 1]]:
            acc = acc - (p[k] - p[j])
        g[j] = 2.0 * acc / n
    return g.reshape(v.shape)


def opacity_term(o, mode):
    if mode == "quad":
        return (0.25 - (o - 0.5) ** 2).mean(), -2.0 * (o - 0.5) / o.size
    if mode == "linear":
        return (1.0 - o).mean(), np.full_like(o, -1.0 / o.size)
    return 0.0, np.zeros_like(o)


def schedule(cfg, it):
    w_s, q, l, qs, ls, wv, vs, vi = cfg
    mode, w_o = ("none", 0.0) if it <= qs else (("quad", q) if it <= ls else ("linear", l))
    return w_s, mode, w_o, (wv if it > vs else 0.0)


def affine(x, W, b):
    pre = np.einsum("khw,kc->chw", x, W) + b[:, None, None]
    return pre, np.clip(pre, 0.0, 1.0)


def affine_grads(x, W, b, gy):
    pre, _ = affine(x, W, b)
    g = np.where((pre >= 0.0) & (pre <= 1.0), gy, 0.0)  # torch's clamp backward: bounds included
    return np.einsum("kc,chw->khw", W, g), np.einsum("khw,chw->kc", x, g), g.sum((1, 2))


# ---- pinned against the reference ---------------------------------------------------------------------------------------------------------
def test_fixture_has_the_structures_it_claims(gold):
    v, nearest = gold["vertex"].astype(np.float64), gold["nearest"]
    d = gold["degenerate"]
    assert np.array_equal(v[d, 0], v[d, 1])  # a zero-length side
    p = v.reshape(-1, 3)
    assert (np.linalg.norm(p - p[nearest], axis=1) == 0).sum() >= 60  # coincident vertices (back-face twins)
    assert not np.any(nearest // 3 == np.arange(nearest.size) // 3)  # never the vertex's own triangle
    assert np.bincount(nearest).max() >= 2  # fan-in above one


def test_scaling_and_nearest_dist2_match_the_reference(gold):
    v = gold["vertex"].astype(np.float64)
    np.testing.assert_allclose(scaling(v), gold["scaling_f64"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(scaling(v), gold["scaling_f32"], rtol=1e-6, atol=0)
    p = v.reshape(-1, 3)
    np.testing.assert_allclose(((p - p[gold["nearest"]]) ** 2).sum(1), gold["dist2_f64"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("k", range(10))
def test_every_case_of_get_loss_matches_the_restatement(gold, k):
    name, cfg, it = str(gold["case_names"][k]), gold["case_cfg"][k], int(gold["case_iter"][k])
    v, o, nearest = gold["vertex"].astype(np.float64), gold["opacity"].astype(np.float64), gold["nearest"]
    w_s, mode, w_o, w_v = schedule(cfg, it)
    o_val, o_grad = opacity_term(o, mode)
    vr = vertex_reg(v, nearest) if w_v else 0.0
    loss = w_s * scaling(v).mean() + w_o * o_val + w_v * vr
    dv = w_s * scaling_grad(v) + (w_v * vertex_grad(v, nearest) if w_v else 0.0)
    do = w_o * o_grad
    np.testing.assert_allclose(loss, gold[f"loss_{name}_f64"], rtol=1e-12)
    np.testing.assert_allclose(vr, gold[f"vertex_loss_{name}_f64"], rtol=1e-12)
    for got, key in ((dv, "dvertex"), (do, "dopacity")):
        ref = gold[f"{key}_{name}_f64"]
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * max(np.abs(ref).max(), 1e-300))
        ref32 = gold[f"{key}_{name}_f32"]  # the reference's own float32 run: within float32 rounding of the same numbers
        np.testing.assert_allclose(got, ref32, rtol=0, atol=1e-5 * max(np.abs(ref32).max(), 1e-30))
    np.testing.assert_allclose(loss, gold[f"loss_{name}_f32"], rtol=1e-5)


def test_degenerate_side_contributes_no_gradient(gold):
    v = gold["vertex"].astype(np.float64)
    d = int(gold["degenerate"])
    g = gold["dvertex_scaling_f64"][d]
    # the zero side v2 - v1 gives nothing: what v1 and v2 receive comes from the other two sides only, which share no term with it
    e1, e2 = v[d, 0] - v[d, 2], v[d, 1] - v[d, 2]
    np.testing.assert_allclose(g[0], e1 / np.linalg.norm(e1) / (3 * v.shape[0]), rtol=1e-12)
    np.testing.assert_allclose(g[1], e2 / np.linalg.norm(e2) / (3 * v.shape[0]), rtol=1e-12)


@pytest.mark.parametrize("m", [0, 1])
def test_colour_affine_and_affine_reg_match_the_reference(gold, m):
    x, W, b, uid, R = gold[f"x{m}"].astype(np.float64), gold["weight"].astype(np.float64), gold["bias"].astype(np.float64), int(gold["uid"]), gold[f"R{m}"]
    mask = gold[f"mask{m}"].astype(np.float64) if f"mask{m}" in gold else np.ones((1,) + x.shape[1:])
    pre, y = affine(x, W[uid], b[uid])
    np.testing.assert_allclose(y, gold[f"y{m}_f64"], rtol=0, atol=1e-14)
    assert ((pre == 1.0).sum(), (pre == 0.0).sum()) >= (8, 8)  # exact boundary pixels are present
    d = y * mask - x * mask
    areg = np.abs(d).mean()
    np.testing.assert_allclose(areg, gold[f"affine_reg{m}_f64"], rtol=1e-13)
    gd = np.sign(d) * mask / d.size  # d affine_reg / d y; d / d x (as render_original) = the negative
    gx_aff, gW, gb = affine_grads(x, W[uid], b[uid], gd + R)
    np.testing.assert_allclose(gx_aff - gd, gold[f"dx{m}_f64"], rtol=0, atol=1e-12)
    dW = np.zeros_like(W)
    dW[uid] = gW
    db = np.zeros_like(b)
    db[uid] = gb
    np.testing.assert_allclose(dW, gold[f"dweight{m}_f64"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(db, gold[f"dbias{m}_f64"], rtol=0, atol=1e-10)


# ---- TrainerRegularizers: schedule and cache, with stand-ins for the native calls -----------------------------------------------------------
class Recorder:
    def __init__(self):
        self.nearest_calls, self.prepare_calls, self.reg_calls, self.affine_calls = [], [], [], []

    def nearest(self, pts, bs):
        assert bs == 3
        self.nearest_calls.append(pts.shape[0])
        return torch.arange(pts.shape[0])

    def prepare(self, nearest):
        self.prepare_calls.append(nearest.numel())
        return types.SimpleNamespace(P=nearest.numel() // 3)

    def reg(self, vertex, opacity, nearest, *, w_scaling, w_opacity, opacity_mode, w_vertex, prepared):
        self.reg_calls.append(dict(w_scaling=w_scaling, w_opacity=w_opacity, mode=opacity_mode, w_vertex=w_vertex,
                                   nearest=nearest, prepared=prepared))
        return torch.tensor(1.0), torch.tensor([1.0, 0.1, 0.2, 0.3])

    def affine(self, image, original, mask):
        self.affine_calls.append(mask)
        return torch.tensor(2.0)


CONFIG = types.SimpleNamespace(w_scaling_reg=0.0, w_affine_reg=0.0,
                               w_opacity_reg=types.SimpleNamespace(quad_reg=0.01, linear_reg=0.02, quad_start_iter=6000, linear_start_iter=9000),
                               vertex_reg=types.SimpleNamespace(w_vertex_reg=0.5, start_iter=100, interval_iter=10))


def make(config=CONFIG, **kw):
    from diff_recon_hip.regularizers import TrainerRegularizers
    r = Recorder()
    return TrainerRegularizers(config, nearest_fn=r.nearest, prepare_fn=r.prepare, reg_fn=r.reg, affine_fn=r.affine, **kw), r


def pkg(P=4, original=False):
    d = {"vertex": torch.zeros((P, 3, 3)), "opacity": torch.zeros((P, 1)), "render": torch.zeros((3, 2, 2))}
    if original:
        d["render_original"] = torch.zeros((3, 2, 2))
    return d


def test_opacity_phases_switch_on_the_reference_boundaries():
    t, r = make(vertex_reg=types.SimpleNamespace(w_vertex_reg=0.0, start_iter=0, interval_iter=10))
    expect = {6000: None, 6001: ("quad", 0.01), 9000: ("quad", 0.01), 9001: ("linear", 0.02)}
    for it, e in expect.items():
        n = len(r.reg_calls)
        loss = t(it, pkg())
        if e is None:
            assert len(r.reg_calls) == n and loss == 0.0  # every active weight 0: nothing launched
        else:
            c = r.reg_calls[-1]
            assert (c["mode"], c["w_opacity"]) == e and c["w_vertex"] == 0.0 and c["nearest"] is None


def test_from_a_dict_config_too():
    t, _ = make({"w_scaling_reg": 0.3, "w_opacity_reg": {"quad_reg": 1.0, "linear_reg": 2.0, "quad_start_iter": 5, "linear_start_iter": 7},
                 "vertex_reg": {"w_vertex_reg": 0.0, "start_iter": 1, "interval_iter": 3}, "w_affine_reg": 0.25})
    assert (t.w_scaling_reg, t.opacity_term(6), t.opacity_term(8), t.w_affine_reg) == (0.3, ("quad", 1.0), ("linear", 2.0), 0.25)


def test_vertex_term_starts_after_start_iter_and_refreshes_on_the_reference_rule():
    t, r = make()
    p = pkg()
    t(100, p)
    assert r.nearest_calls == [] and p["vertex_loss"] == 0
    refreshed = []
    for it in range(101, 135):
        n = len(r.nearest_calls)
        t(it, p)
        if len(r.nearest_calls) > n:
            refreshed.append(it)
        assert r.reg_calls[-1]["w_vertex"] == 0.5 and r.reg_calls[-1]["prepared"] is not None
        assert float(p["vertex_loss"]) == pytest.approx(0.3)
    assert refreshed == [101, 111, 121, 131]  # (iteration - 1) % 10 == 0; 101 is also the first use (empty cache)
    assert len(r.prepare_calls) == len(r.nearest_calls)


def test_empty_cache_refreshes_off_the_interval():
    t, r = make()
    t(105, pkg())
    assert r.nearest_calls == [12]


def test_a_change_in_P_refreshes_the_cache():
    t, r = make()
    t(101, pkg(4))
    t(102, pkg(4))
    assert r.nearest_calls == [12]
    t(103, pkg(6))  # densified between two refreshes
    assert r.nearest_calls == [12, 18] and r.prepare_calls == [12, 18]
    assert r.reg_calls[-1]["prepared"].P == 6


def test_affine_reg_only_with_a_render_original():
    cfg = types.SimpleNamespace(**{**vars(CONFIG), "w_affine_reg": 0.5})
    t, r = make(cfg)
    assert t(50, pkg()) == 0.0 and r.affine_calls == []
    m = torch.ones((1, 2, 2))
    loss = t(50, pkg(original=True), gt_mask=m)
    assert r.affine_calls == [m] and r.reg_calls == [] and float(loss) == pytest.approx(1.0)
    loss = t(6001, pkg(original=True))
    assert float(loss) == pytest.approx(1.0 + 0.5 * 2.0) and r.affine_calls[-1] is None
