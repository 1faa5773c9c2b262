"""Generates tests/golden/regularizers.npz from the REFERENCE's own Python code (build container only; the reference never travels):

    python tests/golden/make_golden_regularizers.py

What runs is the reference's:
  * get_scaling of VanillaTSModel (src/diff_recon/models/VanillaTS_model.py:72-76), through make_golden.load_reference_model_class;
  * nearest_dist2 and L1 of src/diff_recon/trainers/trainer_utils.py:323-324, 339-346, through make_golden.load_trainer_utils;
  * VanillaTSTrainer._get_loss itself (src/diff_recon/trainers/VanillaTS_trainer.py:43-117), imported like the model class (package shells with
    the real paths, empty placeholders for third-party modules this image lacks) and called unbound on a stand-in `self` that carries the
    trainer config and the nearest-index cache.  Its image terms are switched off or made exactly 0: w_ssim = w_dog = w_smoothness = 0 and a
    target equal to the render, so L1 = 0 with gradient sign(0) = 0, and the geometry term never starts.  What remains, loss = reg_loss, is
    lines 86-116.  nearest_neighbor (the module-level name _get_loss calls, :108) is replaced by the brute-force search below, because
    simple_knn is a GPU extension.
  * The colour affine of VanillaTSModel.forward (:678-684) cannot run without the renderer, so those four lines are restated one for one in
    color_affine() below.

Nearest indices: brute force in float64 over all 3P vertices, excluding the vertex's own triangle (the batch_size = 3 rule of
simple_knn's nearestNeighbor).  Tie rule: the smallest index among the candidates at the minimal squared distance (np.argmin).  The
inputs have exact ties: back-face twins put two vertices at one point, and a triangle with a zero-length side has two coincident vertices,
both of which are candidates for its twin's vertex.

Stored (f32 = the reference run on float32 tensors, f64 = the same code on float64 copies of the same float32 inputs; gradients by
torch autograd):
  vertex (P, 3, 3), raw_opacity (P, 1), opacity = sigmoid(raw) (P, 1), nearest (3P,) int64, degenerate (index of the zero-side triangle),
  scaling_{f32,f64} = get_scaling;  dist2_{f32,f64} = nearest_dist2(vertex.view(-1, 3), nearest);
  per case c of CASES (config, iteration): loss_c_{dt}, vertex_loss_c_{dt}, dvertex_c_{dt}, dopacity_c_{dt}  (case_names, case_cfg, case_iter);
  colour affine: x{m} (3, H, W), weight (V, 3, 3), bias (V, 3), uid, mask{m} (1, H, W) or absent, R{m} (3, H, W); per m:
      y{m}_{dt} = affine(x), affine_reg{m}_{dt} = the affine_reg line of _get_loss (:98-105), and for L = affine_reg + sum(y * R):
      L{m}_{dt}, dx{m}_{dt}, dweight{m}_{dt}, dbias{m}_{dt}.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (the loaders; not edited here)

# (name, w_scaling_reg, quad_reg, linear_reg, quad_start_iter, linear_start_iter, w_vertex_reg, v_start_iter, v_interval_iter, iteration)
BIG = 10 ** 9
CASES = [
    ("scaling", 1.0, 0.0, 0.0, BIG, BIG, 0.0, 0, 10, 1),
    ("quad", 0.0, 1.0, 0.0, 0, BIG, 0.0, 0, 10, 1),
    ("linear", 0.0, 0.0, 1.0, 0, 0, 0.0, 0, 10, 1),
    ("vertex", 0.0, 0.0, 0.0, BIG, BIG, 1.0, 0, 10, 1),
]
SCHED = (0.3, 0.05, 0.02, 100, 200, 5.0, 150, 10)
for it in (100, 101, 150, 151, 200, 201):
    CASES.append((f"sched{it}",) + SCHED + (it,))


def triangles(rng, P_free=160, P_twin=40):
    v = rng.normal(0.0, 1.0, (P_free, 1, 3)) + 0.08 * rng.normal(0.0, 1.0, (P_free, 3, 3))
    v[7, 1] = v[7, 0]  # triangle 7: zero-length side v2 - v1
    twins = v[:P_twin][:, [0, 2, 1]]  # back-face twins: the same points, opposite winding
    return np.concatenate([v, twins]).astype(np.float32), 7


def brute_nearest(vertex):
    p = vertex.reshape(-1, 3).astype(np.float64)
    n = p.shape[0]
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    own = np.arange(n) // 3
    d2[own[:, None] == own[None, :]] = np.inf
    return np.argmin(d2, axis=1).astype(np.int64)  # first index at the minimum


def load_trainer_class():
    """VanillaTS_trainer.py with the package shells of make_golden.load_reference_model_class (which must have run first) plus the trainers
    package; third-party names this image lacks become empty modules, names imported FROM them become placeholders."""
    root = "/root/reference/src/diff_recon"
    m = types.ModuleType("diff_recon.trainers")
    m.__path__ = [os.path.join(root, "trainers")]
    m.__package__ = "diff_recon.trainers"
    sys.modules["diff_recon.trainers"] = m
    for sub in ("datasets",):
        s = types.ModuleType("diff_recon." + sub)
        s.__path__ = [os.path.join(root, sub)]
        sys.modules["diff_recon." + sub] = s
    for _ in range(200):
        try:
            return importlib.import_module("diff_recon.trainers.VanillaTS_trainer")
        except ModuleNotFoundError as e:
            if e.name is None or e.name.startswith("diff_recon"):
                raise
            sys.modules[e.name] = types.ModuleType(e.name)
        except ImportError as e:  # `from X import Y` out of a placeholder module
            msg = str(e)
            if "cannot import name" not in msg:
                raise
            name = msg.split("'")[1]
            mod = msg.split("from '")[1].split("'")[0]
            if mod.startswith("diff_recon"):
                raise
            setattr(sys.modules[mod], name, type(name, (), {}))
    raise RuntimeError("could not import the reference trainer")


def trainer_config(w_s, q, l, qs, ls, wv, vs, vi, w_a=0.0):
    ns = types.SimpleNamespace
    return ns(w_ssim=0.0, w_dog=0.0, w_smoothness=0.0, w_scaling_reg=w_s, w_affine_reg=w_a,
              vertex_reg=ns(w_vertex_reg=wv, start_iter=vs, interval_iter=vi),
              geometry_loss=ns(start_iter=BIG, w_geometry=0.0),
              w_opacity_reg=ns(quad_reg=q, linear_reg=l, quad_start_iter=qs, linear_start_iter=ls))


def run_get_loss(trainer_mod, cfg, iteration, render_pkg):
    self = types.SimpleNamespace(config=types.SimpleNamespace(trainer=cfg), _nearest_indices_cache=None)
    return trainer_mod.VanillaTSTrainer._get_loss(self, iteration, render_pkg, None)


def color_affine(image, W, b, uid):
    """VanillaTS_model.py:680-683, restated (the model's forward needs the renderer)."""
    image_transformed = (image.permute(1, 2, 0) @ W[uid] + b[uid]).permute(2, 0, 1)
    return image_transformed.clamp(0, 1)


def main():
    model_cls, _ = make_golden.load_reference_model_class()
    tu = make_golden.load_trainer_utils()
    trainer_mod = load_trainer_class()
    rng = np.random.default_rng(31)
    vertex, degenerate = triangles(rng)
    P = vertex.shape[0]
    raw = rng.normal(0.0, 2.0, (P, 1)).astype(np.float32)
    opacity = torch.sigmoid(torch.tensor(raw)).numpy()
    nearest = brute_nearest(vertex)
    trainer_mod.nearest_neighbor = lambda pc, bs=1: torch.tensor(nearest)  # :108 (simple_knn is a GPU extension)
    out = dict(vertex=vertex, raw_opacity=raw, opacity=opacity, nearest=nearest, degenerate=np.int64(degenerate),
               case_names=np.array([c[0] for c in CASES]), case_cfg=np.array([c[1:9] for c in CASES], np.float64),
               case_iter=np.array([c[9] for c in CASES], np.int64))
    for dt, tdt in (("f32", torch.float32), ("f64", torch.float64)):
        fake = types.SimpleNamespace(_vertex=torch.tensor(vertex, dtype=tdt))
        out[f"scaling_{dt}"] = model_cls.get_scaling.fget(fake).numpy()
        out[f"dist2_{dt}"] = tu.nearest_dist2(torch.tensor(vertex, dtype=tdt).view(-1, 3), torch.tensor(nearest)).numpy()
        for c in CASES:
            name, it = c[0], c[9]
            v = torch.tensor(vertex, dtype=tdt, requires_grad=True)
            o = torch.tensor(opacity, dtype=tdt, requires_grad=True)
            img = torch.zeros((3, 4, 4), dtype=tdt)
            # `scaling` is get_scaling of the model's vertices (:72-76); here the same tensor that "vertex" holds
            pkg = {"render": img, "scaling": model_cls.get_scaling.fget(types.SimpleNamespace(_vertex=v)), "opacity": o, "vertex": v,
                   "gt_image": img.clone(), "gt_mask": None, "depth": None, "normal": None}
            loss = run_get_loss(trainer_mod, trainer_config(*c[1:9]), it, pkg)
            if isinstance(loss, torch.Tensor) and loss.requires_grad:
                loss.backward()
            gv = v.grad.numpy().copy() if v.grad is not None else np.zeros_like(vertex, dtype=np.float64 if dt == "f64" else np.float32)
            go = o.grad.numpy().copy() if o.grad is not None else np.zeros_like(opacity, dtype=np.float64 if dt == "f64" else np.float32)
            out[f"loss_{name}_{dt}"] = np.array(float(loss.detach() if isinstance(loss, torch.Tensor) else loss))
            vl = pkg["vertex_loss"]
            out[f"vertex_loss_{name}_{dt}"] = np.array(float(vl.detach() if isinstance(vl, torch.Tensor) else vl))
            out[f"dvertex_{name}_{dt}"], out[f"dopacity_{name}_{dt}"] = gv, go

    # ---- colour affine + affine_reg --------------------------------------------------------------------------------------------------
    H, Wd, V, uid = 24, 32, 4, 2
    weight = np.tile(np.eye(3, dtype=np.float32), (V, 1, 1)) + rng.uniform(-0.1, 0.1, (V, 3, 3)).astype(np.float32)
    weight[uid] = np.array([[0.75, 0.125, -0.0625], [0.0625, 1.125, 0.0], [-0.125, 0.0625, 0.875]], np.float32)  # dyadic: exact boundary pixels
    bias = rng.uniform(-0.05, 0.05, (V, 3)).astype(np.float32)
    bias[uid] = np.array([0.0625, -0.0625, 0.125], np.float32)
    out.update(weight=weight, bias=bias, uid=np.int64(uid))
    for m in range(2):
        x = rng.uniform(-0.2, 1.2, (3, H, Wd)).astype(np.float32)
        # pixels whose pre-clamp value is exactly 1 or 0 (dyadic inputs and weights: every order of summation is exact):
        x[:, 0, 0:4] = np.array([1.25, 0.0, 0.0], np.float32)[:, None]     # channel 0: 1.25 * 0.75 + 0.0625 = 1
        x[:, 1, 0:4] = np.array([-0.125, 0.5, 0.0], np.float32)[:, None]   # channel 0: -0.09375 + 0.03125 + 0.0625 = 0
        x[:, 2, 0:4] = np.array([0.5, 0.875, 0.25], np.float32)[:, None]   # channel 1: 0.0625 + 0.984375 + 0.015625 - 0.0625 = 1
        x[:, 3, 0:4] = np.array([2.0, 0.0, 0.0], np.float32)[:, None]      # channel 2: -0.125 + 0.125 = 0
        R = rng.normal(0.0, 1.0, (3, H, Wd)).astype(np.float32)
        mask = (rng.uniform(0, 1, (1, H, Wd)) > 0.3).astype(np.float32) if m == 1 else None
        out[f"x{m}"], out[f"R{m}"] = x, R
        if mask is not None:
            out[f"mask{m}"] = mask
        for dt, tdt in (("f32", torch.float32), ("f64", torch.float64)):
            xt = torch.tensor(x, dtype=tdt, requires_grad=True)
            Wt = torch.tensor(weight, dtype=tdt, requires_grad=True)
            bt = torch.tensor(bias, dtype=tdt, requires_grad=True)
            y = color_affine(xt, Wt, bt, uid)
            mt = torch.tensor(mask, dtype=tdt) if mask is not None else None
            zero = torch.zeros((1, 1, 3), dtype=tdt)
            # _get_loss with only w_affine_reg = 1: loss = 0 (L1 of the render against itself) + affine_reg; the per-triangle terms are off
            pkg = {"render": y, "render_original": xt, "scaling": zero, "opacity": zero, "vertex": zero, "gt_image": y.detach().clone(),
                   "gt_mask": mt, "depth": None, "normal": None}
            areg = run_get_loss(trainer_mod, trainer_config(0.0, 0.0, 0.0, BIG, BIG, 0.0, BIG, 10, w_a=1.0), 1, pkg)
            L = areg + (y * torch.tensor(R, dtype=tdt)).sum()
            L.backward()
            out[f"y{m}_{dt}"] = y.detach().numpy()
            out[f"affine_reg{m}_{dt}"] = np.array(float(areg.detach()))
            out[f"L{m}_{dt}"] = np.array(float(L.detach()))
            out[f"dx{m}_{dt}"], out[f"dweight{m}_{dt}"], out[f"dbias{m}_{dt}"] = xt.grad.numpy(), Wt.grad.numpy(), bt.grad.numpy()
    # the L1 of trainer_utils on its own, for the restatement of affine_reg (:103)
    out["l1_f64"] = np.array(float(tu.L1(torch.tensor(out["x0"], dtype=torch.float64), torch.tensor(out["y0_f64"]))))
    path = os.path.join(HERE, "regularizers.npz")
    np.savez_compressed(path, **out)
    print("regularizers.npz:", os.path.getsize(path), "bytes;", {c[0]: float(out[f"loss_{c[0]}_f64"]) for c in CASES})


if __name__ == "__main__":
    main()
