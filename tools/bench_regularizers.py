"""Times the trainer's regularisers and the per-view colour affine (csrc/regularizers.hip) on MI355X, fwd+bwd, next to an eager-torch statement of the
same expressions (the kernel chain the reference runs: VanillaTS_trainer.py:86-116, trainer_utils.py:339-346, VanillaTS_model.py:72-76, 678-684).
Prints one JSON line.

    python tools/bench_regularizers.py [P] [H W]          (default 1 M triangles, 1080 x 1920)

Per-triangle workload: scaling + quad opacity + vertex terms, nearest indices from nearestNeighbor, the prepared inverse built once (as between two
refreshes of the cache; its cost is reported separately).  Affine workload: ColorAffine + affine_reg (masked L1 against the raw render, no mask).
Algorithmic bytes per triangle: forward 36 (vertex) + 4 (opacity) + 12 (nearest) + 36 (neighbour rows) = 88; backward those 88 + 24 (run offsets and
sources) + 36 (source rows, mean in-degree 1) + 40 (gradients) = 188.  Per pixel: affine forward 24, backward 36 (x, dL/dy in, dL/dx out); masked L1
forward 28, backward 40."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "triangle-splatting_amd")]
import torch  # noqa: E402

from diff_recon_hip import ColorAffine, affine_reg, prepare_nearest, triangle_regularization  # noqa: E402
from diff_triangle_rasterization_2D import _C  # noqa: E402
from simple_knn import nearestNeighbor  # noqa: E402

HBM_GBPS = 8000.0


def timed(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e6


def profiled(fn, n=50):
    _C.profile_reset()
    _C.profile_only("")
    _C.profile_enable(True)
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    rows = {name: ms * 1e3 / max(c, 1) for name, ms, c in _C.profile_read()}
    _C.profile_enable(False)
    return rows


def eager_reg(v, o, nearest, w_s, w_o, w_v):
    l1 = (v[:, 2] - v[:, 1]).norm(dim=1)
    l2 = (v[:, 0] - v[:, 2]).norm(dim=1)
    l3 = (v[:, 1] - v[:, 0]).norm(dim=1)
    pc = v.view(-1, 3)
    return (w_s * torch.stack((l1, l2, l3), dim=1).mean(dim=1).mean() + w_o * (0.25 - (o - 0.5) ** 2).mean()
            + w_v * ((pc - pc[nearest]) ** 2).sum(dim=1).mean())


def main():
    P = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    H, W = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1080, 1920)
    g = torch.Generator(device="cuda").manual_seed(0)
    c = torch.rand((P, 1, 3), device="cuda", generator=g) * 4 - 2
    v = (c + 0.01 * torch.randn((P, 3, 3), device="cuda", generator=g)).requires_grad_(True)
    o = torch.rand((P, 1), device="cuda", generator=g).requires_grad_(True)
    nearest = nearestNeighbor(v.detach().view(-1, 3), 3)
    nearest_long = nearest.view(torch.int32).long()
    prep = prepare_nearest(nearest)
    w_s, w_o, w_v = 0.3, 0.05, 5.0

    def native_reg():
        v.grad = o.grad = None
        triangle_regularization(v, o, nearest, w_scaling=w_s, w_opacity=w_o, opacity_mode="quad", w_vertex=w_v, prepared=prep)[0].backward()

    def torch_reg():
        v.grad = o.grad = None
        eager_reg(v, o, nearest_long, w_s, w_o, w_v).backward()

    native_reg()
    gv, go = v.grad.clone(), o.grad.clone()
    torch_reg()
    err_reg = float(max((gv - v.grad).norm() / v.grad.norm(), (go - o.grad).norm() / o.grad.norm()))
    us_reg, us_reg_eager = timed(native_reg), timed(torch_reg)
    rows = profiled(native_reg)
    rows.update(profiled(lambda: prepare_nearest(nearest), 10))

    ca = ColorAffine(8, device="cuda")
    with torch.no_grad():
        ca.weight.add_(0.05 * torch.randn(ca.weight.shape, device="cuda", generator=g))
        ca.bias.add_(0.02 * torch.randn(ca.bias.shape, device="cuda", generator=g))
    x = (torch.rand((3, H, W), device="cuda", generator=g) * 1.2 - 0.1).requires_grad_(True)
    w_a, uid = 0.1, 3

    def native_affine():
        x.grad = None
        ca.zero_grad(set_to_none=True)
        (w_a * affine_reg(ca(x, uid), x)).backward()

    def torch_affine():
        x.grad = None
        ca.zero_grad(set_to_none=True)
        y = (x.permute(1, 2, 0) @ ca.weight[uid] + ca.bias[uid]).permute(2, 0, 1).clamp(0, 1)
        (w_a * (y - x).abs().mean()).backward()

    native_affine()
    gx, gW = x.grad.clone(), ca.weight.grad.clone()
    torch_affine()
    err_aff = float(max((gx - x.grad).norm() / x.grad.norm(), (gW - ca.weight.grad).norm() / ca.weight.grad.norm()))
    us_aff, us_aff_eager = timed(native_affine), timed(torch_affine)
    rows.update(profiled(native_affine))

    n_px = H * W
    alg = {"reg_fwd": 88 * P, "reg_bwd": 188 * P, "color_affine_fwd": 24 * n_px, "color_affine_bwd": 36 * n_px, "masked_l1_fwd": 28 * n_px,
           "masked_l1_bwd": 40 * n_px}
    print(json.dumps({
        "workload": f"regularisers fwd+bwd at {P} triangles (scaling + quad opacity + vertex); colour affine + affine_reg fwd+bwd at 3x{H}x{W}",
        "reg_native_us": round(us_reg, 1), "reg_eager_torch_us": round(us_reg_eager, 1), "reg_speedup": round(us_reg_eager / us_reg, 2),
        "affine_native_us": round(us_aff, 1), "affine_eager_torch_us": round(us_aff_eager, 1), "affine_speedup": round(us_aff_eager / us_aff, 2),
        "kernels_avg_us": {k: round(t, 2) for k, t in rows.items()},
        "algorithmic_bytes": alg,
        "achieved_GBps": {k: round(alg[k] / (rows[k] * 1e-6) / 1e9, 1) for k in alg if k in rows},
        "hbm_frac": {k: round(alg[k] / (rows[k] * 1e-6) / 1e9 / HBM_GBPS, 3) for k in alg if k in rows},
        "grad_rel_l2_native_vs_eager": {"reg": err_reg, "affine": err_aff}}))


if __name__ == "__main__":
    main()
