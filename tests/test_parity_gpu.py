"""GPU parity tests: the HIP path (through the drop-in autograd module -> ctypes -> C ABI of libts2d.so) against
the CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star / SURVEY.md 8c):
  * integer / index state bit-exact: radii, tiles_touched, prefix sums, tile rectangles, the (tile,depth)-sorted
    instance list, tile ranges; n_contrib exact up to a tiny outlier budget (it depends on a fp32 threshold);
  * rendered image relative L2 < 1e-4; depth / normal likewise;
  * gradients relative L2 < 1e-3.
The HIP blend kernels use FMA contraction and v_exp/v_log where the oracle uses glibc expf/powf without
contraction, hence tolerances rather than bit equality on floating-point outputs.
"""
import os

import numpy as np
import pytest

import helpers
import synthetic

pytestmark = pytest.mark.gpu

IMG_TOL = 1e-4   # north_star: image relative L2
GRAD_TOL = 1e-3  # north_star: gradient relative L2
OUTLIER_FRAC = 1e-5  # pixels allowed to differ in n_contrib (threshold flips at T <= 1e-4, alpha >= 1/255); at least 2


def _check_state(s, hf, of):
    st = of["state"]
    assert hf["num_rendered"] == of["num_rendered"]
    assert np.array_equal(hf["radii"], of["radii"])
    for hip_name, ora_name in [("tiles_touched", "tiles_touched"), ("vals", "vals"), ("ranges", "ranges")]:
        a = helpers.hip_state(hf, s, hip_name).astype(np.int64).reshape(-1)
        b = st.field(ora_name).astype(np.int64).reshape(-1)
        assert np.array_equal(a, b), hip_name
    assert np.array_equal(helpers.hip_state(hf, s, "keys").reshape(-1), st.field("keys").view(np.int64).reshape(-1))
    # private ordering state: triangles in (depth bits, id) order, and the instance slots that follow from it
    perm = helpers.hip_state(hf, s, "depth_perm").astype(np.int64)
    dbits = st.field("depth").view(np.uint32).astype(np.int64)
    assert np.array_equal(perm, np.lexsort((np.arange(len(dbits)), dbits)))
    assert np.array_equal(helpers.hip_state(hf, s, "point_offsets").astype(np.int64),
                          np.cumsum(st.field("tiles_touched").astype(np.int64)[perm]))
    rect = helpers.hip_state(hf, s, "rect")
    vis = of["radii"] > 0
    assert np.array_equal(rect[vis, :2], st.field("rect_min")[vis].astype(np.int32))
    assert np.array_equal(rect[vis, 2:], st.field("rect_max")[vis].astype(np.int32))
    # screen-space vertices and depth keys come from the contraction-free preprocess: bit-exact
    v2d = helpers.hip_state(hf, s, "v_2D")
    ora_v2d = np.concatenate([st.field("v1_2D"), st.field("v2_2D"), st.field("v3_2D")], axis=1)
    assert np.array_equal(v2d[vis], ora_v2d[vis])
    assert np.array_equal(helpers.hip_state(hf, s, "depth")[vis], st.field("depth")[vis])
    assert np.array_equal(helpers.hip_state(hf, s, "rgb")[vis], st.field("rgb")[vis])
    nc_h = helpers.hip_state(hf, s, "n_contrib").astype(np.int64)
    nc_o = st.field("n_contrib").astype(np.int64)
    # termination (T <= 1e-4) and the alpha threshold are fp32-rounding-sensitive per pixel: a budget, at least 2 pixels
    assert (nc_h != nc_o).sum() <= max(2, OUTLIER_FRAC * nc_h.size)


def _check_outputs(hf, of, ob, rich, use_feature=False):
    assert helpers.rel_l2(hf["out_feature"], of["out_feature"]) < IMG_TOL
    if rich:
        assert helpers.rel_l2(hf["depth"], of["depth"]) < IMG_TOL
        assert helpers.rel_l2(hf["normal"], of["normal"]) < IMG_TOL
        assert helpers.rel_l2(hf["contrib_sum"], of["contrib_sum"]) < IMG_TOL
        assert helpers.rel_l2(hf["contrib_max"], of["contrib_max"]) < IMG_TOL
    keys = ["dL_dvertex", "dL_dcenter2D", "dL_dopacity", "dL_dfeature" if use_feature else "dL_dshs"]
    for k in keys:
        assert helpers.rel_l2(hf[k], ob[k]) < GRAD_TOL, k


CASES = [
    # P, W, H, D, rich, gamma, back_culling, kwargs
    (300, 64, 64, 3, True, 1.0, False, {}),
    (2000, 128, 96, 3, True, 1.0, False, {}),
    (10000, 256, 256, 0, True, 1.0, False, {}),          # BASELINE.json configs[0]
    (10000, 256, 256, 3, False, 1.0, False, {}),         # inference mode (2-tuple output) incl. the fixed backward
    (5000, 200, 120, 2, True, 2.5, False, {}),           # general gamma (pow path), ragged image size
    (5000, 200, 120, 1, True, 50.0, True, {}),           # end of the gamma schedule + back-face culling
    (3000, 130, 70, 3, True, 0.5, False, {}),
    (1000, 320, 240, 3, True, 1.0, False, {"mode": "maincu"}),  # R2D/main.cu recipe: huge triangles, long lists
    (20000, 96, 96, 1, True, 1.0, False, {"edge_px": 2.0}),    # heavy overdraw, early termination
]


@pytest.mark.parametrize("P,W,H,D,rich,gamma,back_culling,kw", CASES)
def test_hip_matches_oracle(P, W, H, D, rich, gamma, back_culling, kw):
    s = synthetic.scene(P, W, H, D, seed=1234 + P, **kw)
    s["gamma"] = gamma
    of = helpers.oracle_forward(s, rich, back_culling)
    ob = helpers.oracle_backward(s, of, rich)
    hf = helpers.hip_forward_backward(s, rich, back_culling)
    _check_state(s, hf, of)
    _check_outputs(hf, of, ob, rich)


def test_feature_mode_and_background():
    """Pre-computed colours (`feature`, C=3) instead of SH, non-zero background colour and depth."""
    s = synthetic.scene(4000, 160, 144, 0, seed=5)
    rng = np.random.default_rng(5)
    s["feature"] = rng.random((4000, 3), dtype=np.float32)
    s["background"] = np.array([0.2, 0.5, 0.9], np.float32)
    s["background_depth"] = 1234.5
    of = helpers.oracle_forward(s, True, False, use_feature=True)
    ob = helpers.oracle_backward(s, of, True, use_feature=True)
    hf = helpers.hip_forward_backward(s, True, False, use_feature=True)
    _check_outputs(hf, of, ob, True, use_feature=True)


def test_max_sh_degree_larger_than_active():
    """M = 16 coefficients stored, active degree 1: gradients of the inactive coefficients are exactly zero."""
    s = synthetic.scene(3000, 128, 128, 1, seed=11, max_degree=3)
    of = helpers.oracle_forward(s, True)
    ob = helpers.oracle_backward(s, of, True)
    hf = helpers.hip_forward_backward(s, True)
    _check_outputs(hf, of, ob, True)
    assert np.all(hf["dL_dshs"][:, 4:, :] == 0)


def test_culled_and_degenerate_triangles():
    """Behind-camera, degenerate (zero-area) and off-screen triangles get radii 0 and exactly zero gradients."""
    s = synthetic.scene(512, 96, 96, 2, seed=3)
    v = s["vertex"]
    v[0:50, :, 2] += 5000.0          # behind the camera (near cull)
    v[50:100, 1, :] = v[50:100, 0, :]  # two coincident vertices
    v[100:150, :, 0] += 1e5          # far off-screen
    v[150:160] = 0.0                 # all-zero triangle
    of = helpers.oracle_forward(s, True)
    ob = helpers.oracle_backward(s, of, True)
    hf = helpers.hip_forward_backward(s, True)
    _check_state(s, hf, of)
    _check_outputs(hf, of, ob, True)
    dead = of["radii"] == 0
    assert dead[:160].all()
    assert np.all(hf["dL_dvertex"][dead] == 0) and np.all(hf["dL_dshs"][dead] == 0) and np.all(hf["dL_dopacity"][dead] == 0)


def test_empty_inputs():
    """P == 0 returns background-free zero images without launching anything (extension_interface.cu:130)."""
    import torch
    from diff_triangle_rasterization_2D import TriangleRasterizer

    s = synthetic.scene(4, 48, 32, 0, seed=1)
    rs = helpers.hip_settings(s, rich_info=True)
    vertex = torch.zeros((0, 3, 3), device="cuda", requires_grad=True)
    opacity = torch.zeros((0, 1), device="cuda", requires_grad=True)
    shs = torch.zeros((0, 1, 3), device="cuda", requires_grad=True)
    center2D = torch.zeros((0, 2), device="cuda", requires_grad=True)
    out = TriangleRasterizer(rs)(vertex, center2D, opacity, shs=shs)
    assert len(out) == 6 and out[0].shape == (3, 32, 48) and float(out[0].abs().sum()) == 0.0
    assert out[1].shape == (0,)


def test_nothing_visible():
    """All triangles culled: num_rendered == 0, image == background, depth == background depth."""
    s = synthetic.scene(100, 64, 48, 0, seed=2)
    s["vertex"][:, :, 2] += 1e4
    s["background"] = np.array([0.1, 0.2, 0.3], np.float32)
    hf = helpers.hip_forward_backward(s, True)
    assert hf["num_rendered"] == 0
    assert np.allclose(hf["out_feature"], s["background"][:, None, None])
    assert np.allclose(hf["depth"], s["background_depth"])
    assert np.all(hf["dL_dvertex"] == 0)


FULL_SIZE = [
    # P, W, H, D, variant  -- bench headline + BASELINE.json configs[1..4] as (P, W, H, D); the oracle is too
    # slow for these inside a unit test, so size-independent properties are checked instead
    (1_000_000, 1920, 1080, 3, 2),   # bench.py headline
    (300_000, 800, 800, 3, 2),       # configs[1]  NerfSynthetic 'lego'
    (2_000_000, 1920, 1080, 3, 2),   # configs[2]  MipNerf360 'bicycle'
    (93_000, 1600, 1600, 0, 3),      # configs[3]  VanillaTS_mesh 'ship', 800^2 x render_up_scale 2, 3D rasterizer
    (5_000_000, 1920, 1080, 0, 3),   # configs[4]  MatrixCity VanillaTS_mesh, 3D rasterizer
    (1_000_000, 1920, 1080, 3, 3),   # headline scene through the 3D rasterizer
]


@pytest.mark.parametrize("P,W,H,D,variant", FULL_SIZE)
def test_full_size_properties(P, W, H, D, variant):
    """Sortedness of the instance list, exact tile ranges, transmittance identity (sum of contributions + T_final == 1
    via a unit-colour render) and linearity of the backward in the upstream gradient."""
    import torch
    if variant == 3:
        from diff_triangle_rasterization_3D import TriangleRasterizer
    else:
        from diff_triangle_rasterization_2D import TriangleRasterizer

    s = synthetic.scene(P, W, H, D, seed=42, with_grads=False)
    rs = helpers.hip_settings(s, rich_info=True)
    t = lambda a: torch.from_numpy(a).cuda()
    vertex, opacity, shs = t(s["vertex"]).requires_grad_(True), t(s["opacity"]).requires_grad_(True), t(s["shs"])
    c2d = torch.zeros((P, 2), device="cuda", requires_grad=True)
    out = TriangleRasterizer(rs)(vertex, c2d, opacity, shs=shs)
    node = out[0].grad_fn
    N = node.num_rendered
    g, b, im = node.saved_tensors[5:8]
    from diff_triangle_rasterization_2D import _C
    keys = helpers.debug_read_state("keys", P, N, W, H, g, b, im).numpy()
    assert np.all(np.diff(keys) >= 0)                       # sorted by (tile, depth)
    ranges = helpers.debug_read_state("ranges", P, N, W, H, g, b, im).numpy().astype(np.int64)
    tiles = keys >> 32
    counts = np.bincount(tiles, minlength=ranges.shape[0])
    assert np.array_equal(ranges[:, 1] - ranges[:, 0], counts)
    assert int(counts.sum()) == N
    tt = helpers.debug_read_state("tiles_touched", P, N, W, H, g, b, im).numpy().astype(np.int64)
    assert int(tt.sum()) == N
    # unit "colour" via the feature path: out = sum_i contrib_i, and final_T = prod(1 - alpha_i) => out + T == 1
    ones = torch.ones((P, 3), device="cuda")
    out1 = TriangleRasterizer(rs)(vertex.detach(), c2d.detach(), opacity.detach(), feature=ones)
    final_T = helpers.debug_read_state("final_T", P, N, W, H, g, b, im)  # same geometry/opacity => same transmittance
    resid = (out1[0][0].cpu() + final_T - 1.0).abs().max()
    assert float(resid) < 2e-4
    # linearity of the backward in the upstream gradient
    g1 = torch.rand((3, H, W), device="cuda")
    gd = torch.zeros((H, W), device="cuda")
    gn = torch.zeros((3, H, W), device="cuda")
    grads1 = torch.autograd.grad([out[0], out[2], out[3]], [vertex, opacity], [g1, gd, gn], retain_graph=True)
    grads2 = torch.autograd.grad([out[0], out[2], out[3]], [vertex, opacity], [2.5 * g1, gd, gn])
    for a, b2 in zip(grads1, grads2):
        assert float((2.5 * a - b2).norm() / b2.norm()) < 2e-4  # fp32 atomics: summation order differs between runs


LAB_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bin", "libts2d_lab.so")


def test_forced_ticket_passes_match_oracle():
    """The hierarchical (ticket) radix passes, the elected-block scan and the ticket-path depth census -- which otherwise only scenes of
    more than ~6 M triangles / 12.6 M instances reach, and which produce num_rendered there -- forced on a small scene through the lab
    library's switch (csrc/ts2d_lab.h: ts2d_lab_force_ticket_passes), once with a constant top key byte of the depths and once with
    a varying one: num_rendered, radii, sorted keys and ids bit-exact against the oracle, images and gradients within the bars."""
    import json
    import subprocess
    import sys
    if not os.path.exists(LAB_LIB):
        pytest.skip("tools/bin/libts2d_lab.so not built")
    e = dict(os.environ, TS2D_LIBRARY_PATH=LAB_LIB, LAB_FORCE_TICKETS="1")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "lab_worker.py")], env=e, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("LAB_RESULT ")][-1][len("LAB_RESULT "):])
    assert len(res) == 2
    for case in res:
        for k, v in case.items():
            assert v < (1.0 if k.startswith("int_") else GRAD_TOL if k.startswith("dL_") else IMG_TOL), (k, v)


def test_one_launch_depth_order_equals_the_multi_launch_forms():
    """up to 12 288 triangles ONE launch (depth_order.hip: depth_order_small_kernel) replaces the depth sort's eight launches and the block-sum
    launch, with its own census and its own rule for the skipped fourth pass.  P = 1, 63, 64, 65, 1023, 12 287, 12 288 (the limit), 12 289 (first scene
    past it) and two all-culled scenes through the one-launch form, the ticket-free multi-launch passes and the hierarchical ticket passes (lab
    switches, tests/lab_worker.py): depth permutation, instance offsets, num_rendered, the sorted instance list and the image are identical."""
    import json
    import subprocess
    import sys
    if not os.path.exists(LAB_LIB):
        pytest.skip("tools/bin/libts2d_lab.so not built")
    e = dict(os.environ, TS2D_LIBRARY_PATH=LAB_LIB, LAB_DEPTH_ORDER="1")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "lab_worker.py")], env=e, capture_output=True,
                       text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("LAB_RESULT ")][-1][len("LAB_RESULT "):])
    assert len(res) == 12
    for case in res:
        assert case["multi_launch"] == 0.0 and case["tickets"] == 0.0, case
        assert (case["num_rendered"] == 0) == case["culled"], case


def test_split_depth_order_equals_the_multi_launch_forms():
    """Round 6: the sampled-splitter depth order (the product's path between 12 288 and 500 000 triangles; tested up to the 1.6 M it supports) against the LSD passes and against its own
    global-memory path, on scenes that bend the buckets -- tests/lab_worker.py, LAB_DEPTH_SPLIT."""
    import json
    import subprocess
    import sys
    if not os.path.exists(LAB_LIB):
        pytest.skip("tools/bin/libts2d_lab.so not built")
    e = dict(os.environ, TS2D_LIBRARY_PATH=LAB_LIB, LAB_DEPTH_SPLIT="1")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "lab_worker.py")], env=e, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("LAB_RESULT ")][-1][len("LAB_RESULT "):])
    assert len(res) == 9
    for case in res:
        assert case["split"] == 0.0 and case.get("split_cap512", 0.0) == 0.0, case
        assert case["num_rendered"] > 0, case


@pytest.mark.parametrize("P,W,H,D,variant,gamma", [
    (1_000_000, 1920, 1080, 3, 2, 1.0),   # bench.py headline
    (300_000, 800, 800, 3, 2, 1.0),       # BASELINE.json configs[1]
    (2_000_000, 1920, 1080, 3, 2, 1.0),   # configs[2]
    (93_000, 1600, 1600, 0, 3, 1.0),      # configs[3] (3D rasterizer, 800^2 x render_up_scale 2)
    # gamma > 1 at size: the *_mesh configurations ramp gamma 1 -> 50 (config/NerfSynthetic_VanillaTS_mesh.yaml:142-146,
    # VanillaTS_model.py:181-192), i.e. configs[3] / [4] spend most of their iterations in the kernels' GAMMA1 = false instantiation
    # (pow(ecc, 2 gamma): R3D/src/forward.cu:263-264, backward.cu:347-349, 384-385; R2D forward.cu:309-311, backward.cu:443-447)
    (1_000_000, 1920, 1080, 3, 2, 50.0),
    (1_000_000, 1920, 1080, 3, 2, 7.0),
    (93_000, 1600, 1600, 0, 3, 50.0),
    (93_000, 1600, 1600, 0, 3, 7.0),
])
def test_full_size_against_oracle(P, W, H, D, variant, gamma):
    """Full-size parity against the oracle itself (not only through properties).  The OpenMP oracle needs a many-core host
    for this to stay within seconds (about 6 s for the headline on the GPU box); skipped on small hosts.

    2D rasterizer: NO outlier budget -- images, SH / opacity gradients and the geometry gradients meet the north-star bars
    outright (measured at the headline: dL_dvertex 1.5e-4, dL_dcenter2D 1.9e-4 over all 10^6 triangles, which is the
    distance between two faithful fp32 evaluations: the oracle and the reference's own kernels differ by 1.6e-4,
    tests/test_reference_gpu.py::test_headline_size_three_way_noise_floor).  Round 1 needed a budget of 205 triangles here:
    its blend kernels evaluated the barycentrics as affine forms of the pixel offset, ~10x noisier than the reference's
    pixel-relative cross products on sub-pixel slivers (profiles/r02_noise_floor_1M_before.json).
    3D rasterizer (render3d_group.hip, the reference's per-pixel ray / plane expressions): integer state bit-exact against the oracle,
    floating-point outputs by the ONE criterion for the 3D variant (helpers.py): inside the spread of the reference's own three builds,
    no budget and no mask."""
    import os
    if (os.cpu_count() or 1) < 32:
        pytest.skip("full-size oracle runs need a many-core host")
    import test_parity3d_gpu as T3
    s = synthetic.scene(P, W, H, D, seed=42)
    s["gamma"] = gamma
    of = helpers.oracle_forward(s, True, False, variant=variant)
    ob = helpers.oracle_backward(s, of, True)
    hf = helpers.hip_forward_backward(s, True, False, variant=variant)
    assert hf["num_rendered"] == of["num_rendered"]
    assert np.array_equal(hf["radii"], of["radii"])
    for name in ("tiles_touched", "vals", "ranges"):
        assert np.array_equal(helpers.hip_state(hf, s, name).astype(np.int64).reshape(-1),
                              of["state"].field(name).astype(np.int64).reshape(-1)), name
    nc_h = helpers.hip_state(hf, s, "n_contrib").astype(np.int64)
    differ = int((nc_h != of["state"].field("n_contrib").astype(np.int64)).sum())
    print(f"n_contrib differs on {differ} of {nc_h.size} pixels")
    # 2D: SURVEY 8c's 1e-5; the 3D variant's ray / plane depth is ill-conditioned at grazing angles (tests/test_parity3d_gpu.py: 2e-4)
    assert differ <= max(2, (OUTLIER_FRAC if variant == 2 else 2e-4) * nc_h.size)
    if variant == 2:
        for k in ("out_feature", "depth", "normal"):
            assert helpers.rel_l2(hf[k], of[k]) < IMG_TOL, k
        for k in ("contrib_sum", "contrib_max"):
            assert helpers.rel_l2(hf[k], of[k]) < IMG_TOL, k
        for k in ("dL_dshs", "dL_dopacity", "dL_dvertex", "dL_dcenter2D"):
            assert helpers.rel_l2(hf[k], ob[k]) < GRAD_TOL, (k, helpers.rel_l2(hf[k], ob[k]))
        return
    T3._check_outputs(s, hf, of, ob, True)


def test_backward_when_the_loss_ignores_the_rich_outputs():
    """A loss that touches only the image (or only depth / normal): autograd hands the Function `None` for the other outputs
    (no zero tensors are materialised any more); the result must be what explicit zero upstream gradients give."""
    import torch
    from diff_triangle_rasterization_2D import TriangleRasterizer
    s = synthetic.scene(3000, 96, 64, 2, seed=5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    full = dict(s)
    full["dL_dout_depth"] = np.zeros_like(s["dL_dout_depth"])
    full["dL_dout_normal"] = np.zeros_like(s["dL_dout_normal"])
    want = helpers.hip_forward_backward(full, True, False)
    vertex, shs, opacity = (t(s[k]).requires_grad_(True) for k in ("vertex", "shs", "opacity"))
    center2D = torch.zeros((3000, 2), device="cuda", requires_grad=True)
    out = TriangleRasterizer(helpers.hip_settings(s, True))(vertex, center2D, opacity, shs=shs)
    (out[0] * t(s["dL_dout_feature"])).sum().backward()
    for got, k in ((vertex.grad, "dL_dvertex"), (shs.grad, "dL_dshs"), (opacity.grad, "dL_dopacity"), (center2D.grad, "dL_dcenter2D")):
        assert helpers.rel_l2(got.cpu().numpy().reshape(want[k].shape), want[k]) < 1e-5, k
    # only the depth map: the image's upstream gradient is the missing one
    vertex.grad = shs.grad = opacity.grad = None
    out = TriangleRasterizer(helpers.hip_settings(s, True))(vertex, torch.zeros((3000, 2), device="cuda", requires_grad=True), opacity, shs=shs)
    out[2].sum().backward()
    assert torch.isfinite(vertex.grad).all() and float(vertex.grad.abs().sum()) > 0.0
    assert float(shs.grad.abs().sum()) == 0.0  # the colours do not influence the depth map


@pytest.mark.parametrize("variant,P,K", [(2, 5000, 4), (2, 130, 3), (3, 5000, 7), (2, 60, 2)])
def test_ranged_backward_equals_the_single_launch(variant, P, K):
    """ts2d_backward_ranged (round 5): the per-triangle kernel of the backward in K launches over consecutive triangle ranges, an event behind each.
    Same results as ts2d_backward -- the per-triangle arithmetic does not know about ranges; only the atomic sums of the blend kernel in front of it
    vary from run to run -- for range sizes that do and do not divide P, ranges beyond P (P = 60, K = 2: the second range is empty), both variants."""
    import torch
    from diff_triangle_rasterization_2D import _C
    s = synthetic.scene(P, 160, 128, 2, seed=900 + P)
    hf = helpers.hip_forward_backward(s, True, variant=variant)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g, b, im = hf["buffers"]
    args = (s["tanfovx"], s["tanfovy"], t(s["viewmatrix"]), t(s["projmatrix"]), t(s["campos"]), s["sh_degree"], 1.0, 1.0, float(s["background_depth"]),
            t(s["background"]), t(s["vertex"]), t(s["shs"]), torch.Tensor([]), t(s["opacity"]), hf["num_rendered"], t(hf["radii"]), g, b, im,
            t(s["dL_dout_feature"]), t(s["dL_dout_depth"]), t(s["dL_dout_normal"]), True, False)
    events = [torch.cuda.Event() for _ in range(K)]
    for e in events:
        e.record()
    rows = _C.backward_range_rows(P, K)
    assert rows % 64 == 0 and rows * K >= P and rows * (K - 1) < P + 64 * K
    got = _C.rasterize_triangles_backward(*args, variant=variant, range_events=events)
    for e in events:
        e.synchronize()  # every event was recorded behind its range (an empty range records too)
    for name, x in zip(("dL_dvertex", "dL_dcenter2D", "dL_dshs", None, "dL_dopacity"), got):
        if name:
            assert helpers.rel_l2(x.cpu().numpy().reshape(hf[name].shape), hf[name]) < 1e-6, name


@pytest.mark.parametrize("variant,gamma,use_feature", [(2, 1.0, False), (2, 2.5, False), (2, 1.0, True), (3, 1.0, False), (3, 2.5, False), (3, 1.0, True)])
def test_colour_only_loss_on_a_rich_forward_equals_zero_depth_and_normal_gradients(variant, gamma, use_feature):
    """rich_info forward, loss on the colours only.  The reference's autograd hands its kernel two images of zeros for depth and normal
    (rasterizer.cu:290-300 runs the RICH_INFO kernels on them); here the module passes "no gradient" (include/ts2d.h: ts2d_loss_grads with both
    NULL) and the colour-only pixel kernel runs over the rich records.  Every depth / normal term is an exact zero in the reference's kernel
    (backward.cu:419-437), so the gradients must agree up to the order of the atomic adds."""
    s = synthetic.scene(6000, 200, 136, 2, seed=4242 + variant)
    s["gamma"] = gamma
    if use_feature:
        rng = np.random.default_rng(5)
        s["feature"] = rng.random((s["vertex"].shape[0], 3), dtype=np.float32)
    a = helpers.hip_forward_backward(s, True, use_feature=use_feature, variant=variant, depth_normal_grads="none")
    b = helpers.hip_forward_backward(s, True, use_feature=use_feature, variant=variant, depth_normal_grads="zeros")
    assert np.array_equal(a["out_feature"], b["out_feature"])
    for k in ("dL_dvertex", "dL_dcenter2D", "dL_dopacity", "dL_dfeature" if use_feature else "dL_dshs"):
        assert np.abs(b[k]).max() > 0
        assert helpers.rel_l2(a[k], b[k]) < 2e-6, k
