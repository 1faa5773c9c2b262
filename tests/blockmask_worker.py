"""Runs small scenes through the LAB library twice in one process -- the 4x4 block masks taken from the tile keys, as the product does, then the
blend kernels' own in-kernel cull (ts2d_lab_force_kernel_cull) -- and prints how far apart the results are, plus what each scene exercised
(emission paths, lists long enough for a second pass, how sparse the masks are).  tests/test_blockmask_gpu.py asserts on the printed numbers.

    TS2D_LIBRARY_PATH=tools/bin/libts2d_lab.so python tests/blockmask_worker.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "triangle-splatting_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import helpers  # noqa: E402
import synthetic  # noqa: E402
from diff_triangle_rasterization_2D import _C  # noqa: E402

STAGE, SMALL, SB = 2048, 32, 256  # csrc/emit.hip: scan_emit_kernel


def world_of_pixel(s, px, py, zv):
    """World-space point that the scene's camera projects to pixel (px, py) at view depth zv (synthetic.camera: x_view = -x, z_view = dist - z)."""
    W, H = s["image_width"], s["image_height"]
    xv = ((2.0 * px + 1.0) / W - 1.0) * zv * s["tanfovx"]
    yv = ((2.0 * py + 1.0) / H - 1.0) * zv * s["tanfovy"]
    return np.stack([-xv, yv, synthetic.CAM_DIST - zv], -1)


def borders_and_slivers(s, rng):
    """A third of the triangles get vertices ON block and quadrant borders (pixel coordinates that are multiples of 4, or half a pixel before
    one), a third become slivers (the third vertex within ~1e-3 px of the opposite edge), and a fifth of all opacities straddle 1/255."""
    P = s["vertex"].shape[0]
    W, H = s["image_width"], s["image_height"]
    v = s["vertex"].astype(np.float64)
    zv = rng.uniform(1000.0, 1200.0, P)
    kind = rng.integers(0, 3, P)
    snap = kind == 0
    gx = rng.integers(0, W // 4 + 1, (P, 3)) * 4.0 - 0.5 * rng.integers(0, 2, (P, 3))
    gy = rng.integers(0, H // 4 + 1, (P, 3)) * 4.0 - 0.5 * rng.integers(0, 2, (P, 3))
    near = rng.integers(-2, 3, (P, 3, 2)) * 4.0  # the three vertices a few blocks apart
    gx[:, 1:] = gx[:, :1] + near[:, 1:, 0]; gy[:, 1:] = gy[:, :1] + near[:, 1:, 1]
    for k in range(3):
        v[snap, k] = world_of_pixel(s, gx[snap, k], gy[snap, k], zv[snap])
    sl = kind == 1
    t = rng.uniform(-0.2, 1.2, (P, 1))
    v[sl, 2] = (v[sl, 0] + t[sl] * (v[sl, 1] - v[sl, 0])) + rng.normal(0, 2e-3, (int(sl.sum()), 3))
    s["vertex"] = v.astype(np.float32)
    op = s["opacity"].copy()
    low = rng.random(P) < 0.2
    op[low, 0] = rng.uniform(0.0035, 0.0045, int(low.sum())).astype(np.float32)
    s["opacity"] = op
    return s


def partly_out_of_view(s, rng):
    """Half of the scene leaves the frustum sideways, a twentieth of it goes behind the camera."""
    v = s["vertex"].copy()
    v[:, :, :2] *= 1.5
    behind = rng.random(v.shape[0]) < 0.05
    v[behind, :, 2] += synthetic.CAM_DIST + 100.0
    s["vertex"] = v
    return s


CASES = [
    # name, P, W, H, D, gamma, back_culling, scene kwargs, edits
    ("small_staged", 3000, 100, 70, 1, 1.0, False, {}, (borders_and_slivers,)),                      # runs fit the stage: the affine flush
    ("small_gamma", 3000, 100, 70, 1, 2.5, False, {"edge_px": 8.0}, (borders_and_slivers,)),         # gamma != 1
    ("medium_unstaged", 2500, 116, 84, 1, 1.0, False, {"edge_px": 45.0}, (borders_and_slivers,)),    # runs beyond the stage, rectangles up to SMALL tiles and above
    ("huge_cooperative", 1500, 116, 84, 2, 0.7, True, {"mode": "maincu"}, ()),                        # the reference's main.cu recipe: every rectangle above SMALL; back_culling
    ("culled_view", 4000, 100, 70, 1, 1.0, True, {"edge_px": 10.0}, (partly_out_of_view, borders_and_slivers)),
    ("dense_lists", 6000, 52, 38, 0, 1.0, False, {"edge_px": 5.0}, ()),                               # > 32 entries of a batch with work: second pass
]


def emission_paths(hf, s):
    """Which of scan_emit_kernel's three paths the scene's instances took, from the depth order and the tile counts (256 triangles per block)."""
    P, W, H = s["vertex"].shape[0], s["image_width"], s["image_height"]
    tt = helpers.debug_read_state("tiles_touched", P, hf["num_rendered"], W, H, *hf["buffers"]).numpy().astype(np.int64)
    perm = helpers.debug_read_state("depth_perm", P, hf["num_rendered"], W, H, *hf["buffers"]).numpy().astype(np.int64)
    ts = np.zeros(((P + SB - 1) // SB) * SB, np.int64)
    ts[:P] = tt[perm]
    blocks = ts.reshape(-1, SB)
    staged = blocks.sum(1) <= STAGE
    return dict(staged=int(blocks[staged].sum()), unstaged_small=int(blocks[~staged][blocks[~staged] <= SMALL].sum()),
                cooperative=int(blocks[~staged][blocks[~staged] > SMALL].sum()), largest_run=int(blocks.sum(1).max()))


out = []
rng = np.random.default_rng(4711)
for name, P, W, H, D, gamma, back, kw, edits in CASES:
    s = synthetic.scene(P, W, H, D, seed=900 + P, **kw)
    s["gamma"] = gamma
    for f in edits:
        s = f(s, rng)
    res = []
    for kernel_cull in (0, 1):
        _C._lib.ts2d_lab_force_kernel_cull(kernel_cull)
        hf = helpers.hip_forward_backward(s, True, back_culling=back)
        hf["n_contrib"] = helpers.hip_state(hf, s, "n_contrib")
        hf["final_T"] = helpers.hip_state(hf, s, "final_T")
        res.append(hf)
    _C._lib.ts2d_lab_force_kernel_cull(0)
    a, b = res
    N = a["num_rendered"]
    e = {"name": name, "P": P, "gamma": gamma, "num_rendered": N, "same_num_rendered": N == b["num_rendered"],
         "visible": int((a["radii"] > 0).sum())}
    e.update(emission_paths(a, s))
    # one tile-sort pass at these sizes: the ping-pong partner of the sorted keys is what the emission kernel wrote, block masks included
    raw = helpers.debug_read_state("tile_unsorted", P, N, W, H, *a["buffers"]).numpy().view(np.uint32)
    quads = helpers.debug_read_state("vals_unsorted", P, N, W, H, *a["buffers"]).numpy().view(np.uint32) >> 28
    m16 = (raw >> 16).astype(np.uint16)
    e["block_bits_set_fraction"] = float(np.unpackbits(m16.view(np.uint8)).sum() / (16.0 * max(N, 1)))
    nib_or = sum((((m16 >> (4 * q)) & 0xF) != 0).astype(np.uint32) << q for q in range(4))
    e["quadrant_bits_are_the_or_of_the_nibbles"] = bool(np.array_equal(nib_or, quads))
    e["tiles_in_range"] = bool(((raw & 0xFFFF) < ((W + 15) // 16) * ((H + 15) // 16)).all())
    # the longest quadrant list: more than 32 entries with work in one 64-entry batch take the second pass of the 32-row table
    keys = helpers.debug_read_state("keys", P, N, W, H, *a["buffers"]).numpy() >> 32
    sorted_quads = helpers.debug_read_state("vals", P, N, W, H, *a["buffers"]).numpy().view(np.uint32) >> 28
    e["longest_quadrant_list"] = int(max((np.bincount(keys[((sorted_quads >> q) & 1) == 1], minlength=1).max() if N else 0) for q in range(4)))
    for k in ("out_feature", "depth", "normal", "final_T", "n_contrib", "radii"):
        e["exact_" + k] = bool(np.array_equal(a[k], b[k]))
        if not e["exact_" + k]:
            e["differing_" + k] = int((a[k] != b[k]).sum())
    for k in ("contrib_sum", "contrib_max", "dL_dvertex", "dL_dcenter2D", "dL_dshs", "dL_dopacity"):
        e[k] = float(helpers.rel_l2(a[k], b[k]))
        e["finite_" + k] = bool(np.isfinite(a[k]).all() and np.isfinite(b[k]).all())
    e["image_not_empty"] = bool((a["n_contrib"] > 0).mean() > 0.5)
    out.append(e)
print("BLOCKMASK_RESULT " + json.dumps(out))
