"""The block masks on the GPU, with the real kernels.  The emission kernel forms the 4x4 block mask of every instance once and leaves it in the
top half of the tile key; the 2D blend kernels take it from there and cull nothing themselves.  The lab library's ts2d_lab_force_kernel_cull
switches them to their second instantiation, the in-kernel block cull (what runs on grids of more than 65 535 tiles): both are pure culling of
work that contributes nothing, so every output must be the same either way -- out_feature, depth, normal, final_T and n_contrib bit for bit (a
pixel's blend order and arithmetic do not depend on what else its group looked at; a wrongly dropped block changes pixels), the atomically
summed outputs within the bars tests/helpers.py applies against a reference (R3D_BARS: 3e-4 for the contribution statistics, 1e-3 for
gradients).  tests/blockmask_worker.py runs the scenes -- a few thousand triangles on images of about 100 x 70 whose sizes are no multiples of
16 -- in one process of its own, because the switch exists only in the lab library and a process binds one library."""
import json
import os
import subprocess
import sys

import pytest

import helpers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAB_LIB = os.path.join(ROOT, "tools", "bin", "libts2d_lab.so")
NAMES = ["small_staged", "small_gamma", "medium_unstaged", "huge_cooperative", "culled_view", "dense_lists"]


@pytest.fixture(scope="module")
def results():
    assert os.path.exists(LAB_LIB), "tools/bin/libts2d_lab.so not built (python triangle-splatting_amd/build.py --lab)"
    e = dict(os.environ, TS2D_LIBRARY_PATH=LAB_LIB)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "blockmask_worker.py")], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("BLOCKMASK_RESULT ")][-1][len("BLOCKMASK_RESULT "):])
    assert [c["name"] for c in res] == NAMES
    return {c["name"]: c for c in res}


@pytest.mark.parametrize("name", NAMES)
def test_masks_from_the_keys_equal_the_in_kernel_cull(results, name):
    case = results[name]
    print(case)
    assert case["same_num_rendered"] and case["num_rendered"] > 1000 and case["image_not_empty"], case
    assert case["tiles_in_range"] and case["quadrant_bits_are_the_or_of_the_nibbles"], case
    assert 0.02 < case["block_bits_set_fraction"] < 0.98, case  # the masks do cull (and do not cull everything)
    for k in ("out_feature", "depth", "normal", "final_T", "n_contrib", "radii"):
        assert case["exact_" + k], case
    for k in ("contrib_sum", "contrib_max", "dL_dvertex", "dL_dcenter2D", "dL_dshs", "dL_dopacity"):
        assert case["finite_" + k], case
        assert case[k] < helpers.R3D_BARS[k], case


def test_the_scenes_cover_what_they_are_meant_to(results):
    """Each emission path (csrc/emit.hip: scan_emit_kernel) is taken by thousands of instances in the scene named for it, one of them through
    runs beyond the 2048-entry stage; a view that culls part of its scene; quadrant lists longer than the 32-row table (second pass)."""
    r = results
    assert r["small_staged"]["staged"] == r["small_staged"]["num_rendered"] and r["small_staged"]["largest_run"] <= 2048, r["small_staged"]
    assert r["medium_unstaged"]["unstaged_small"] > 5000 and r["medium_unstaged"]["largest_run"] > 2048, r["medium_unstaged"]
    assert r["huge_cooperative"]["cooperative"] > 5000 and r["huge_cooperative"]["largest_run"] > 2048, r["huge_cooperative"]
    assert 0.2 * r["culled_view"]["P"] < r["culled_view"]["visible"] < 0.8 * r["culled_view"]["P"], r["culled_view"]
    assert r["huge_cooperative"]["visible"] < r["huge_cooperative"]["P"], r["huge_cooperative"]  # back_culling removes about half
    assert r["dense_lists"]["longest_quadrant_list"] > 64, r["dense_lists"]  # whole 64-entry batches with work: two passes
    assert {r[n]["gamma"] for n in NAMES} >= {1.0, 2.5, 0.7}


def test_a_grid_above_65535_tiles_has_no_room_for_masks_and_culls_in_the_kernel():
    """513 x 129 = 66 177 tiles: the tile id needs 17 bits, the keys carry the tile alone (ts_tile_keymask) and the host picks the blend kernels'
    second instantiation.  The product library against the oracle, with the bars of helpers.R3D_BARS (image 1e-4, gradients 1e-3)."""
    import numpy as np
    import synthetic
    s = synthetic.scene(800, 8200, 2052, 0, seed=5, edge_px=50.0)
    assert ((s["image_width"] + 15) // 16) * ((s["image_height"] + 15) // 16) > 65535
    of = helpers.oracle_forward(s, rich_info=True)
    ob = helpers.oracle_backward(s, of, rich_info=True)
    hf = helpers.hip_forward_backward(s, rich_info=True)
    assert hf["num_rendered"] == of["num_rendered"] > 50000 and np.array_equal(hf["radii"], of["radii"])
    for k in ("out_feature", "depth", "normal", "contrib_sum", "contrib_max"):
        e = helpers.rel_l2(hf[k], of[k])
        print(k, e)
        assert e < helpers.R3D_BARS[k], (k, e)
    for k in ("dL_dvertex", "dL_dcenter2D", "dL_dshs", "dL_dopacity"):
        e = helpers.rel_l2(hf[k], ob[k])
        print(k, e)
        assert e < helpers.R3D_BARS[k], (k, e)
