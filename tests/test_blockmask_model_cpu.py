"""The 4x4 block masks that the emission kernel forms once per instance (csrc/ts2d_support.h: block_mask, quad_anchor + block_mask_affine on a
setup with the 4x4 sample box), replayed in numpy fp32 (tools/sim/blockmask_model.py) against the blend kernels' per-pixel expression
(render_group.hip: barycentrics -> ecc -> ecc_in_range and alpha >= 1/255, evaluated relative to the quadrant's origin as the kernels do).  The
blend kernels no longer cull: a block the mask leaves out is a block whose pixels are not blended, so NO block that holds a hitting pixel may
ever be left unflagged -- on the populations tools/sim/qmask_model.py uses (slivers, 0.2 - 600 px, opacities around 1/255, gamma 0.5 - 50,
rectangles of up to 41 x 41 tiles for the affine form).  How many blocks the masks flag against the in-kernel block_cull they replace is
reported (profiles/blockmask_ab.txt records it), not asserted; that the masks cull at all is."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", [11, 12])
def test_block_masks_never_leave_out_a_block_with_a_hit(seed):
    sys.path.insert(0, os.path.join(ROOT, "tools", "sim"))
    import blockmask_model
    r = blockmask_model.run(1200, seed)
    print({k: v for k, v in r.items() if k != "first_miss"})
    assert r["hit_blocks"] > 100000 and r["instances"] > 100000  # the population reaches the tiles it is tested on
    for form in ("per_tile", "affine"):  # block_mask (the unstaged emission paths) and quad_anchor + block_mask_affine (the staged flush)
        assert r["missed32_" + form] == 0, (form, r["first_miss"])
        assert r["missed64_" + form] == 0, form  # the exact test's hits too: the margins are not spent on fp32 luck
        assert r["hit_blocks"] / r["flagged_" + form] > 0.9, form  # a mask that flags everything would pass the lines above
    assert r["missed32_block_cull"] == 0  # the in-kernel cull, which stays as the kernels' second instantiation


def test_mask_bit_order_is_block_culls():
    """Bit 4 q + g: quadrant q = qy << 1 | qx, block g = (by >> 2) * 2 + (bx >> 2) inside it -- a triangle inside one 4x4 block flags that bit alone."""
    sys.path.insert(0, os.path.join(ROOT, "tools", "sim"))
    import numpy as np
    import blockmask_model as B
    from qmask_model import quad_setup, support_scale
    f32 = np.float32
    for i in range(4):
        for j in range(4):
            x, y = 32 + 4 * i + 1.5, 48 + 4 * j + 1.5
            v = np.array([[x - 0.6, y - 0.5, x + 0.6, y - 0.4, x, y + 0.6]], f32)
            op, g2 = np.array([0.02], f32), np.array([2.0], f32)  # E ~ 1.8: the support stays inside the block
            E = support_scale(op, g2)
            q = quad_setup(v, E); q["E"] = E
            TX, TY = np.array([32], f32), np.array([48], f32)
            want = 1 << (4 * (2 * (j >> 1) + (i >> 1)) + 2 * (j & 1) + (i & 1))
            assert int(B.block_mask(q, B.block_offsets(q), TX, TY)[0]) == want
            assert int(B.pixel_hits_blocks(v, q["ia"], op, g2, TX, TY, np.float32)[0]) == want
            assert int(B.block_cull(v, q["ia"], op, g2, TX, TY)[0]) == want
