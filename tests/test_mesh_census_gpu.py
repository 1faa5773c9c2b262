"""GPU tests of the mesh census (diff_recon_hip.MeshCensus over ts2d_mesh_census_add, csrc/mesh_census.hip) against the numpy reference
tests/ref_mesh_census.py -- integer accumulators, so every comparison is exact -- and of what is built on it: baked face colours,
multi-view visibility pruning, the GLB round trip of a refined mesh and the example's --refine-mesh scores."""
import os
import sys

import numpy as np
import pytest
import torch

import ref_mesh_census as ref
import ref_mesh_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H, F = 70, 37, 97  # a row is neither a multiple of 64 nor of 16: runs straddle wavefront and row boundaries; 2590 pixels = 11 workgroups
SENTINEL = -0x0123456789ABCDEF
GUARD = 8


class Cam:  # the camera pattern of tests/test_mesh_gpu.py
    def __init__(self, s):
        self.device = DEV
        self.image_width, self.image_height = s["image_width"], s["image_height"]
        self.tan_fovx, self.tan_fovy = s["tanfovx"], s["tanfovy"]
        self.world_view_transform = torch.from_numpy(np.ascontiguousarray(s["viewmatrix"])).to(DEV)


def _runs(lengths, n, first=0):
    """n indices: runs of the given lengths laid end to end (cyclically), every run another face."""
    out, f, k = [], first, 0
    while len(out) < n:
        out += [f % F] * lengths[k % len(lengths)]
        f += 1
        k += 1
    return np.array(out[:n], np.int32)


def _patterns():
    n = W * H
    p = np.arange(n)
    runs = _runs([1, 2, 63, 64, 65, 70], n)
    holes = np.where(p % 2 == 0, (p // 2) % F, -1)
    last = np.where((p // 5) % 3 == 0, F - 1, (p // 5) % F)
    bad = _runs([7, 1, 30, 64], n, first=40)
    bad[3::11] = F        # one past the last row
    bad[5::13] = F + 5
    bad[0::17] = -7
    bad[n - 1] = F
    big = runs.copy()
    big[10::29] = np.iinfo(np.int32).max
    big[11::31] = np.iinfo(np.int32).min
    pats = {"one face": np.full(n, 13), "all different": p % F, "runs 1 2 63 64 65 70": runs, "alternating holes": holes,
            "index F-1": last, "only F-1": np.full(n, F - 1), "F, F+5 and -7 among neighbours": bad, "int32 extremes": big}
    return {k: np.ascontiguousarray(v.astype(np.int32).reshape(H, W)) for k, v in pats.items()}


def _target(seed):
    rng = np.random.default_rng(seed)
    t = rng.random((3, H, W), dtype=np.float32)
    flat = t.reshape(-1)
    plant = np.array([-0.5, 1.5, np.nan, 0.5 + 2.0 ** -17, 0.0, 1.0, np.inf, -np.inf, 0.5 + 3 * 2.0 ** -17], np.float32)
    where = rng.choice(flat.size, size=40 * len(plant), replace=False)
    flat[where] = np.tile(plant, 40)
    return t


def _mask(seed):
    return np.random.default_rng(seed).choice(np.array([0.0, -1.0, 1e-30, 1.0], np.float32), size=(H, W)).astype(np.float32)


def _guarded_census(num_faces):
    """A MeshCensus whose accumulator lies between guard rows of one allocation."""
    from diff_recon_hip import MeshCensus
    block = torch.full((num_faces + 2 * GUARD, 4), SENTINEL, device=DEV, dtype=torch.int64)
    c = MeshCensus(0, DEV)
    c.acc = block[GUARD:GUARD + num_faces]
    c.acc.zero_()
    assert c.acc.is_contiguous() and c.acc.data_ptr() == block.data_ptr() + GUARD * 32
    return c, block


def _guards_untouched(block, num_faces):
    return bool((block[:GUARD] == SENTINEL).all()) and bool((block[GUARD + num_faces:] == SENTINEL).all())


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("masked", [False, True])
def test_hand_made_index_images_match_the_reference_exactly(masked):
    mask = _mask(5) if masked else None
    for k, (name, fi) in enumerate(_patterns().items()):
        target = _target(100 + k)
        want = ref.census(F, fi, target, mask)
        c, block = _guarded_census(F)
        c.add(_t(fi), _t(target), _t(mask))
        torch.cuda.synchronize()
        got = c.acc.cpu().numpy()
        print(f"{name} (mask {masked}): counted {int(want[:, 0].sum())} of {W * H} pixels, rows that differ {int((got != want).any(1).sum())}")
        assert torch.equal(c.acc.cpu(), torch.from_numpy(want)), name
        assert _guards_untouched(block, F), name
        if name == "one face" and not masked:
            assert got[13, 0] == W * H and not np.delete(got, 13, 0).any()  # all 2590 adds on one row
    # the (1, H, W) mask form and a second view on top of the first
    fi, target = _patterns()["runs 1 2 63 64 65 70"], _target(7)
    c, block = _guarded_census(F)
    c.add(_t(fi), _t(target), _t(mask)).add(_t(fi), _t(target), None if mask is None else _t(mask[None]))
    assert torch.equal(c.acc.cpu(), torch.from_numpy(2 * ref.census(F, fi, target, mask))) and _guards_untouched(block, F)


def test_without_a_target_only_the_pixel_column_changes():
    for name, fi in _patterns().items():
        c, block = _guarded_census(F)
        c.acc[:, 1:] = 77
        c.add(_t(fi), None, _t(_mask(6)))
        want = ref.census(F, fi, None, _mask(6))
        assert not want[:, 1:].any()
        want[:, 1:] = 77
        assert torch.equal(c.acc.cpu(), torch.from_numpy(want)), name
        assert torch.equal(c.pixels().cpu(), torch.from_numpy(want[:, 0])) and _guards_untouched(block, F)


def test_view_order_and_repetition_leave_the_same_bits():
    pats = _patterns()
    views = [(pats["runs 1 2 63 64 65 70"], _target(1), None), (pats["all different"], _target(2), _mask(3)),
             (pats["F, F+5 and -7 among neighbours"], _target(4), _mask(8))]

    def run(order):
        from diff_recon_hip import MeshCensus
        c = MeshCensus(F, DEV)
        for i in order:
            fi, t, m = views[i]
            c.add(_t(fi), _t(t), _t(m))
        return c.acc.cpu()
    abc, cab, again = run([0, 1, 2]), run([2, 0, 1]), run([0, 1, 2])
    assert torch.equal(abc, cab) and torch.equal(abc, again)
    want = np.zeros((F, 4), np.int64)
    for fi, t, m in views:
        ref.census_add(want, fi, t, m)
    assert torch.equal(abc, torch.from_numpy(want))


@pytest.fixture(scope="module")
def scenes():
    cache = {}

    def get(name):
        if name not in cache:
            s, vertices, faces, colors, period = ref_mesh_f64.build_scene(name)
            view = Cam(s)
            rng = np.random.default_rng(21)
            view.gt_image = torch.from_numpy(rng.random((3, s["image_height"], s["image_width"]), dtype=np.float32)).to(DEV)
            cache[name] = (s, view, _t(vertices), _t(faces), _t(colors), period)
        return cache[name]
    return get


@pytest.mark.parametrize("name,alpha", [("A", False), ("B", False), ("B", True)])
def test_add_view_equals_the_reference_on_the_render_s_own_face_idx(scenes, name, alpha):
    from diff_recon_hip import MeshCensus
    s, view, vertices, faces, colors, period = scenes(name)
    view = Cam(s)
    view.gt_image = scenes(name)[1].gt_image
    if alpha:
        a = torch.zeros(1, s["image_height"], s["image_width"], device=DEV)
        a[:, :, 17:s["image_width"] // 2] = 1
        view.alpha_mask = a
    nf = faces.shape[0]
    c = MeshCensus(nf, DEV)
    out = c.add_view(view, vertices, faces, colors)
    assert set(out) == {"render", "mask", "depth", "face_idx"}
    fi, gt = out["face_idx"].cpu().numpy(), view.gt_image.cpu().numpy()
    want = ref.census(nf, fi, gt, view.alpha_mask.cpu().numpy() if alpha else None)
    print(f"scene {name} (alpha {alpha}): faces {nf}, with pixels {int((want[:, 0] > 0).sum())}, counted {int(want[:, 0].sum())}, covered {int((fi >= 0).sum())}")
    assert want[:, 0].sum() == ((fi >= 0) & ((view.alpha_mask[0].cpu().numpy() > 0) if alpha else True)).sum() > 1000
    assert torch.equal(c.acc.cpu(), torch.from_numpy(want))
    fallback = np.random.default_rng(3).random((nf, 3), dtype=np.float32)
    got, expect = c.mean_color(_t(fallback)).cpu().numpy(), ref.mean_color(want, fallback)
    ulps = np.abs(got.view(np.int32).astype(np.int64) - expect.view(np.int32).astype(np.int64))
    print(f"scene {name}: mean colour differs from the float64 formula by at most {int(ulps.max())} ulp")
    assert ulps.max() <= 1
    assert np.array_equal(got[want[:, 0] == 0], fallback[want[:, 0] == 0])
    assert np.array_equal(c.pixels().cpu().numpy(), want[:, 0])


def _render(view, vertices, faces, colors):
    from diff_recon_hip import MeshRenderer
    return MeshRenderer(view).render(vertices, faces, colors)


def test_baked_colours_cannot_lose_against_the_old_ones(scenes):
    from diff_recon_hip import bake_face_colors
    s, view, vertices, faces, colors, period = scenes("B")
    old = _t(np.random.default_rng(31).random((faces.shape[0], 3), dtype=np.float32))
    baked = bake_face_colors([view], vertices, faces, old)
    assert baked.shape == old.shape and baked.dtype == torch.float32
    a, b = _render(view, vertices, faces, old), _render(view, vertices, faces, baked)
    assert torch.equal(a["face_idx"], b["face_idx"])
    counted = (a["face_idx"] >= 0).cpu().numpy()
    gt = view.gt_image.cpu().numpy().astype(np.float64)
    err_old = (a["render"].cpu().numpy().astype(np.float64) - gt)[:, counted]
    err_new = (b["render"].cpu().numpy().astype(np.float64) - gt)[:, counted]
    mse_old, mse_new = (err_old ** 2).mean(), (err_new ** 2).mean()
    bias = np.abs(err_new.mean(1))
    print(f"baking: counted pixels {int(counted.sum())}, MSE {mse_old:.6f} -> {mse_new:.6f}, |mean residual| per channel {bias}")
    assert counted.sum() > 10000
    assert mse_new <= mse_old + 1e-9
    assert (bias < 2.0 ** -16).all()
    won = torch.zeros(faces.shape[0], dtype=torch.bool, device=DEV)
    won[a["face_idx"][a["face_idx"] >= 0].long()] = True
    assert torch.equal(baked[~won], old[~won]) and bool((~won).any())  # a face without pixels keeps its colour


@pytest.mark.parametrize("name", ["A", "B"])
def test_pruning_by_visibility_changes_nothing_that_is_seen(scenes, name):
    from diff_recon_hip import mesh_from_triangles, visible_triangle_mask
    s, view, vertices, faces, colors, period = scenes(name)
    P = s["vertex"].shape[0]
    twins = period is not None
    vertex, shs = _t(s["vertex"]), _t(s["shs"])
    mv, mf, _ = mesh_from_triangles(vertex, shs, save_back=twins)
    assert torch.equal(mv, vertices) and torch.equal(mf.long(), faces.long())  # the scene's mesh is the model's exported mesh
    keep = visible_triangle_mask([view], vertex, shs, save_back=twins)
    assert keep.shape == (P,) and keep.dtype == torch.bool
    kept = int(keep.sum())
    print(f"scene {name}: {kept} of {P} triangles win a pixel")
    assert 0 < kept < P  # at least one triangle is dropped and at least one is kept
    before = _render(view, vertices, faces, colors)
    face_keep = torch.cat([keep, keep]) if twins else keep
    old_index = torch.nonzero(face_keep).flatten().to(torch.int32)  # compaction: new face index -> old face index
    after = _render(view, vertices, faces[face_keep], colors[face_keep])
    torch.cuda.synchronize()
    for k in ("render", "mask", "depth"):
        assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), k
    mapped = torch.where(after["face_idx"] >= 0, old_index[after["face_idx"].clamp_min(0).long()], after["face_idx"])
    assert torch.equal(mapped, before["face_idx"])
    # the mask is the reference's count over this render's face_idx, twins added: min_pixels is a threshold on the triangle's pixels
    px = ref.census(faces.shape[0], before["face_idx"].cpu().numpy())[:, 0]
    px = px[:P] + px[P:] if twins else px
    assert np.array_equal(keep.cpu().numpy(), px >= 1)
    stricter = visible_triangle_mask([view], vertex, shs, min_pixels=3, save_back=twins)
    assert np.array_equal(stricter.cpu().numpy(), px >= 3)


def test_no_back_twin_wins_a_pixel_in_scene_a(scenes):
    """The twin fact on the raw (unfolded) census of scene A: a back twin f + P gets its front face's record bit for bit (mesh_preprocess.hip
    builds a record from the vertices in ascending index order), so it has the same coverage and depth on every pixel, the tie goes to the
    smaller index, and rows P .. 2 P - 1 hold no pixel.  The soup with twins therefore renders exactly like the front faces alone."""
    from diff_recon_hip import MeshCensus
    s, view, vertices, faces, colors, period = scenes("A")
    c = MeshCensus(faces.shape[0], DEV)
    both = c.add_view(view, vertices, faces, colors)
    px = c.pixels().cpu().numpy()
    print(f"scene A raw census: front faces hold {int(px[:period].sum())} pixels ({int((px[:period] > 0).sum())} faces), "
          f"back twins {int(px[period:].sum())} pixels ({int((px[period:] > 0).sum())} faces)")
    assert px[:period].sum() > 0
    assert px[period:].sum() == 0
    front = _render(view, vertices, faces[:period], colors[:period])
    for k in ("render", "mask", "depth", "face_idx"):
        assert torch.equal(both[k].view(torch.int32), front[k].view(torch.int32)), k


def test_twins_share_one_colour_and_the_refined_mesh_survives_a_glb_round_trip(scenes, tmp_path):
    from diff_recon_hip import MeshCensus, MeshRenderer, RawTriangle, bake_face_colors, mesh_from_triangles
    s, view, vertices, faces, colors, P = scenes("A")
    c = MeshCensus(2 * P, DEV)
    c.add_view(view, vertices, faces, colors)
    folded = c.fold_twins(P)
    assert folded.num_faces == P and torch.equal(folded.acc, c.acc[:P] + c.acc[P:]) and int(folded.pixels().sum()) == int(c.pixels().sum())
    with pytest.raises(ValueError):
        c.fold_twins(P - 1)
    baked = bake_face_colors([view], vertices, faces, colors, twin_period=P)
    assert baked.shape == (2 * P, 3) and torch.equal(baked[:P], baked[P:])
    assert torch.equal(baked[:P], folded.mean_color(colors[:P]))
    model = RawTriangle(s["vertex"], np.zeros((P, 1), np.float32), np.ascontiguousarray(s["shs"].reshape(P, -1)[:, :3])).with_face_colors(baked[:P])
    model.saveGLB(str(tmp_path / "refined.glb"))
    r = MeshRenderer(view)
    a = r.render(mesh_path=str(tmp_path / "refined.glb"))
    b = r.render(vertices, faces, baked)
    assert torch.equal(a["face_idx"], b["face_idx"]) and torch.equal(a["depth"], b["depth"]) and torch.equal(a["mask"], b["mask"])
    worst = (a["render"] - b["render"]).abs().max().item()
    print(f"GLB round trip of the baked colours: worst difference {worst:.6f}")
    assert worst <= 0.5 / 255 + 1e-6  # the file keeps 8 bits per channel (test_mesh_path_reads_what_save_glb_wrote's bound)
    # the same through the model-side helpers: the baked mesh of the model is the baked mesh of the file
    mv, mf, mc = mesh_from_triangles(_t(model.vertex), _t(model.shs))
    assert torch.equal(mf.long(), faces.long()) and (mc - baked).abs().max().item() <= 1e-6


def test_example_refinement_prunes_and_does_not_lower_the_score():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic
    cfg = dict(iters=60, triangles=4000, width=160, height=112, views=3)
    _, m, _ = train_synthetic.train("2D", views_per_step=2, log=None, **cfg)
    plain = train_synthetic.mesh_scores(m, "2D", **cfg)
    assert "refined" not in plain
    res = train_synthetic.mesh_scores(m, "2D", refine=True, **cfg)
    ref_ = res["refined"]
    print(f"example: {ref_['kept']} of {ref_['triangles']} triangles kept; mean PSNR {res['mean_psnr']:.3f} -> {ref_['mean_psnr']:.3f} dB, "
          f"mean SSIM {res['mean_ssim']:.4f} -> {ref_['mean_ssim']:.4f}")
    assert res["psnr"] == plain["psnr"] and res["ssim"] == plain["ssim"]  # the unrefined figures are what they were
    assert ref_["triangles"] == m._vertex.shape[0] and 0 < ref_["kept"] < ref_["triangles"]
    assert len(ref_["psnr"]) == 3 and ref_["mean_psnr"] >= res["mean_psnr"]
