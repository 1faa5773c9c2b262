"""CPU tests of the opaque mesh renderer: the float64 checker (tests/ref_mesh_f64.py) on hand-made cases and its ambiguous shares on the
four test scenes, the C ABI of include/ts_mesh.h (presence + argument validation, no device touched), mesh_from_triangles, psnr, and
the MeshRenderer signature."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ref_mesh_f64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4)


def _unproject(sx, sy, z, W, H, t=1.0):
    """View-space point (identity view matrix) at depth z that projects to pixel-frame position (sx, sy)."""
    return [(sx * 2 / W - 1) * z * t, (sy * 2 / H - 1) * z * t, z]


def test_one_triangle_covers_exactly_the_pixel_centres_inside_or_on_it():
    W = H = 8
    verts = np.array([_unproject(1, 1, 2.0, W, H), _unproject(7, 1, 2.0, W, H), _unproject(1, 7, 2.0, W, H)])
    out = ref.render(verts, [[0, 1, 2]], [[0.2, 0.4, 0.6]], W, H, 1.0, 1.0, EYE, background=(1.0, 0.0, 0.0))
    j, i = np.mgrid[0:H, 0:W]
    expect = (i + 0.5 >= 1) & (j + 0.5 >= 1) & ((i + 0.5) + (j + 0.5) <= 8)  # the hypotenuse x + y = 8 passes through centres: "on" counts
    assert np.array_equal(out["mask"], expect) and expect.sum() == 21
    assert np.array_equal(out["face_idx"], np.where(expect, 0, -1))
    assert np.allclose(out["depth"][expect], 2.0, rtol=1e-14) and np.all(out["depth"][~expect] == 0)
    assert np.allclose(out["render"][:, expect].T, [0.2, 0.4, 0.6]) and np.allclose(out["render"][:, ~expect].T, [1.0, 0.0, 0.0])
    assert out["ambiguous"][(i + j == 7) & expect].all()  # the centres on the hypotenuse: float32 may put them on either side
    assert not out["ambiguous"][(i + j <= 6) | ~expect].any()  # every other centre is at least 0.5 px / sqrt(2) from the boundary
    assert all(-1 in out["candidates"][(int(y), int(x))] and 0 in out["candidates"][(int(y), int(x))] for y, x in zip(*np.nonzero((i + j == 7) & expect)))


def test_two_crossing_triangles_split_along_their_intersection():
    W, H = 16, 12
    za = lambda x: 3 + 0.1 * x  # noqa: E731  plane A: nearer for x < 0
    zb = lambda x: 3 - 0.1 * x  # noqa: E731  plane B: nearer for x > 0
    verts = np.array([[-10, -10, za(-10)], [10, -10, za(10)], [0, 20, za(0)], [-10, -10, zb(-10)], [10, -10, zb(10)], [0, 20, zb(0)]], float)
    out = ref.render(verts, [[0, 1, 2], [3, 4, 5]], np.zeros((2, 3)), W, H, 1.0, 0.75, EYE)
    assert out["mask"].all()
    assert (out["face_idx"][:, : W // 2] == 0).all() and (out["face_idx"][:, W // 2:] == 1).all()  # x_ndc = 0 lies between two columns of centres
    x_ndc = (np.arange(W) + 0.5) * 2 / W - 1
    expect = np.where(x_ndc < 0, 3 / (1 - 0.1 * x_ndc), 3 / (1 + 0.1 * x_ndc))  # z = 3 +- 0.1 x with x = x_ndc z
    assert np.allclose(out["depth"], expect[None, :], rtol=1e-13)
    assert not out["ambiguous"].any()  # at the centres next to the split line the depths differ by 0.8 %: far outside both intervals


def test_a_face_with_one_vertex_behind_znear_draws_nothing():
    W = H = 8
    tri = [_unproject(1, 1, 2.0, W, H), _unproject(7, 1, 2.0, W, H), _unproject(1, 7, 0.5, W, H)]
    out = ref.render(np.array(tri), [[0, 1, 2]], np.ones((1, 3)), W, H, 1.0, 1.0, EYE, znear=1.0)
    assert not out["mask"].any() and (out["face_idx"] == -1).all() and not out["valid"].any() and not out["ambiguous"].any()
    assert ref.render(np.array(tri), [[0, 1, 2]], np.ones((1, 3)), W, H, 1.0, 1.0, EYE, znear=0.25)["mask"].any()
    assert not ref.render(np.array(tri), [[0, 1, 7]], np.ones((1, 3)), W, H, 1.0, 1.0, EYE, znear=0.25)["mask"].any()  # an index outside [0, V)


def test_equal_depths_go_to_the_smaller_face_index():
    W = H = 8
    verts = np.array([_unproject(1, 1, 2.0, W, H), _unproject(7, 1, 3.0, W, H), _unproject(1, 7, 2.5, W, H)])
    dup = ref.render(verts, [[0, 1, 2], [0, 1, 2]], np.zeros((2, 3)), W, H, 1.0, 1.0, EYE)
    assert dup["mask"].any() and (dup["face_idx"][dup["mask"]] == 0).all()
    twin = ref.render(verts, [[0, 1, 2], [2, 1, 0]], np.zeros((2, 3)), W, H, 1.0, 1.0, EYE, twin_period=1)
    assert np.array_equal(twin["mask"], dup["mask"]) and (twin["face_idx"][twin["mask"]] % 1 == 0).all()
    single = ref.render(verts, [[0, 1, 2]], np.zeros((1, 3)), W, H, 1.0, 1.0, EYE)
    inner = twin["mask"] & ~single["ambiguous"]  # away from the triangle's boundary
    assert inner.any() and not twin["ambiguous"][inner].any()  # a coincident twin makes no pixel ambiguous ...
    assert ref.render(verts, [[0, 1, 2], [2, 1, 0]], np.zeros((2, 3)), W, H, 1.0, 1.0, EYE)["ambiguous"][inner].all()  # ... an unrelated coincident face does


# the shares the issue measured for the checker's prototype; a checker that lands elsewhere has another definition
SHARES = {"A": 0.017, "B": 0.035, "C": 0.008, "D": 0.005}


@pytest.mark.parametrize("name", sorted(ref.SCENES))
def test_ambiguous_share_of_the_test_scenes_is_under_the_cap(name):
    s, vertices, faces, colors, period = ref.build_scene(name)
    out = ref.render_scene(s, vertices, faces, colors, twin_period=period)
    share = out["ambiguous"].mean()
    print(f"scene {name}: covered {out['mask'].mean():.3f} ambiguous {share:.4f}")
    assert share <= ref.MAX_AMBIGUOUS_SHARE
    assert abs(share - SHARES[name]) <= 0.002, share
    if name == "C":
        assert abs((~out["mask"]).mean() - 0.68) < 0.02
    amb = out["ambiguous"]
    assert set(out["candidates"]) == {(int(y), int(x)) for y, x in zip(*np.nonzero(amb))}
    for (y, x), c in out["candidates"].items():
        assert out["face_idx"][y, x] in c  # the checker's own answer is always allowed


def test_znear_inside_scene_a_leaves_straddlers_and_stays_under_the_cap():
    s, vertices, faces, colors, period = ref.build_scene("A")
    out = ref.render_scene(s, vertices, faces, colors, znear=1100.0, twin_period=period)
    z = out["view_vertices"][:period, :, 2]
    straddlers = int(((z > 1100.0).any(1) & ~(z > 1100.0).all(1)).sum())
    print(f"znear 1100: valid {out['valid'].mean():.3f} straddlers {straddlers} covered {out['mask'].mean():.3f} ambiguous {out['ambiguous'].mean():.4f}")
    assert straddlers >= 100
    assert out["ambiguous"].mean() <= ref.MAX_AMBIGUOUS_SHARE
    assert out["valid"][out["face_idx"][out["mask"]]].all()


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(hip_lib_built):
    from diff_triangle_rasterization_2D import _abi  # the one table of signatures, on a CDLL of this module's own
    return _abi.bind(ctypes.CDLL(hip_lib_built))


def test_mesh_entry_points_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "ts_mesh.h")).read()
    for name in ("ts2d_mesh_geometry_state_bytes", "ts2d_mesh_bin", "ts2d_mesh_render", "ts2d_mesh_render_counted"):
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
        assert hasattr(lib, name), name
    assert lib.ts2d_mesh_geometry_state_bytes(12345) == lib.ts2d_geometry_state_bytes(12345)


def test_mesh_argument_validation_touches_no_device(lib):
    from diff_triangle_rasterization_2D._abi import _Camera, _State
    INVALID, CAPACITY = 1, 3
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused before anything is queued
    n = ctypes.c_int64(-7)
    cam = _Camera(64, 48, 0.5, 0.4, fake, None, None)
    st = _State(fake, 1 << 30, fake, 1 << 30, fake, 1 << 30)
    bin_ = lambda c, znear, V, v, F, f, s, out: lib.ts2d_mesh_bin(c, znear, V, v, F, f, s, out, None)  # noqa: E731
    assert bin_(None, 1.0, 3, fake, 1, fake, ctypes.byref(st), ctypes.byref(n)) == INVALID and b"camera" in lib.ts2d_last_error()
    assert bin_(ctypes.byref(cam), 1.0, 3, fake, 1, fake, None, ctypes.byref(n)) == INVALID
    assert bin_(ctypes.byref(cam), 1.0, 3, fake, 1, fake, ctypes.byref(st), None) == INVALID
    assert bin_(ctypes.byref(cam), 1.0, 3, fake, -1, fake, ctypes.byref(st), ctypes.byref(n)) == INVALID
    assert bin_(ctypes.byref(cam), 1.0, -3, fake, 1, fake, ctypes.byref(st), ctypes.byref(n)) == INVALID
    assert bin_(ctypes.byref(cam), -1.0, 3, fake, 1, fake, ctypes.byref(st), ctypes.byref(n)) == INVALID and b"znear" in lib.ts2d_last_error()
    assert bin_(ctypes.byref(cam), float("nan"), 3, fake, 1, fake, ctypes.byref(st), ctypes.byref(n)) == INVALID
    assert bin_(ctypes.byref(cam), 1.0, 3, None, 1, fake, ctypes.byref(st), ctypes.byref(n)) == INVALID
    assert bin_(ctypes.byref(cam), 1.0, 3, fake, 1, None, ctypes.byref(st), ctypes.byref(n)) == INVALID
    assert bin_(ctypes.byref(cam), 1.0, 3, fake, 1 << 28, fake, ctypes.byref(st), ctypes.byref(n)) == CAPACITY and b"2^28" in lib.ts2d_last_error()
    small = _State(fake, 16, fake, 1 << 30, fake, 1 << 30)
    assert bin_(ctypes.byref(cam), 1.0, 3, fake, 1, fake, ctypes.byref(small), ctypes.byref(n)) == CAPACITY
    for bad in (_Camera(0, 48, 0.5, 0.4, fake, None, None), _Camera(64, 48, 0.0, 0.4, fake, None, None), _Camera(64, 48, 0.5, 0.4, None, None, None)):
        assert bin_(ctypes.byref(bad), 1.0, 3, fake, 1, fake, ctypes.byref(st), ctypes.byref(n)) == INVALID
    n.value = -7
    assert bin_(ctypes.byref(cam), 1.0, 0, None, 0, None, ctypes.byref(st), ctypes.byref(n)) == 0 and n.value == 0  # no faces: nothing to queue

    render = lambda c, F, col, bg, N, s, r, m: lib.ts2d_mesh_render(c, F, col, bg, N, s, r, m, None, None, None)  # noqa: E731
    assert render(None, 1, fake, fake, 1, ctypes.byref(st), fake, fake) == INVALID
    assert render(ctypes.byref(cam), 1, None, fake, 1, ctypes.byref(st), fake, fake) == INVALID
    assert render(ctypes.byref(cam), 1, fake, None, 1, ctypes.byref(st), fake, fake) == INVALID
    assert render(ctypes.byref(cam), 1, fake, fake, 1, None, fake, fake) == INVALID
    assert render(ctypes.byref(cam), 1, fake, fake, 1, ctypes.byref(st), None, fake) == INVALID
    assert render(ctypes.byref(cam), 1, fake, fake, 1, ctypes.byref(st), fake, None) == INVALID
    assert render(ctypes.byref(cam), 1, fake, fake, -1, ctypes.byref(st), fake, fake) == INVALID
    assert render(ctypes.byref(cam), 0, None, fake, 5, ctypes.byref(st), fake, fake) == INVALID
    assert render(ctypes.byref(cam), 1 << 28, fake, fake, 1, ctypes.byref(st), fake, fake) == CAPACITY
    assert render(ctypes.byref(cam), 1, fake, fake, 1 << 31, ctypes.byref(st), fake, fake) == CAPACITY
    no_image = _State(fake, 1 << 30, fake, 1 << 30, fake, 16)
    assert render(ctypes.byref(cam), 1, fake, fake, 1, ctypes.byref(no_image), fake, fake) == CAPACITY
    no_binning = _State(fake, 1 << 30, fake, 16, fake, 1 << 30)
    assert render(ctypes.byref(cam), 1, fake, fake, 1, ctypes.byref(no_binning), fake, fake) == CAPACITY


# ---- Python -----------------------------------------------------------------------------------------------------------------------
def test_mesh_renderer_has_the_reference_signature():
    import diff_recon_hip
    params = [(p.name, p.default) for p in inspect.signature(diff_recon_hip.MeshRenderer.render).parameters.values()]
    assert params == [("self", inspect.Parameter.empty), ("vertices", None), ("faces", None), ("faces_color", None), ("mesh_path", None)]
    ctor = list(inspect.signature(diff_recon_hip.MeshRenderer.__init__).parameters.values())
    assert [p.name for p in ctor] == ["self", "cam", "bg_color"]
    assert torch.equal(ctor[2].default, torch.Tensor([0, 0, 0]))

    class Cam:
        device = "cpu"
        image_width, image_height, tan_fovx, tan_fovy = 8, 8, 1.0, 1.0
        world_view_transform = torch.eye(4)
    r = diff_recon_hip.MeshRenderer(Cam())
    with pytest.raises(ValueError, match="Either mesh_path or vertices, faces, and faces_color must be provided"):
        r.render(vertices=torch.zeros(3, 3), faces=torch.zeros(1, 3, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="GLB"):
        r.render(mesh_path="model.ply")
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a missing device is an error, never an eager substitute
        r.render(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, 3))


@pytest.mark.parametrize("save_back", [True, False])
@pytest.mark.parametrize("flat", [False, True])
def test_mesh_from_triangles_matches_a_numpy_restatement(save_back, flat):
    from diff_recon_hip import mesh_from_triangles
    rng = np.random.default_rng(5)
    P, K = 37, 4
    vertex = rng.standard_normal((P, 3, 3)).astype(np.float32)
    shs = (rng.standard_normal((P, K, 3)) * 3).astype(np.float32)  # wide enough for both clip bounds to bite
    arg = torch.from_numpy(shs.reshape(P, K * 3) if flat else shs)
    v, f, c = mesh_from_triangles(torch.from_numpy(vertex), arg, save_back=save_back)
    rgb = np.clip(shs[:, 0, :].astype(np.float32) * np.float32(0.28209479177387814) + np.float32(0.5), 0, 1)
    faces = np.arange(3 * P).reshape(P, 3)
    if save_back:
        faces, rgb = np.concatenate([faces, faces[:, ::-1]]), np.concatenate([rgb, rgb])
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and c.dtype == torch.float32
    assert np.array_equal(v.numpy(), vertex.reshape(-1, 3)) and np.array_equal(f.numpy(), faces)
    assert np.allclose(c.numpy(), rgb, rtol=0, atol=1e-7) and (c.numpy() == 0).any() and (c.numpy() == 1).any()
    assert np.array_equal(v.numpy()[f.numpy()[:P]], vertex)  # face i owns triangle i's vertices, in order


def test_mesh_from_triangles_writes_what_save_glb_writes(tmp_path):
    from diff_recon_hip import RawTriangle, mesh_from_triangles
    from diff_recon_hip.mesh_renderer import load_glb_mesh
    rng = np.random.default_rng(6)
    P = 11
    vertex = rng.standard_normal((P, 3, 3)).astype(np.float32)
    shs = rng.standard_normal((P, 3)).astype(np.float32)
    RawTriangle(vertex, np.zeros((P, 1), np.float32), shs).saveGLB(str(tmp_path / "m.glb"))
    v, f, c = load_glb_mesh(str(tmp_path / "m.glb"), "cpu")
    v2, f2, c2 = mesh_from_triangles(torch.from_numpy(vertex), torch.from_numpy(shs))
    assert torch.equal(v, v2) and torch.equal(f, f2)
    assert torch.allclose(c, c2, rtol=0, atol=0.5 / 255 + 1e-6)  # the file keeps 8 bits per channel


@pytest.mark.parametrize("masked", [False, True])
def test_psnr_matches_float64_numpy(masked):
    from diff_recon_hip import psnr
    rng = np.random.default_rng(8)
    a, b = rng.random((3, 40, 56)), rng.random((3, 40, 56))
    m = (rng.random((1, 40, 56)) > 0.4).astype(np.float64) if masked else None
    if masked:
        mse = (((a - b) ** 2) * m).sum() / (m.sum() + 1e-10) + 1e-10
    else:
        mse = ((a - b) ** 2).mean() + 1e-10
    expect = 20 * np.log10(1.0 / np.sqrt(mse))
    got = psnr(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(m) if masked else None)
    assert abs(got.item() - expect) <= 1e-6 * abs(expect)
    got32 = psnr(torch.from_numpy(a).float(), torch.from_numpy(b).float(), torch.from_numpy(m).float() if masked else None)
    assert abs(got32.item() - expect) <= 1e-4 * abs(expect)  # float32 inputs: the sum's own rounding
    same = psnr(torch.from_numpy(a), torch.from_numpy(a))
    assert abs(same.item() - 100.0) < 1e-9  # the 1e-10 ceiling
