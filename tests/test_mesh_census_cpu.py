"""CPU tests of the mesh census: the C ABI of ts2d_mesh_census_add (presence + argument validation, no device touched), the argument checks
of MeshCensus.add, the RawTriangle conveniences that export a refined mesh, and the numpy reference (tests/ref_mesh_census.py) on a
hand-computed example, so that the yardstick of the GPU tests is itself pinned."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ref_mesh_census as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, 1


@pytest.fixture(scope="module")
def lib(hip_lib_built):
    from diff_triangle_rasterization_2D import _abi  # the one table of signatures, on a CDLL of this module's own
    return _abi.bind(ctypes.CDLL(hip_lib_built))


def test_census_entry_point_is_declared_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ts_mesh.h")).read(), flags=re.S)
    assert re.search(r"\bts2d_mesh_census_add\s*\(", header)
    assert hasattr(lib, "ts2d_mesh_census_add")


def test_census_argument_validation_touches_no_device(lib):
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is decided before anything is queued
    add = lambda W, H, F, fi, census: lib.ts2d_mesh_census_add(W, H, F, fi, None, None, census, None)  # noqa: E731
    for args in ((0, 8, 4, fake, fake), (8, 0, 4, fake, fake), (-3, 8, 4, fake, fake), (8, -1, 4, fake, fake),  # width, height >= 1
                 (8, 8, -1, fake, fake),        # F >= 0
                 (8, 8, 4, None, fake),         # face_idx non-NULL
                 (8, 8, 0, None, None),         # ... also when there is no face
                 (8, 8, 4, fake, None)):        # census non-NULL unless F == 0
        assert add(*args) == INVALID, args
        assert lib.ts2d_last_error(), args
    assert add(8, 8, 4, fake, None) == INVALID and b"census" in lib.ts2d_last_error()
    assert add(8, 8, 4, None, fake) == INVALID and b"face_idx" in lib.ts2d_last_error()
    assert add(1 << 16, 1 << 16, 4, fake, fake) == INVALID and b"large" in lib.ts2d_last_error()  # 2^32 pixels: the sweep's index range
    assert add(8, 8, 0, fake, None) == OK  # no faces: a no-op, nothing to queue
    assert add(8, 8, 0, fake, fake) == OK


def test_add_checks_shapes_and_dtypes_and_has_no_cpu_path():
    from diff_recon_hip import MeshCensus
    c = MeshCensus(5, "cpu")
    assert c.acc.shape == (5, 4) and c.acc.dtype == torch.int64 and not c.acc.any() and c.num_faces == 5
    fi = torch.zeros(6, 7, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="face_idx"):
        c.add(torch.zeros(6, 7, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="face_idx"):
        c.add(torch.zeros(1, 6, 7, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="target"):
        c.add(fi, torch.zeros(3, 7, 6))
    with pytest.raises(RuntimeError, match="target"):
        c.add(fi, torch.zeros(3, 6, 7, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="pixel_mask"):
        c.add(fi, None, torch.zeros(6, 6))
    with pytest.raises(RuntimeError, match="pixel_mask"):
        c.add(fi, None, torch.zeros(6, 7, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="pixel_mask"):
        c.add(fi, torch.zeros(3, 6, 7), torch.zeros(2, 6, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # well-formed host tensors: a missing device is an error, never an eager substitute
        c.add(fi, torch.zeros(3, 6, 7), torch.ones(1, 6, 7))
    assert not c.acc.any()
    with pytest.raises(ValueError, match="fold_twins"):
        c.fold_twins(2)
    with pytest.raises(ValueError, match="fallback"):
        c.mean_color(torch.zeros(4, 3))


def test_fold_twins_and_mean_color_on_a_hand_made_accumulator():
    from diff_recon_hip import MeshCensus
    c = MeshCensus(4, "cpu")
    c.acc[:] = torch.tensor([[2, 65536, 0, 32768], [0, 0, 0, 0], [1, 65536, 65536, 0], [0, 0, 0, 0]])
    fb = torch.tensor([[0.1, 0.2, 0.3]] * 4)
    assert torch.equal(c.pixels(), torch.tensor([2, 0, 1, 0]))
    assert torch.equal(c.mean_color(fb), torch.tensor([[0.5, 0.0, 0.25], [0.1, 0.2, 0.3], [1.0, 1.0, 0.0], [0.1, 0.2, 0.3]]))
    f = c.fold_twins(2)
    assert torch.equal(f.acc, torch.tensor([[3, 131072, 65536, 32768], [0, 0, 0, 0]])) and f.num_faces == 2
    assert torch.equal(f.mean_color(fb[:2]), torch.tensor([[2 / 3, 1 / 3, 1 / 6], [0.1, 0.2, 0.3]], dtype=torch.float64).float())


def test_raw_triangle_mask_indexing_and_face_colours(tmp_path):
    from diff_recon_hip import RawTriangle
    from diff_recon_hip.raw_triangle import SH2RGB
    rng = np.random.default_rng(4)
    P = 9
    t = RawTriangle(rng.standard_normal((P, 3, 3)).astype(np.float32), rng.standard_normal((P, 1)).astype(np.float32),
                    rng.standard_normal((P, 12)).astype(np.float32))
    keep = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1], bool)
    for key in (keep, torch.from_numpy(keep)):
        k = t[key]
        assert len(k) == 5 and np.array_equal(k.vertex, t.vertex[keep]) and np.array_equal(k.opacity, t.opacity[keep]) and np.array_equal(k.shs, t.shs[keep])
    with pytest.raises(IndexError):
        t[keep[:4]]
    rgb = rng.random((P, 3)).astype(np.float32)
    c = t.with_face_colors(torch.from_numpy(rgb))
    assert np.allclose(SH2RGB(c.shs[:, :3]), rgb, rtol=0, atol=1e-6) and np.array_equal(c.shs[:, 3:], t.shs[:, 3:]) and c.shs is not t.shs
    assert np.array_equal(c.vertex, t.vertex) and not np.array_equal(c.shs[:, :3], t.shs[:, :3])
    with pytest.raises(ValueError):
        t.with_face_colors(rgb[:3])
    c[keep].saveGLB(str(tmp_path / "m.glb"))  # the refined mesh goes out through the unchanged writer
    back = RawTriangle(glb_path=str(tmp_path / "m.glb"))
    assert len(back) == 5 and np.allclose(SH2RGB(back.shs), rgb[keep], rtol=0, atol=0.5 / 255 + 1e-6)


def test_reference_agrees_with_a_hand_computed_example():
    """3 x 4 pixels, F = 3.  By hand: Q16 of 0.5 is 32768, of 0.25 16384, of 1.5 (clamped) 65536, of -0.5 and NaN 0; 0.5 + 2^-17 times 2^16
    is 32768.5, a tie that goes to the even 32768; 0.5 + 3 * 2^-17 gives 32769.5, a tie that goes to the even 32770."""
    t = 0.5 + 2.0 ** -17
    u = 0.5 + 3 * 2.0 ** -17
    nan = float("nan")
    face_idx = np.array([[0, 0, 1, -1],
                         [2, 3, 1, 1],
                         [-7, 2, 0, 5]], np.int32)
    red = np.array([[0.5, 0.25, 1.5, 0.5],
                    [t, 0.5, -0.5, nan],
                    [0.5, u, 1.0, 0.5]], np.float32)
    green = np.zeros((3, 4), np.float32)
    blue = np.full((3, 4), 0.25, np.float32)
    target = np.stack([red, green, blue])
    # face 0: pixels (0,0) (0,1) (2,2): red 32768 + 16384 + 65536;  face 1: (0,2) (1,2) (1,3): 65536 + 0 + 0;  face 2: (1,0) (2,1): 32768 + 32770
    want = np.array([[3, 114688, 0, 3 * 16384], [3, 65536, 0, 3 * 16384], [2, 65538, 0, 2 * 16384]], np.int64)
    assert np.array_equal(ref.census(3, face_idx, target), want)
    assert np.array_equal(ref.census(3, face_idx), np.array([[3, 0, 0, 0], [3, 0, 0, 0], [2, 0, 0, 0]]))  # no target: counts only
    mask = np.array([[1, 0, 1e-30, 1], [-1, 1, nan, 2], [1, 1, 0, 1]], np.float32)  # > 0 counts: 1e-30 does, 0, -1 and NaN do not
    want_m = np.array([[1, 32768, 0, 16384], [2, 65536, 0, 2 * 16384], [1, 32770, 0, 16384]], np.int64)
    assert np.array_equal(ref.census(3, face_idx, target, mask), want_m)
    assert np.array_equal(ref.census(3, face_idx, target, mask[None]), want_m)
    twice = ref.census_add(ref.census(3, face_idx, target), face_idx, target, mask)  # accumulation over views
    assert np.array_equal(twice, want + want_m)
    assert np.array_equal(ref.q16([0.0, 1.0, t, u, -0.5, 1.5, nan, np.inf, -np.inf]), [0, 65536, 32768, 32770, 0, 65536, 0, 65536, 0])
    got = ref.mean_color(want_m, np.full((3, 3), 0.75, np.float32))
    assert np.array_equal(got, np.array([[0.5, 0, 0.25], [0.5, 0, 0.25], [np.float32(32770 / 65536), 0, 0.25]], np.float32))
    assert np.array_equal(ref.mean_color(np.zeros((2, 4), np.int64), [[0.1, 0.2, 0.3]] * 2), np.array([[0.1, 0.2, 0.3]] * 2, np.float32))
