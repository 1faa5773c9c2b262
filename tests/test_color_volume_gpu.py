"""GPU tests of the colour volume against tests/ref_color_volume.py: the integrated colour state, the colour field, the sampler and the
vertex-attribute pass bit for bit, the two projection texts held together, purity, fuse_colored_mesh end to end against the numpy pipeline,
the GLB writer and the example's report."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import poison
import ref_color_volume as cref
import ref_volume as ref
from test_volume_gpu import _latlong_sphere

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
W_IMG, H_IMG = 48, 40
# (dims, origin, h, trunc): neither grid is a multiple of the block, no origin or spacing is a power of two
GRIDS = {"big": ((20, 18, 16), (-1.0, -0.9, -0.8), 0.1, 0.35), "small": ((9, 8, 7), (-1.25, -1.0, -0.95), 0.3, 0.9)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cam(view, tan_fovx, tan_fovy, W, H):
    return SimpleNamespace(world_view_transform=_dev(np.asarray(view, np.float32)), tan_fovx=tan_fovx, tan_fovy=tan_fovy, image_width=W,
                           image_height=H, device="cuda:0")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def _views():
    """Three views of 48 x 40: one that sees all of the grid, one whose narrow frustum misses part of it, one whose eye sits inside the grid
    (samples at z <= 0).  Depth: random about the distance to the grid's centre, with 0, negative, NaN and infinite entries; a colour image
    with values below 0 and above 1, NaN and infinities in single channels; a random mask."""
    rng = np.random.default_rng(23)
    out = []
    for eye, tan in (((0.3, -0.2, -3.0), (0.5, 0.45)), ((2.5, 1.0, 0.4), (0.12, 0.1)), ((0.35, 0.2, -0.45), (0.9, 0.8))):
        view = ref.look_at_view(eye)
        dist = float(np.linalg.norm(eye))
        depth = (dist + rng.uniform(-0.9, 0.9, (H_IMG, W_IMG))).astype(np.float32)
        special = rng.integers(0, 14, (H_IMG, W_IMG))
        for code, value in ((0, 0.0), (1, -0.5), (2, np.nan), (3, np.inf), (4, -np.inf), (5, -0.0)):
            depth[special == code] = value
        image = rng.uniform(-0.3, 1.3, (3, H_IMG, W_IMG)).astype(np.float32)
        bad = rng.integers(0, 40, (3, H_IMG, W_IMG))
        for code, value in ((0, np.nan), (1, np.inf), (2, -np.inf)):
            image[bad == code] = value
        mask = (rng.integers(0, 4, (H_IMG, W_IMG)) != 0).astype(np.uint8)
        out.append((view, tan, depth, image, mask))
    return out


def _volume(grid):
    from diff_recon_hip import ColorTSDFVolume
    dims, origin, h, trunc = GRIDS[grid]
    return ColorTSDFVolume(origin, h, dims, trunc, DEV)


def _integrate_gpu(grid, order, use_mask, carve=True):
    vol = _volume(grid)
    colored = torch.zeros(1, device=DEV, dtype=torch.int64)
    counts = []
    for k in order:
        view, (tx, ty), depth, image, mask = _views()[k]
        vol.integrate(_cam(view, tx, ty, W_IMG, H_IMG), _dev(depth), image=_dev(image), mask=_dev(mask) if use_mask else None, carve_uncovered=carve,
                      colored=colored)
        counts.append(int(colored.item()))
    return vol, counts


@functools.lru_cache(maxsize=None)
def _integrate_ref(grid, order, use_mask, carve=True):
    dims, origin, h, trunc = GRIDS[grid]
    n = dims[0] * dims[1] * dims[2]
    s, w = np.zeros(n, np.int64), np.zeros(n, np.int32)
    cs, cw, counts, total = np.zeros((n, 3), np.int64), np.zeros(n, np.int32), [], 0
    for k in order:
        view, (tx, ty), depth, image, mask = _views()[k]
        ref.integrate(s, w, dims, origin, h, trunc, view, tx, ty, W_IMG, H_IMG, depth, mask if use_mask else None, ref.CARVE_UNCOVERED if carve else 0)
        total += cref.integrate(cs, cw, dims, origin, h, trunc, view, tx, ty, W_IMG, H_IMG, depth, image, mask if use_mask else None)
        counts.append(total)
    return s, w, cs, cw, counts


# ---- integrate and colour field ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("grid", ["big", "small"])
def test_integrate_matches_the_reference_bit_for_bit(grid, use_mask):
    vol, counts = _integrate_gpu(grid, (0, 1, 2), use_mask)
    s, w, cs, cw, want = _integrate_ref(grid, (0, 1, 2), use_mask)
    dims = GRIDS[grid][0]
    assert vol.csum.shape == (*dims[::-1], 3) and vol.cweight.shape == dims[::-1] and vol.csum.dtype == torch.int64 and vol.cweight.dtype == torch.int32
    got_cs, got_cw = vol.csum.cpu().numpy().reshape(-1, 3), vol.cweight.cpu().numpy().reshape(-1)
    print(grid, "coloured per view", want, "weights", np.bincount(cw))
    assert counts == want
    assert np.array_equal(got_cw, cw), np.nonzero(got_cw != cw)[0][:10]
    assert np.array_equal(got_cs, cs), np.nonzero((got_cs != cs).any(axis=1))[0][:10]
    assert np.array_equal(vol.sum.cpu().numpy().reshape(-1), s) and np.array_equal(vol.weight.cpu().numpy().reshape(-1), w)  # the parent's state
    assert want[0] > 0 and want[1] > want[0] and want[2] > want[1] and (cw == 0).any() and cw.max() >= 2  # every view adds; not everything is seen
    assert (cw <= w).all() and (cw < w).any()  # colour only inside the band


def test_the_views_carry_the_cases_the_kernel_branches_on():
    dims, origin, h, trunc = GRIDS["big"]
    for view, (tx, ty), depth, image, mask in _views():
        ok, pix = cref.in_band(dims, origin, h, trunc, view, tx, ty, W_IMG, H_IMG, depth)
        x = image.reshape(3, -1)[:, pix[ok]]
        assert ok.any() and np.isnan(x).any() and np.isinf(x).any() and (x[np.isfinite(x)] < 0).any() and (x[np.isfinite(x)] > 1).any()
        for value in (0.0, np.inf, -np.inf):
            assert (depth == value).any()
        assert np.isnan(depth).any() and (depth < 0).any() and (mask == 0).any()


def test_a_saturated_colour_weight_is_left_alone():
    vol = _volume("big")
    vol.cweight.view(-1)[::3] = cref.INT32_MAX
    vol.csum.view(-1, 3)[::3] = -7
    view, (tx, ty), depth, image, _ = _views()[0]
    colored = torch.zeros(1, device=DEV, dtype=torch.int64)
    vol.integrate(_cam(view, tx, ty, W_IMG, H_IMG), _dev(depth), image=_dev(image), colored=colored)
    dims, origin, h, trunc = GRIDS["big"]
    n = dims[0] * dims[1] * dims[2]
    cs, cw = np.zeros((n, 3), np.int64), np.zeros(n, np.int32)
    cw[::3], cs[::3] = cref.INT32_MAX, -7
    want = cref.integrate(cs, cw, dims, origin, h, trunc, view, tx, ty, W_IMG, H_IMG, depth, image)
    free = np.zeros(n, np.int32)
    assert 0 < want < cref.integrate(np.zeros((n, 3), np.int64), free, dims, origin, h, trunc, view, tx, ty, W_IMG, H_IMG, depth, image)
    assert int(colored.item()) == want
    assert np.array_equal(vol.cweight.cpu().numpy().reshape(-1), cw) and np.array_equal(vol.csum.cpu().numpy().reshape(-1, 3), cs)


def test_view_order_does_not_matter_volumes_add_and_the_field_is_bit_equal():
    a, _ = _integrate_gpu("big", (0, 1, 2), True)
    b, _ = _integrate_gpu("big", (2, 0, 1), True)
    assert torch.equal(a.csum, b.csum) and torch.equal(a.cweight, b.cweight)
    _, _, cs, cw, _ = _integrate_ref("big", (0, 1, 2), True)
    for min_weight in (1, 2):
        got = b.color_field(min_weight)
        assert got.shape == (3, 16, 18, 20) and got.dtype == torch.float32
        got = got.cpu().numpy().reshape(3, -1)
        want = cref.color_field(cs, cw, min_weight)
        assert np.array_equal(_bits(got), _bits(want)), min_weight
        assert np.array_equal(np.isnan(got), np.broadcast_to(cw < min_weight, got.shape)) and np.isnan(got).any() and not np.isnan(got).all()
    half, rest = _integrate_gpu("big", (0,), True)[0], _integrate_gpu("big", (1, 2), True)[0]
    half.csum += rest.csum
    half.cweight += rest.cweight
    assert torch.equal(half.csum, a.csum) and torch.equal(half.cweight, a.cweight)


def test_the_two_projection_texts_agree():
    """One view, an image that is finite everywhere: the colour lands exactly on the samples on which the distance landed and whose pixel was
    covered within the band; and the parent's state is what TSDFVolume alone computes."""
    from diff_recon_hip import TSDFVolume
    dims, origin, h, trunc = GRIDS["big"]
    for k in range(3):
        view, (tx, ty), depth, _, mask = _views()[k]
        image = np.full((3, H_IMG, W_IMG), 0.5, np.float32)
        cam = _cam(view, tx, ty, W_IMG, H_IMG)
        plain = TSDFVolume(origin, h, dims, trunc, DEV)
        plain.integrate(cam, _dev(depth), mask=_dev(mask))
        vol = _volume("big")
        vol.integrate(cam, _dev(depth), image=_dev(image), mask=_dev(mask))
        assert torch.equal(vol.sum, plain.sum) and torch.equal(vol.weight, plain.weight)
        band, _ = cref.in_band(dims, origin, h, trunc, view, tx, ty, W_IMG, H_IMG, depth, mask)
        weight = plain.weight.cpu().numpy().reshape(-1)
        cweight = vol.cweight.cpu().numpy().reshape(-1)
        assert set(np.unique(cweight)) <= {0, 1} and np.array_equal(cweight == 1, (weight == 1) & band)
        assert band.any() and ((weight == 1) & ~band).any()
        assert (vol.csum.cpu().numpy().reshape(-1, 3)[band] == 32768).all()


# ---- sampler ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sampler_case(C, grid="big"):
    """(grid values (C, n), dims, origin, h, points (N, 3), expected number of special points by kind)."""
    if grid == "flat":
        dims, origin, h = (5, 1, 4), (0.3, -0.7, 1.1), 0.23
    else:
        dims, origin, h, _ = GRIDS[grid]
    nx, ny, nz = dims
    n = nx * ny * nz
    rng = np.random.default_rng(100 + C)
    g = rng.normal(0.0, 1.0, (C, nz, ny, nx)).astype(np.float32)
    holes = rng.integers(0, n, n // 12)
    g.reshape(C, n)[rng.integers(0, C, len(holes)), holes] = np.nan  # one bad channel: the sample has no data
    g.reshape(C, n)[rng.integers(0, C, 10), rng.integers(0, n, 10)] = np.inf
    lattice = np.stack(ref.sample_positions(dims, origin, h)[0], axis=1).astype(np.float32)
    o32 = np.asarray(origin, np.float32)
    lo, hi = lattice[0], lattice[-1]
    scattered = rng.uniform(lo - 0.05, hi + 0.05, (1000, 3)).astype(np.float32)
    for a in range(3):
        if dims[a] == 1:  # an axis of one sample: only its own plane is inside
            scattered[:800, a] = lo[a]
    pts = [scattered, lattice[rng.permutation(n)[:300] if n >= 300 else rng.integers(0, n, 300)]]
    upper = rng.uniform(lo, hi, (60, 3)).astype(np.float32)
    for a in range(3):  # on each upper face, one fp32 step below it and one above it
        for m, step in enumerate((0.0, -np.inf, np.inf)):
            rows = slice(20 * a + m, 20 * a + 20, 3)
            upper[rows, a] = hi[a] if step == 0.0 else np.nextafter(hi[a], np.float32(step))
    pts.append(upper)
    outside = rng.uniform(lo, hi, (12, 3)).astype(np.float32)
    for a in range(3):
        outside[4 * a, a] = np.nextafter(lo[a], np.float32(-np.inf))
        outside[4 * a + 1, a] = np.nan
        outside[4 * a + 2, a] = np.inf
        outside[4 * a + 3, a] = -np.inf
    pts.append(outside)
    kinds = {}
    if grid == "big":
        g[:, 8:12, 8:12, 8:12] = np.nan  # a block without data: the cells inside it find nothing
        nodata = (o32 + np.float32(h) * rng.uniform(9.05, 9.95, (20, 3))).astype(np.float32)
        g[:, 2:6, 2:6, 0] = np.nan        # ... and a wall on the face x = 0: a point ON that face weighs the data of x = 1 with 0
        g[:, 2:6, 2:6, 1] = 1.5
        wall = np.stack([np.full(20, o32[0]), o32[1] + np.float32(h) * rng.uniform(3.05, 3.95, 20), o32[2] + np.float32(h) * rng.uniform(3.05, 3.95, 20)],
                        axis=1).astype(np.float32)
        pts += [nodata, wall]
        kinds = {"nodata": 20, "wall": 20}
    pts = np.concatenate(pts)
    assert len(pts) % 256 != 0
    return g.reshape(C, n), dims, origin, h, pts, kinds


@pytest.mark.parametrize("grid", ["big", "flat"])
@pytest.mark.parametrize("C", [1, 3, 8])
def test_sampler_matches_the_reference_bit_for_bit(C, grid):
    from diff_recon_hip import sample_grid
    g, dims, origin, h, pts, kinds = _sampler_case(C, grid)
    want, want_valid = cref.sample(g, dims, origin, h, pts)
    shaped = g.reshape(C, *dims[::-1])
    out, valid = sample_grid(_dev(shaped[0] if C == 1 else shaped), origin, h, _dev(pts))
    assert out.shape == (len(pts), C) and out.dtype == torch.float32 and valid.shape == (len(pts),) and valid.dtype == torch.bool
    got, got_valid = out.cpu().numpy(), valid.cpu().numpy()
    print(grid, "C", C, "points", len(pts), "valid", int(want_valid.sum()))
    assert np.array_equal(got_valid, want_valid.astype(bool)), np.nonzero(got_valid != want_valid.astype(bool))[0][:10]
    diff = (_bits(got) != _bits(want)).any(axis=1)
    assert not diff.any(), (np.nonzero(diff)[0][:10], got[diff][:2], want[diff][:2])
    assert (_bits(got[~got_valid]) == 0x7FC00000).all() and np.isfinite(got[got_valid]).all()
    # the specials are what they were built to be (by the reference)
    assert want_valid[:1000].any() and not want_valid[:1000].all()
    lattice_valid = want_valid[1000:1300].astype(bool)
    assert lattice_valid.any() and not lattice_valid.all()
    assert want_valid[1300:1360].any() and not want_valid[1300:1360].all()  # the upper faces: inside up to the face, outside past it
    assert not want_valid[1360:1372].any()
    if kinds:
        assert not want_valid[1372:].any()
        gx = (pts[1392:, 0].astype(np.float64) - float(np.float32(origin[0]))) / float(np.float32(h))
        assert (gx == 0).all()  # the wall points sit at t = 0: the only corners with data have weight 0


def test_sampler_takes_no_points():
    from diff_recon_hip import sample_grid
    out, valid = sample_grid(torch.zeros((3, 4, 4), device=DEV), (0, 0, 0), 0.1, torch.zeros((0, 3), device=DEV))
    assert out.shape == (0, 1) and valid.shape == (0,)


# ---- interpolation ------------------------------------------------------------------------------------------------------------------------------
W_INT, H_INT = 50, 37


@functools.lru_cache(maxsize=None)
def _interp_case():
    """A 10 x 5 sphere (80 faces) plus a zero-area face (drawn by hand only) and a face that names a vertex outside [0, V)."""
    v, f = _latlong_sphere(10, 5, 0.6)
    f = np.concatenate([f, np.array([[3, 3, 7], [2, len(v), 5], [-1, 2, 3]], np.int32)])
    view = ref.look_at_view((1.1, -0.8, -2.2))
    return v, f, view, 0.5, 0.42


def _face_images():
    """name -> (H, W) int32: MeshRenderer's own image with a few wild entries, and one made by hand that assigns pixels to faces that do not
    cover them."""
    from diff_recon_hip import MeshRenderer
    v, f, view, tx, ty = _interp_case()
    cam = _cam(view, tx, ty, W_INT, H_INT)
    F = len(f)
    colour = torch.zeros((F - 2, 3), device=DEV)
    rendered = MeshRenderer(cam).render(vertices=_dev(v), faces=_dev(f[:F - 2]), faces_color=colour)["face_idx"].cpu().numpy().copy()
    assert (rendered >= 0).sum() > 100 and (rendered < 0).sum() > 100
    rendered[0, :6] = (-1, F, -2 ** 31, F - 1, F - 2, 2 ** 31 - 1)  # uncovered, one past the end, INT32_MIN, the two faces with bad indices, INT32_MAX
    rendered[1, :3] = F - 3  # the zero-area face
    rng = np.random.default_rng(9)
    by_hand = rng.integers(-2, F + 2, (H_INT, W_INT)).astype(np.int32)
    return {"rendered": rendered, "by_hand": by_hand}


@pytest.mark.parametrize("C", [1, 3, 4])
def test_interpolate_matches_the_reference_bit_for_bit(C):
    from diff_recon_hip import interpolate_vertex_attributes
    v, f, view, tx, ty = _interp_case()
    cam = _cam(view, tx, ty, W_INT, H_INT)
    rng = np.random.default_rng(40 + C)
    attr = rng.uniform(-2.0, 3.0, (len(v), C)).astype(np.float32)
    bg = rng.uniform(-1.0, 1.0, C).astype(np.float32)
    for name, fi in _face_images().items():
        want, want_bary = cref.interpolate(view, tx, ty, W_INT, H_INT, v, f, fi, attr, bg)
        out, bary = interpolate_vertex_attributes(cam, _dev(v), _dev(f), _dev(fi), _dev(attr), _dev(bg), return_bary=True)
        assert out.shape == (C, H_INT, W_INT) and bary.shape == (3, H_INT, W_INT)
        got, got_bary = out.cpu().numpy(), bary.cpu().numpy()
        assert np.array_equal(_bits(got_bary), _bits(want_bary)), (name, np.argwhere(_bits(got_bary) != _bits(want_bary))[:5])
        assert np.array_equal(_bits(got), _bits(want)), (name, np.argwhere(_bits(got) != _bits(want))[:5])
        only = interpolate_vertex_attributes(cam, _dev(v), _dev(f), _dev(fi), _dev(attr), _dev(bg))
        assert torch.equal(only, out)
        F = len(f)
        drawn = (fi >= 0) & (fi < F - 2)
        assert drawn.any() and (~drawn).any()
        assert (got[:, ~drawn] == bg[:, None]).all() and (got_bary[:, ~drawn] == 0).all()
        b = got_bary[:, drawn]
        assert (b >= 0).all() and np.abs(b.astype(np.float64).sum(axis=0) - 1.0).max() <= 2 * 2.0 ** -23
        inside = (b > 0).all(axis=0)
        print(name, "C", C, "drawn", int(drawn.sum()), "strictly inside", int(inside.sum()), "held at the border", int((~inside).sum()))
        assert inside.any() and (~inside).any()
        lo, hi = attr.min(axis=0), attr.max(axis=0)
        assert (got[:, drawn] >= lo[:, None] - 1e-5).all() and (got[:, drawn] <= hi[:, None] + 1e-5).all()  # a convex combination


def test_interpolate_without_faces_writes_the_background():
    from diff_recon_hip import interpolate_vertex_attributes
    _, _, view, tx, ty = _interp_case()
    cam = _cam(view, tx, ty, W_INT, H_INT)
    fi = torch.zeros((H_INT, W_INT), device=DEV, dtype=torch.int32)
    out, bary = interpolate_vertex_attributes(cam, torch.zeros((0, 3), device=DEV), torch.zeros((0, 3), device=DEV, dtype=torch.int32), fi,
                                              torch.zeros((0, 2), device=DEV), torch.tensor([0.25, -3.0], device=DEV), return_bary=True)
    assert (out[0] == 0.25).all() and (out[1] == -3.0).all() and (bary == 0).all()


# ---- purity -------------------------------------------------------------------------------------------------------------------------------------
def test_all_four_calls_are_pure():
    from diff_recon_hip import interpolate_vertex_attributes, sample_grid
    g, dims, origin, h, pts, _ = _sampler_case(3)
    grid, points = _dev(g.reshape(3, *dims[::-1])), _dev(pts)
    v, f, view, tx, ty = _interp_case()
    cam = _cam(view, tx, ty, W_INT, H_INT)
    fi = _dev(_face_images()["by_hand"])
    attr, bg = _dev(np.linspace(-1, 2, 3 * len(v), dtype=np.float32).reshape(len(v), 3)), _dev(np.array([0.1, 0.2, 0.3], np.float32))
    vd, fd = _dev(v), _dev(f)

    def call(pattern):  # the accumulators are inputs: cleared by the volume's constructor; every output comes from torch.empty and is poisoned
        vol, counts = _integrate_gpu("big", (2, 1), True)
        out, valid = sample_grid(grid, origin, h, points)
        image, bary = interpolate_vertex_attributes(cam, vd, fd, fi, attr, bg, return_bary=True)
        return {"csum": vol.csum, "cweight": vol.cweight, "coloured": torch.tensor(counts), "field": vol.color_field(1), "field2": vol.color_field(2),
                "sample": out, "valid": valid, "image": image, "bary": bary}

    base = poison.assert_pure(call)
    _, _, cs, cw, want = _integrate_ref("big", (2, 1), True)
    assert np.array_equal(base["cweight"].numpy().view(np.int32), cw) and base["coloured"].numpy().view(np.int64).tolist() == want


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fused():
    from diff_recon_hip import MeshRenderer, fuse_colored_mesh
    v, f = _latlong_sphere()
    centre = v[f].astype(np.float64).mean(axis=1)
    colour = cref.sphere_color(centre).astype(np.float32)  # 0.5 + 0.4 n
    cams = [_cam(ref.look_at_view(eye), 0.45, 0.45, 48, 48) for eye in ref.AXIS_EYES]
    vd, fd, cd = _dev(v), _dev(f), _dev(colour)
    mesh, vol = fuse_colored_mesh(cams, vd, fd, cd, 20, return_volume=True)
    renders = [MeshRenderer(cam).render(vertices=vd, faces=fd, faces_color=cd) for cam in cams]
    return dict(v=vd, f=fd, colour=cd, cams=cams, mesh=mesh, vol=vol, renders=renders)


def test_fuse_colored_mesh_equals_the_numpy_pipeline():
    from diff_recon_hip import ColoredMesh, ColorTSDFVolume, fuse_mesh
    m = _fused()
    mesh, vol = m["mesh"], m["vol"]
    assert isinstance(mesh, ColoredMesh) and isinstance(vol, ColorTSDFVolume) and vol.dims == (20, 20, 20)
    n = 20 ** 3
    s, w, cs, cw = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros((n, 3), np.int64), np.zeros(n, np.int32)
    for cam, out in zip(m["cams"], m["renders"]):
        depth, image = out["depth"].cpu().numpy(), out["render"].cpu().numpy()
        args = (vol.dims, vol.origin, vol.voxel_size, vol.trunc, cam.world_view_transform.cpu().numpy(), 0.45, 0.45, 48, 48, depth)
        ref.integrate(s, w, *args, flags=ref.CARVE_UNCOVERED)
        cref.integrate(cs, cw, *args, image)
    assert np.array_equal(vol.sum.cpu().numpy().reshape(-1), s) and np.array_equal(vol.weight.cpu().numpy().reshape(-1), w)
    assert np.array_equal(vol.csum.cpu().numpy().reshape(-1, 3), cs) and np.array_equal(vol.cweight.cpu().numpy().reshape(-1), cw)
    want_tri, _ = ref.extract(ref.field(s, w), vol.dims, vol.origin, vol.voxel_size)
    got_tri = mesh.vertices[mesh.faces.to(torch.int64)].cpu().numpy()
    assert mesh.stats["num_faces"] == len(want_tri) and np.array_equal(_bits(got_tri), _bits(want_tri))
    verts = mesh.vertices.cpu().numpy()
    want_colour, want_valid = cref.sample(cref.color_field(cs, cw), vol.dims, vol.origin, vol.voxel_size, verts)
    assert want_valid.all() and mesh.color_valid.all() and mesh.color_valid.dtype == torch.bool  # every vertex found a colour
    assert mesh.vertex_color.shape == (len(verts), 3) and np.array_equal(_bits(mesh.vertex_color.cpu().numpy()), _bits(want_colour))
    plain = fuse_mesh(m["cams"], m["v"], m["f"], 20)
    assert torch.equal(plain.vertices, mesh.vertices) and torch.equal(plain.faces, mesh.faces) and plain.stats == mesh.stats
    err = np.abs(want_colour.astype(np.float64) - cref.sphere_color(verts))
    print("vertices", len(verts), "largest colour error against 0.5 + 0.4 n", err.max())


def test_vertex_colours_score_above_the_mean_colour_on_every_view():
    from diff_recon_hip import evaluate_vertex_colors, psnr, render_vertex_colors
    m = _fused()
    mesh = m["mesh"]
    mean = mesh.vertex_color.mean(dim=0, keepdim=True).expand_as(mesh.vertex_color).contiguous()
    views = []
    for cam, out in zip(m["cams"], m["renders"]):
        target = out["render"]
        got = render_vertex_colors(cam, mesh.vertices, mesh.faces, mesh.vertex_color)
        flat = render_vertex_colors(cam, mesh.vertices, mesh.faces, mean)
        assert set(got) == {"render", "mask", "depth", "face_idx"} and got["render"].shape == (3, 48, 48)
        assert float(got["render"].min()) >= 0.0 and float(got["render"].max()) <= 1.0 and torch.equal(got["face_idx"], flat["face_idx"])
        a, b = float(psnr(got["render"], target)), float(psnr(flat["render"], target))
        print("PSNR of the vertex colours", a, "of the mean colour", b)
        assert a > b
        views.append(SimpleNamespace(**vars(cam), gt_image=target))
    scores = evaluate_vertex_colors(views, mesh.vertices, mesh.faces, mesh.vertex_color, bg_color=torch.zeros(3))
    assert set(scores) == {"psnr", "ssim", "mean_psnr", "mean_ssim"} and len(scores["psnr"]) == len(scores["ssim"]) == 6
    assert np.isfinite(scores["mean_psnr"]) and np.isfinite(scores["mean_ssim"])


# ---- I/O and example ------------------------------------------------------------------------------------------------------------------------------
def test_save_glb_mesh_round_trips(tmp_path):
    from diff_recon_hip import save_glb_mesh
    from diff_recon_hip.mesh_renderer import load_glb_mesh
    from diff_recon_hip.raw_triangle import _accessor, read_glb
    mesh = _fused()["mesh"]
    path = tmp_path / "fused.glb"
    save_glb_mesh(path, mesh.vertices, mesh.faces, mesh.vertex_color)
    doc, binary = read_glb(path)
    prim = doc["meshes"][0]["primitives"][0]
    assert np.array_equal(_accessor(doc, binary, prim["attributes"]["POSITION"]), mesh.vertices.cpu().numpy())
    assert np.array_equal(_accessor(doc, binary, prim["indices"]).reshape(-1, 3), mesh.faces.cpu().numpy())
    col = _accessor(doc, binary, prim["attributes"]["COLOR_0"])
    assert col.dtype == np.uint8 and col.shape == (mesh.vertices.shape[0], 4) and (col[:, 3] == 255).all()
    assert np.array_equal(col[:, :3], np.round(mesh.vertex_color.cpu().numpy().astype(np.float64).clip(0, 1) * 255).astype(np.uint8))
    v, f, c = load_glb_mesh(str(path), DEV)
    assert torch.equal(v, mesh.vertices) and torch.equal(f, mesh.faces) and c.shape == (mesh.faces.shape[0], 3)


def test_example_reports_the_vertex_coloured_fused_mesh():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    res = train_synthetic.mesh_scores(m, "2D", extract=32, extract_color=True, **cfg)
    colour = res["fused"]["color"]
    lines = train_synthetic.fused_color_report(colour)
    print("\n".join(train_synthetic.fused_report(res["fused"]) + lines))
    assert len(lines) == 2 and lines[0].startswith("fused mesh, colours fused from the 2 training views") and "mean PSNR" in lines[0] and "mean SSIM" in lines[0]
    assert lines[1].startswith("the soup, one colour per face: mean PSNR") and "mean SSIM" in lines[1]
    assert colour["soup"]["mean_psnr"] == res["mean_psnr"] and len(colour["psnr"]) == 2 and 0 < colour["coloured"] <= colour["vertices"]
    assert np.isfinite(colour["mean_psnr"]) and np.isfinite(colour["mean_ssim"])
    plain = train_synthetic.mesh_scores(m, "2D", extract=32, **cfg)["fused"]
    assert "color" not in plain and plain["topology"] == res["fused"]["topology"]  # the same mesh; without the flag nothing changes
