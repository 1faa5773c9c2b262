"""GPU tests of the texture atlas (diff_recon_hip/mesh_texture.py, libts_atlas.so, include/ts_atlas.h) against tests/ref_mesh_texture.py:
every index, every accumulator word, every texel of the resolved image and every pixel of its draw bit for bit; view order, additivity, the
R == 1 identity with MeshCensus, argument checks that touch nothing, and purity.

Images are 64 x 48 and 33 x 17 (neither a multiple of a wave nor of a row).  Meshes: (a) one triangle over the whole view, (b) a tilted
6 x 6 grid of quads (72 faces) from two views, (c) 7 faces at R = 64 (almost every texel unobserved, a half-empty last cell, one face that
wins no pixel), (d) no faces / no vertices, (e) the grid with face rows naming -1, V, a repeated vertex and one vertex three times (the
1.0 / 3.0 case) and face_idx entries -1, F, INT32_MIN, INT32_MAX."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import poison
import ref_mesh_texture as tref
import ref_volume as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG, SMALL = (64, 48), (33, 17)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cam(view, tan, size):
    return SimpleNamespace(world_view_transform=_dev(np.asarray(view, np.float32)), tan_fovx=tan[0], tan_fovy=tan[1], image_width=size[0],
                           image_height=size[1], device="cuda:0")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ne = _bits(got) != _bits(want)
    assert not ne.any(), (what, int(ne.sum()), np.argwhere(ne)[:5].tolist())


def _grid(n):
    """An n x n grid of quads over [-1, 1]^2 on the plane z = 0.3 x + 0.2 y: (n + 1)^2 vertices, 2 n^2 faces."""
    xs = np.linspace(-1.0, 1.0, n + 1)
    x, y = np.meshgrid(xs, xs, indexing="xy")
    v = np.stack([x, y, 0.3 * x + 0.2 * y], axis=-1).reshape(-1, 3).astype(np.float32)
    f = []
    for r in range(n):
        for c in range(n):
            a, b, d, e = r * (n + 1) + c, r * (n + 1) + c + 1, (r + 1) * (n + 1) + c, (r + 1) * (n + 1) + c + 1
            f += [(a, b, d), (b, e, d)]
    return v, np.array(f, np.int32)


def _image(rng, size):
    W, H = size
    t = rng.uniform(-0.2, 1.2, (3, H, W)).astype(np.float32)
    t[rng.integers(0, 50, (3, H, W)) == 0] = np.nan
    return t


def _mask(rng, size):
    W, H = size
    m = rng.uniform(-0.5, 1.0, (H, W)).astype(np.float32)
    m[rng.integers(0, 30, (H, W)) == 0] = np.nan
    return m


@functools.lru_cache(maxsize=None)
def _case(name):
    """name -> (vertices, faces, [(view, tan, size, face_idx, target, mask)]).  face_idx is MeshRenderer's own image of the valid mesh, then
    edited by hand where the case says so."""
    from diff_recon_hip import MeshRenderer
    rng = np.random.default_rng({"a": 1, "b": 2, "c": 3, "e": 5}[name])
    if name == "a":
        v = np.array([[-6, -4, 0.2], [6, -4.5, -0.1], [0.3, 8, 0.3]], np.float32)  # every vertex in front of znear = 1 in both views
        f = np.array([[0, 1, 2]], np.int32)
        cams = [((0.3, -0.2, -3.0), (0.5, 0.42), BIG), ((-0.4, 0.5, -2.5), (0.45, 0.5), SMALL)]
    elif name in ("b", "e"):
        v, f = _grid(6)
        cams = [((0.5, -0.4, -3.2), (0.45, 0.4), BIG), ((-1.5, 0.8, -2.6), (0.5, 0.3), SMALL)]
    else:
        v, f = _grid(2)
        f = f[:7]
        cams = [((0.2, 0.3, -3.0), (0.5, 0.3), SMALL)]
    views = []
    for k, (eye, tan, size) in enumerate(cams):
        view = ref.look_at_view(eye)
        fi = MeshRenderer(_cam(view, tan, size)).render(vertices=_dev(v), faces=_dev(f), faces_color=torch.zeros((len(f), 3), device=DEV))
        fi = fi["face_idx"].cpu().numpy().copy()
        assert (fi >= 0).sum() > 100
        if name == "a":
            assert (fi == 0).all()  # the triangle covers the whole view
        if name == "c":
            assert (fi == 6).any() and len(np.unique(fi[fi >= 0])) == 7
            fi[fi == 6] = -1  # face 6 wins no pixel: it takes the caller's fallback, or the fill
        if name == "e":
            fi[0, :4] = (-1, len(f), INT32_MIN, INT32_MAX)
            fi[1, :6] = (3, 10, 20, 21, 20, 21)  # the four edited faces below, whatever covers those pixels
            fi[2, 5:9] = 21
        views.append((view, tan, size, fi, _image(rng, size), _mask(rng, size) if k == 1 else None))
    if name == "e":
        f = f.copy()
        f[3], f[10], f[20], f[21] = (-1, 2, 5), (4, len(v), 9), (7, 7, 15), (8, 8, 8)
    return v, f, views


# (b) at R = 2 besides: 12 words per face on groups of 16 lanes, four faces to a wave with idle lanes inside every group of the face totals
CASES = [("a", 2), ("a", 8), ("b", 1), ("b", 2), ("b", 3), ("b", 8), ("c", 64), ("e", 1), ("e", 3), ("e", 8)]


@functools.lru_cache(maxsize=None)
def _reference(name, R):
    """Per view (texel_idx, atlas_idx, bary), and the accumulator after all views."""
    v, f, views = _case(name)
    lay = tref.layout(len(f), R)
    per_view = [tref.texel_index(view, tan[0], tan[1], size[0], size[1], v, f, fi, R, lay[2]) for view, tan, size, fi, _, _ in views]
    acc = np.zeros((len(f) * lay[1], 4), np.int64)
    for (texel, _, _), (_, _, _, _, target, mask) in zip(per_view, views):
        tref.accumulate(acc, texel, target, mask)
    for a in (*[x for t in per_view for x in t], acc):
        a.setflags(write=False)
    return lay, per_view, acc


def _atlas(name, R, order):
    from diff_recon_hip import TextureAtlas
    v, f, views = _case(name)
    atlas = TextureAtlas(len(f), R, DEV)
    for k in order:
        view, tan, size, fi, target, mask = views[k]
        atlas.add(_cam(view, tan, size), _dev(v), _dev(f), _dev(fi), _dev(target), None if mask is None else _dev(mask))
    return atlas


@pytest.mark.parametrize("name,R", CASES)
def test_texel_index_matches_the_reference_and_the_interpolation_bit_for_bit(name, R):
    from diff_recon_hip import atlas_layout, interpolate_vertex_attributes, texel_index
    v, f, views = _case(name)
    lay, per_view, _ = _reference(name, R)
    layout = atlas_layout(len(f), R)
    assert tuple(layout) == lay
    T = lay[1]
    for (view, tan, size, fi, _, _), (texel, atlas, bary) in zip(views, per_view):
        cam = _cam(view, tan, size)
        got_t, got_a, got_b = texel_index(cam, _dev(v), _dev(f), _dev(fi), layout, return_atlas_idx=True, return_bary=True)
        _same(got_t, texel, "texel_idx")
        _same(got_a, atlas, "atlas_idx")
        _same(got_b, bary, "bary")
        _same(texel_index(cam, _dev(v), _dev(f), _dev(fi), layout), texel, "texel_idx alone")
        _, interp = interpolate_vertex_attributes(cam, _dev(v), _dev(f), _dev(fi), torch.zeros((len(v), 1), device=DEV), torch.zeros(1, device=DEV),
                                                  return_bary=True)
        assert torch.equal(got_b.view(torch.int32), interp.view(torch.int32))  # one source: csrc/ts_mesh_bary.h
        drawn = texel >= 0
        print(name, R, size, "drawn", int(drawn.sum()), "texels hit", len(np.unique(texel[drawn])), "of", len(f) * T)
        assert drawn.any() and ((texel[drawn] // T) == fi[drawn]).all() and (atlas[drawn] < lay[4] * lay[5]).all()
        if R == 1:
            assert (texel[drawn] == fi[drawn]).all()
    if name == "a":  # the view lies inside a few texels of the one face: up to thousands of pixels each, in runs that cross waves and rows
        assert np.bincount(per_view[0][0].reshape(-1)).max() > (1000 if R == 2 else 500)
    if name == "e" and R == 3:  # the face that names one vertex three times: 1.0 / 3.0 each, (1.0 / 3.0) * 3 == 1.0, so texel (1, 1)
        texel, _, bary = per_view[0]
        assert (texel[2, 5:9] == tref.compact_index(21, 1, 1, 3)).all() and (bary[:, 2, 5:9] == np.float32(1.0 / 3.0)).all()
        assert (texel[0, :4] == -1).all() and (texel[1, :2] == -1).all() and (texel[1, 2] >= 0)  # wild indices and bad rows draw nothing


@pytest.mark.parametrize("name,R", CASES)
def test_accumulator_is_the_reference_in_any_view_order_and_atlases_add(name, R):
    from diff_recon_hip import MeshCensus
    v, f, views = _case(name)
    lay, per_view, want = _reference(name, R)
    n = len(views)
    forward = _atlas(name, R, range(n))
    _same(forward.texels, want, "texels")
    assert int(want[:, 0].sum()) > 100
    _same(_atlas(name, R, reversed(range(n))).texels, want, "texels, views reversed")
    first, second = _atlas(name, R, [0]), _atlas(name, R, range(1, n))
    first += second
    _same(first.texels, want, "two atlases added")
    # the census of the faces over the same views: the state itself at R == 1, the face totals otherwise.  A pixel whose face_idx names a face
    # with a bad row is counted by MeshCensus and not drawn here, so in (e) the census gets face_idx with those pixels cleared.
    census = MeshCensus(len(f), DEV)
    for (_, _, _, fi, target, mask), (texel, _, _) in zip(views, per_view):
        census.add(_dev(np.where(texel >= 0, fi, -1).astype(np.int32)), _dev(target), None if mask is None else _dev(mask))
    if R == 1:
        assert torch.equal(forward.texels, census.acc)
    totals = forward.face_totals()
    _same(totals, tref.face_totals(want, len(f), R), "face_totals")
    assert torch.equal(totals, census.acc)


@pytest.mark.parametrize("name,R", CASES)
@pytest.mark.parametrize("min_count", [1, 3])
def test_resolve_matches_the_reference_bit_for_bit(name, R, min_count):
    v, f, views = _case(name)
    lay, _, acc = _reference(name, R)
    atlas = _atlas(name, R, range(len(views)))
    F = len(f)
    rng = np.random.default_rng(17)
    fallback = rng.uniform(-0.5, 1.5, (F, 3)).astype(np.float32)
    fallback[0, 1] = np.nan
    seen = set()
    for fb, fill in ((None, 0.5), (fallback, (0.125, -0.25, 1.75))):
        fill3 = (fill,) * 3 if isinstance(fill, float) else fill
        image, state, rgb8 = tref.resolve(acc, F, R, lay[2], lay[3], min_count, fb, fill3)
        baked = atlas.resolve(min_count, None if fb is None else _dev(fb), fill)
        _same(baked.image, image, "image")
        _same(baked.state, state, "state")
        _same(baked.rgb8, rgb8, "rgb8")
        _same(baked.uv, tref.face_uvs(F, R, lay[2], lay[3]), "uv")
        assert tuple(baked.layout) == lay
        seen |= {(fb is not None, int(s)) for s in np.unique(state)}
        print(name, R, min_count, "fallback" if fb is not None else "no fallback", {int(s): int((state == s).sum()) for s in np.unique(state)})
    if name == "c" and min_count == 1:  # every rule fires: own mean, face mean, the fallback of the face that won nothing, the fill of the empty half-cell
        assert {s for with_fb, s in seen if with_fb} == {0, 1, 2, 3} and {s for with_fb, s in seen if not with_fb} == {0, 2, 3}


@pytest.mark.parametrize("name,R", CASES)
def test_render_textured_matches_the_reference(name, R):
    """MeshRenderer draws no face whose row names an index outside [0, V) or collapses (include/ts_mesh.h), so in (e) the four edited faces leave
    the background where they were and their neighbours keep their pixels."""
    from diff_recon_hip import render_textured
    v, f, views = _case(name)
    lay, _, acc = _reference(name, R)
    baked = _atlas(name, R, range(len(views))).resolve(1, None, (0.25, 0.5, 2.0))
    image, _, _ = tref.resolve(acc, len(f), R, lay[2], lay[3], 1, None, (0.25, 0.5, 2.0))
    bg = np.array([0.1, -0.2, 1.3], np.float32)
    for view, tan, size, _, _, _ in views:
        out = render_textured(_cam(view, tan, size), _dev(v), _dev(f), baked, _dev(bg))
        fi = out["face_idx"].cpu().numpy()
        _, atlas_idx, _ = tref.texel_index(view, tan[0], tan[1], size[0], size[1], v, f, fi, R, lay[2])
        want = np.clip(tref.render(atlas_idx, image, bg), 0.0, 1.0).astype(np.float32).reshape(3, size[1], size[0])
        _same(out["render"], want, "render")
        assert out["mask"].shape == (1, size[1], size[0]) and out["depth"].shape == (size[1], size[0])
        if name == "e":
            assert not np.isin(fi, (3, 10, 20, 21)).any() and (fi >= 0).sum() > 100 and (atlas_idx >= 0).sum() == (fi >= 0).sum()


def test_the_draw_reads_nothing_out_of_bounds_for_any_index():
    from diff_recon_hip import mesh_texture as mt
    rng = np.random.default_rng(8)
    (W, H), Wa, Ha = SMALL, 9, 6
    idx = rng.integers(-3, Wa * Ha + 3, (H, W)).astype(np.int32)
    idx[0, :4] = (INT32_MIN, INT32_MAX, Wa * Ha, -1)
    image = rng.uniform(-1, 2, (3, Ha, Wa)).astype(np.float32)
    bg = np.array([0.5, np.nan, -7.0], np.float32)
    out = torch.empty((3, H, W), device=DEV)
    idx_d, image_d, bg_d = _dev(idx), _dev(image), _dev(bg)  # held until the kernel has run
    mt._check(mt._lib.tsa_render(W, H, Wa, Ha, idx_d.data_ptr(), image_d.data_ptr(), bg_d.data_ptr(), out.data_ptr(), None), "render")
    torch.cuda.synchronize()
    _same(out, tref.render(idx, image, bg).reshape(3, H, W), "render")


@pytest.mark.parametrize("R", [3, 8])
def test_texels_refine_the_face_colours_on_the_bake_s_own_view(R):
    """(b), baked from one view with that view as the target (its values multiples of 2^-16, so the Q16 sums hold them exactly): the mean
    of a texel's pixels is the best constant on them, and the texels of a face partition its pixels, so the summed squared error of the
    textured render is at most that of bake_face_colors' render -- up to the fp32 rounding of either output, at most 2^-24 relative on
    values of at most 1 and errors of at most 1: 3 H W 2^-23 in all.  Both sums in float64."""
    from diff_recon_hip import MeshRenderer, bake_face_colors, bake_texture, render_textured
    v, f, views = _case("b")
    view, tan, size, _, _, _ = views[0]
    W, H = size
    target = (np.random.default_rng(31).integers(0, 65537, (3, H, W)).astype(np.float64) / 65536.0).astype(np.float32)
    cam = SimpleNamespace(**vars(_cam(view, tan, size)), gt_image=_dev(target))
    vd, fd = _dev(v), _dev(f)
    baked = bake_texture([cam], vd, fd, R)
    out = render_textured(cam, vd, fd, baked)
    textured, covered = out["render"].cpu().numpy().astype(np.float64), (out["mask"] > 0).cpu().numpy().reshape(H, W)
    colours = bake_face_colors([cam], vd, fd, torch.full((len(f), 3), 0.5, device=DEV))
    flat = MeshRenderer(cam).render(vertices=vd, faces=fd, faces_color=colours)["render"].cpu().numpy().astype(np.float64)
    sse_t, sse_f = float(((textured - target) ** 2).sum()), float(((flat - target) ** 2).sum())
    print("R", R, "sse textured", sse_t, "sse per face", sse_f, "margin", 3 * H * W * 2.0 ** -23)
    assert sse_t <= sse_f + 3 * H * W * 2.0 ** -23
    on_mesh_t, on_mesh_f = float(((textured - target)[:, covered] ** 2).sum()), float(((flat - target)[:, covered] ** 2).sum())
    assert covered.sum() > 500 and on_mesh_t < 0.9 * on_mesh_f  # and on noise the refinement is not marginal where the mesh is drawn


def test_no_faces_and_no_vertices():
    from diff_recon_hip import TextureAtlas, atlas_layout, mesh_texture as mt, texel_index
    view, tan, size = ref.look_at_view((0.3, -0.2, -3.0)), (0.5, 0.4), SMALL
    W, H = size
    cam = _cam(view, tan, size)
    fi = _dev(np.random.default_rng(4).integers(-2, 5, (H, W)).astype(np.int32))
    nov, nof = torch.zeros((0, 3), device=DEV), torch.zeros((0, 3), device=DEV, dtype=torch.int32)
    for vertices, faces in ((nov, nof), (torch.zeros((5, 3), device=DEV), nof), (nov, torch.zeros((3, 3), device=DEV, dtype=torch.int32))):
        F = faces.shape[0]
        texel, atlas, bary = texel_index(cam, vertices, faces, fi, atlas_layout(F, 4), return_atlas_idx=True, return_bary=True)
        assert (texel == -1).all() and (atlas == -1).all() and (bary == 0).all()
    empty = TextureAtlas(0, 4, DEV)
    empty.add(cam, nov, nof, fi, torch.rand((3, H, W), device=DEV))
    assert empty.texels.shape == (0, 4) and empty.face_totals().shape == (0, 4)
    baked = empty.resolve(fill=(0.25, 0.5, 0.75))
    assert tuple(baked.layout) == (4, 10, 1, 1, 5, 4) and baked.uv.shape == (0, 3, 2)
    assert (baked.state == 0).all() and all((baked.image[c] == x).all() for c, x in enumerate((0.25, 0.5, 0.75)))
    assert (baked.rgb8.reshape(-1, 3).cpu() == torch.tensor([64, 128, 191], dtype=torch.uint8)).all()
    drawn = mt.render_textured(cam, nov, nof, baked, torch.tensor([0.25, -1.0, 3.0]))  # the empty mesh through MeshRenderer as well
    assert all((drawn["render"][c] == x).all() for c, x in enumerate((0.25, 0.0, 1.0))) and (drawn["face_idx"] == -1).all() and not drawn["mask"].any()
    out = torch.empty((3, H, W), device=DEV)
    bg = _dev(np.float32([1, 2, 3]))
    mt._check(mt._lib.tsa_render(W, H, 5, 4, atlas.data_ptr(), baked.image.data_ptr(), bg.data_ptr(), out.data_ptr(), None), "render")
    assert all((out[c] == c + 1).all() for c in range(3))


def test_argument_checks_return_before_anything_is_written():
    """Every TS2D_ERR_INVALID case of the header and the capacity cases, on the C ABI itself: the code comes back, the error text is set,
    and the outputs -- poisoned -- are untouched."""
    from diff_recon_hip import mesh_texture as mt
    lib = mt._lib
    W, H = SMALL
    F, V, R, Cx, Cy = 4, 5, 3, 2, 1
    T = 6
    canary = 0x5A
    outs = {k: torch.full((n,), canary, device=DEV, dtype=torch.uint8) for k, n in
            (("texel", 4 * W * H), ("atlas", 4 * W * H), ("bary", 12 * W * H), ("totals", 32 * F), ("image", 12 * Cx * (R + 1) * Cy * R),
             ("state", Cx * (R + 1) * Cy * R), ("rgb8", 3 * Cx * (R + 1) * Cy * R), ("out", 12 * W * H))}
    p = {k: t.data_ptr() for k, t in outs.items()}
    view, vertices = torch.eye(4, device=DEV), torch.zeros((V, 3), device=DEV)
    faces, fi = torch.zeros((F, 3), device=DEV, dtype=torch.int32), torch.zeros((H, W), device=DEV, dtype=torch.int32)
    texels, image = torch.zeros((F * T, 4), device=DEV, dtype=torch.int64), torch.zeros((3, Cy * R, Cx * (R + 1)), device=DEV)
    bg = torch.zeros(3, device=DEV)
    fill = (C.c_float * 3)(0.5, 0.5, 0.5)
    nan, inf = float("nan"), float("inf")

    def index(**kw):
        a = dict(view=view.data_ptr(), tx=0.5, ty=0.5, W=W, H=H, V=V, vertices=vertices.data_ptr(), F=F, faces=faces.data_ptr(), fi=fi.data_ptr(), R=R,
                 Cx=Cx, texel=p["texel"], atlas=p["atlas"], bary=p["bary"])
        a.update(kw)
        return lib.tsa_texel_index(a["view"], a["tx"], a["ty"], a["W"], a["H"], a["V"], a["vertices"], a["F"], a["faces"], a["fi"], a["R"], a["Cx"],
                                   a["texel"], a["atlas"], a["bary"], None)

    def totals(**kw):
        a = dict(F=F, R=R, texels=texels.data_ptr(), totals=p["totals"])
        a.update(kw)
        return lib.tsa_face_totals(a["F"], a["R"], a["texels"], a["totals"], None)

    def resolve(**kw):
        a = dict(F=F, R=R, Cx=Cx, Cy=Cy, texels=texels.data_ptr(), totals=p["totals"], min_count=1, fallback=None, fill=fill, image=p["image"],
                 state=p["state"], rgb8=p["rgb8"])
        a.update(kw)
        return lib.tsa_resolve(a["F"], a["R"], a["Cx"], a["Cy"], a["texels"], a["totals"], a["min_count"], a["fallback"], a["fill"], a["image"],
                               a["state"], a["rgb8"], None)

    def render(**kw):
        a = dict(W=W, H=H, Wa=Cx * (R + 1), Ha=Cy * R, atlas=fi.data_ptr(), image=image.data_ptr(), bg=bg.data_ptr(), out=p["out"])
        a.update(kw)
        return lib.tsa_render(a["W"], a["H"], a["Wa"], a["Ha"], a["atlas"], a["image"], a["bg"], a["out"], None)

    invalid = [lambda: index(V=-1), lambda: index(F=-1), lambda: index(W=0), lambda: index(H=-3), lambda: index(R=0), lambda: index(R=65),
               lambda: index(Cx=0), lambda: index(tx=nan), lambda: index(ty=inf), lambda: index(tx=-inf), lambda: index(view=None),
               lambda: index(fi=None), lambda: index(texel=None), lambda: index(vertices=None), lambda: index(faces=None),
               lambda: totals(F=-1), lambda: totals(R=0), lambda: totals(R=65), lambda: totals(texels=None), lambda: totals(totals=None),
               lambda: resolve(F=-1), lambda: resolve(R=0), lambda: resolve(R=65), lambda: resolve(Cx=0), lambda: resolve(Cy=0),
               lambda: resolve(Cx=1, Cy=1), lambda: resolve(min_count=0), lambda: resolve(min_count=-2), lambda: resolve(fill=None),
               lambda: resolve(image=None), lambda: resolve(state=None), lambda: resolve(texels=None), lambda: resolve(totals=None),
               lambda: render(W=0), lambda: render(H=-1), lambda: render(Wa=0), lambda: render(Ha=0), lambda: render(atlas=None),
               lambda: render(image=None), lambda: render(bg=None), lambda: render(out=None)]
    for k, call in enumerate(invalid):
        assert call() == 1 and lib.tsa_last_error(), k  # TS2D_ERR_INVALID
    capacity = [lambda: index(F=2 ** 21, R=64),              # F T = 2^21 * 2080 texels
                lambda: index(F=INT32_MAX, R=1, Cx=1),       # F T fits; the atlas is 2 x 2^30
                lambda: index(W=2 ** 16, H=2 ** 15),         # 2^31 pixels
                lambda: totals(F=2 ** 21, R=64),
                lambda: resolve(F=2 ** 21, R=64), lambda: resolve(Cx=2 ** 20, Cy=2 ** 10),
                lambda: render(Wa=2 ** 16, Ha=2 ** 15), lambda: render(W=2 ** 16, H=2 ** 15)]
    for k, call in enumerate(capacity):
        assert call() == 3 and lib.tsa_last_error(), k  # TS2D_ERR_CAPACITY
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == canary).all()), k
    # the same arguments without a fault are accepted: the cases above failed for the reason they name
    assert index() == 0 and totals() == 0 and resolve() == 0 and render() == 0
    torch.cuda.synchronize()
    assert all(bool((outs[k] != canary).any()) for k in ("texel", "atlas", "totals", "image", "state", "rgb8", "out"))


def test_every_call_is_pure():
    """Every output overwritten in full from a poisoned state, nothing outside an output's extent written, identical results from every poison."""
    from diff_recon_hip import mesh_texture as mt
    runs = []
    for name, R in (("e", 3), ("c", 64)):
        v, f, views = _case(name)
        view, tan, size, fi, _, _ = views[0]
        runs.append((name, R, _cam(view, tan, size), _dev(v), _dev(f), _dev(fi), _atlas(name, R, range(len(views))), size))
    bg = _dev(np.float32([0.1, 0.2, 0.3]))
    fallback = {name: _dev(np.linspace(0, 1, 3 * len(_case(name)[1]), dtype=np.float32).reshape(-1, 3)) for name in ("e", "c")}

    def call(pattern):
        out = {}
        for name, R, cam, vd, fd, fid, atlas, (W, H) in runs:
            texel, atlas_idx, bary = mt.texel_index(cam, vd, fd, fid, atlas.layout, return_atlas_idx=True, return_bary=True)
            baked = atlas.resolve(2, fallback[name], 0.5)
            drawn = torch.empty((3, H, W), device=DEV)
            mt._check(mt._lib.tsa_render(W, H, baked.layout.width, baked.layout.height, atlas_idx.data_ptr(), baked.image.data_ptr(), bg.data_ptr(),
                                         drawn.data_ptr(), None), "render")
            out.update({f"{name}.texel": texel, f"{name}.atlas": atlas_idx, f"{name}.bary": bary, f"{name}.totals": atlas.face_totals(),
                        f"{name}.image": baked.image, f"{name}.state": baked.state, f"{name}.rgb8": baked.rgb8, f"{name}.render": drawn})
        return out

    base = poison.assert_pure(call)
    lay, per_view, acc = _reference("e", 3)
    assert np.array_equal(base["e.texel"].numpy().view(np.int32).reshape(per_view[0][0].shape), per_view[0][0])


def test_example_reports_and_writes_the_textured_fused_mesh(tmp_path):
    import os
    import sys
    from diff_recon_hip.mesh_renderer import load_glb_mesh
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    out = tmp_path / "fused.glb"
    res = train_synthetic.mesh_scores(m, "2D", extract=32, extract_color=True, texture=4, out=str(out), **cfg)
    t = res["fused"]["texture"]
    lines = train_synthetic.fused_texture_report(t)
    print("\n".join(train_synthetic.fused_color_report(res["fused"]["color"]) + lines))
    assert len(lines) == 2 and lines[0].startswith(f"fused mesh, a {t['width']} x {t['height']} atlas of 4 texels per face edge baked from the 2 training views")
    assert "mean PSNR" in lines[0] and "mean SSIM" in lines[0] and lines[1] == f"textured mesh written to {out}"
    assert np.isfinite(t["mean_psnr"]) and np.isfinite(t["mean_ssim"]) and len(t["psnr"]) == 2 and 0 < t["observed"] <= t["texels"] == 10 * t["faces"]
    v, f, _ = load_glb_mesh(str(out), "cpu")
    assert f.shape[0] == t["faces"] and v.shape[0] == 3 * t["faces"]
    plain = train_synthetic.mesh_scores(m, "2D", extract=32, **cfg)["fused"]
    assert "texture" not in plain and plain["topology"] == res["fused"]["topology"]  # without the flag nothing changes
