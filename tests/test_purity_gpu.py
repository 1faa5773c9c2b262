"""Purity of the entry points (DESIGN.md "Purity of the entry points"): every family of include/*.h is run on workspaces, state buffers and
outputs that hold a poison pattern on entry (tests/poison.py) and must return, bit for bit, what it returns on zero-filled ones; guard bands
around every buffer must stay intact.  Most calls go through ctypes on the C ABI, where the test owns every buffer and the header's own words
("fully written", "overwritten", "receives") are what is tested; the geometry scores and some forwards go through the Python wrappers
under PoisonedEmpty.  Shapes are the smallest at which a grid, a finisher or a tail can go wrong, not the workload's.

The assertions are equalities of raw bytes; there is no tolerance and no outlier budget in this file, except where the rasterizer family
says so: outputs accumulated with float atomics are held to the bars of tests/test_parity_gpu.py instead."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import poison
from test_purity_cpu import check_positive_control

pytestmark = pytest.mark.gpu

DEV = "cuda"
U8, I32, I64, F32, F64 = torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64


@functools.lru_cache(None)
def lib():
    from diff_triangle_rasterization_2D import _C as native
    return native._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def ok(rc):
    assert rc == 0, f"ts2d error {rc}: {lib().ts2d_last_error().decode()}"


def buf(shape, dtype):
    """A poisoned, guarded device tensor of the active pattern."""
    return poison.filled(shape, dtype, device=DEV)


def rnd(seed, *shape, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo).to(DEV)


def check_family(op, ws_bytes, sizes, large, small):
    """`op(size, ws)` runs the family's calls for one problem size in the workspace `ws` (None: a fresh poisoned one) and returns the dict of
    its documented outputs.  Every size goes through poison.assert_pure; then ONE workspace object, poisoned once, serves
    large -> small -> large, each result compared with its fresh-workspace baseline (what densification and changing views do)."""
    base = {}
    for size in sizes:
        base[size] = poison.assert_pure(lambda pattern, size=size: op(size, None))
    with poison.PoisonedEmpty("nan") as pe:
        ws = buf(max(ws_bytes(large), ws_bytes(small)), U8)
        for size in (large, small, large):
            diff = poison._first_difference(base[size], poison._snapshot(op(size, ws), None))
            assert diff is None, f"workspace reused for size {size} after another problem: {diff}"
            pe.check_guards()
    return base


def test_positive_control_on_the_device():
    check_positive_control(DEV)


# ---- losses --------------------------------------------------------------------------------------------------------------------------------
# photometric: one partial per 32 x 16 tile, the finisher's 1024 threads stride over them: (1, 528, 1056) has 33 x 33 = 1089 tiles
PHOTO_SHAPES = [(3, 5, 7), (1, 16, 32), (4, 33, 31), (1, 528, 1056)]


def photometric(shape, ws):
    c, h, w = shape
    L = lib()
    img, gt, go = rnd(1, c, h, w), rnd(2, c, h, w), torch.tensor([0.75], device=DEV)
    n = L.tsl_workspace_bytes(c, h, w)
    ws = buf(n, U8) if ws is None else ws
    out, out_eval, grad = buf(3, F32), buf(3, F32), buf((c, h, w), F32)
    ok(L.tsl_photometric_forward(ptr(img), ptr(gt), c, h, w, 0.8, 0.2, 1, ptr(ws), n, ptr(out), stream()))
    ok(L.tsl_photometric_backward(ptr(img), ptr(gt), c, h, w, 0.8, 0.2, ptr(ws), n, ptr(go), ptr(grad), stream()))
    ok(L.tsl_photometric_forward(ptr(img), ptr(gt), c, h, w, 0.8, 0.2, 0, ptr(ws), n, ptr(out_eval), stream()))  # need_grad = 0 on a used workspace
    return dict(out=out, grad=grad, out_eval=out_eval)


def test_photometric_loss():
    check_family(photometric, lambda s: lib().tsl_workspace_bytes(*s), PHOTO_SHAPES, PHOTO_SHAPES[3], PHOTO_SHAPES[0])


def test_photometric_loss_through_the_wrapper():
    from diff_recon_hip.losses import photometric_loss
    img, gt = rnd(1, 4, 33, 31), rnd(2, 4, 33, 31)
    poison.assert_pure(lambda p: photometric_loss(img, gt, 0.8, 0.2))


# depth / normal: SUM_BLOCKS = 1024 blocks of 256 pixels; 33 x 41 is the smallest golden case, 513 x 512 is 512 pixels above 1024 * 256
DN_SHAPES = [(33, 41), (513, 512)]
DN_CASES = [(s, q, scale) for s in DN_SHAPES for q in (0.0, 0.3, 0.9, 1.0) for scale in (0.5, None)]


def depth_normal(case, ws):
    (h, w), q, scale = case
    L = lib()
    scale = 1.0 if scale is None else scale
    depth, normal, go = rnd(3, h, w, lo=1.0, hi=3.0), rnd(4, 3, h, w, lo=-1.0, hi=1.0), torch.tensor([1.5], device=DEV)
    n = L.tsl_depth_normal_workspace_bytes(h, w, scale)
    ws = buf(n, U8) if ws is None else ws
    out, dd, dn, dn_only = buf(1, F32), buf((h, w), F32), buf((3, h, w), F32), buf((3, h, w), F32)
    ok(L.tsl_depth_normal_forward(ptr(depth), ptr(normal), h, w, 0.7, 0.5, scale, q, ptr(ws), n, ptr(out), stream()))
    ok(L.tsl_depth_normal_backward(ptr(depth), ptr(normal), h, w, 0.7, 0.5, scale, ptr(ws), n, ptr(go), ptr(dd), ptr(dn), stream()))
    ok(L.tsl_depth_normal_backward(ptr(depth), ptr(normal), h, w, 0.7, 0.5, scale, ptr(ws), n, ptr(go), None, ptr(dn_only), stream()))
    return dict(out=out, ddepth=dd, dnormal=dn, dnormal_only=dn_only)


def test_depth_normal_loss():
    ws_bytes = lambda case: lib().tsl_depth_normal_workspace_bytes(case[0][0], case[0][1], 1.0 if case[2] is None else case[2])
    check_family(depth_normal, ws_bytes, DN_CASES, ((513, 512), 0.9, None), ((33, 41), 0.3, 0.5))


def test_depth_normal_loss_through_the_wrapper():
    from diff_recon_hip.losses import DepthNormalLoss
    depth, normal = rnd(3, 33, 41, lo=1.0, hi=3.0), rnd(4, 3, 33, 41, lo=-1.0, hi=1.0)
    poison.assert_pure(lambda p: DepthNormalLoss(scale_factor=0.5)(depth, normal, 0.7, 0.5))


AUX_CASES = [((3, 5, 7), 0.5), ((1, 16, 32), None), ((4, 33, 31), 0.5), ((2, 513, 512), 0.5)]


def aux_losses(case, ws):
    (c, h, w), scale = case
    L = lib()
    scale = 1.0 if scale is None else scale
    img, gt, go = rnd(5, c, h, w), rnd(6, c, h, w), torch.tensor([0.5], device=DEV)
    n = L.tsl_aux_loss_workspace_bytes(c, h, w, scale)
    ws = buf(n, U8) if ws is None else ws
    dog, smooth = buf((h, w), F32), buf((h, w), F32)
    l1, dl1, sm, dsm = buf(1, F32), buf((c, h, w), F32), buf(1, F32), buf((c, h, w), F32)
    ok(L.tsl_dog_mask(ptr(gt), c, h, w, 1.0, 7, 1.6, 11, 1, scale, ptr(ws), n, ptr(dog), stream()))
    ok(L.tsl_masked_l1_forward(ptr(img), ptr(gt), ptr(dog), c, h, w, ptr(ws), n, ptr(l1), stream()))
    ok(L.tsl_masked_l1_backward(ptr(img), ptr(gt), ptr(dog), c, h, w, ptr(go), ptr(dl1), stream()))
    ok(L.tsl_smoothness_mask(ptr(gt), c, h, w, scale, 0.3, ptr(ws), n, ptr(smooth), stream()))
    ok(L.tsl_scharr_smoothness_forward(ptr(img), ptr(smooth), c, h, w, ptr(ws), n, ptr(sm), stream()))
    ok(L.tsl_scharr_smoothness_backward(ptr(img), ptr(smooth), c, h, w, ptr(ws), n, ptr(go), ptr(dsm), stream()))
    return dict(dog=dog, smooth=smooth, l1=l1, dl1=dl1, sm=sm, dsm=dsm)


def test_aux_losses():
    ws_bytes = lambda case: lib().tsl_aux_loss_workspace_bytes(*case[0], 1.0 if case[1] is None else case[1])
    check_family(aux_losses, ws_bytes, AUX_CASES, AUX_CASES[3], AUX_CASES[0])


def test_downsample():
    """No workspace: the outputs are fully written and nothing around them is.  The _planes form with every plane base 4 bytes off an 8-byte
    boundary takes the general kernels at factor 2 where the aligned call takes the float2 ones; both must give the same bits."""
    L = lib()
    for (c, h, w), f in (((3, 6, 10), 2), ((1, 5, 67), 3), ((9, 4, 65), 2)):  # 9 planes: two launches of the plane groups
        H, W = f * h, f * w
        x, g = rnd(7, c, H, W), rnd(8, c, h, w)
        xo, go_ = torch.zeros(c * H * W + 1, device=DEV), torch.zeros(c * h * w + 1, device=DEV)
        xo[1:] = x.reshape(-1)  # the same values, every plane 4 bytes off
        assert xo[1:].data_ptr() % 8 == 4

        def run(pattern):
            out, gin = buf((c, h, w), F32), buf((c, H, W), F32)
            ok(L.tsl_downsample_forward(ptr(x), c, H, W, h, w, ptr(out), stream()))
            ok(L.tsl_downsample_backward(ptr(g), c, H, W, h, w, ptr(gin), stream()))
            # the planes form: sources 4 bytes off (forward), destinations 4 bytes off (backward)
            out_p, gin_p = buf((c, h, w), F32), buf(c * H * W + 1, F32)
            arr = C.c_void_p * c
            src = arr(*[xo.data_ptr() + 4 + 4 * k * H * W for k in range(c)])
            dst = arr(*[out_p.data_ptr() + 4 * k * h * w for k in range(c)])
            ok(L.tsl_downsample_forward_planes(c, src, H, W, h, w, dst, stream()))
            gsrc = arr(*[g.data_ptr() + 4 * k * h * w for k in range(c)])
            gdst = arr(*[gin_p.data_ptr() + 4 + 4 * k * H * W for k in range(c)])
            ok(L.tsl_downsample_backward_planes(c, gsrc, H, W, h, w, gdst, stream()))
            head = gin_p[:1].clone()
            assert torch.equal(poison.raw(head), poison.pattern_bytes(pattern, 4)), "the word in front of the first plane was written"
            return dict(out=out, gin=gin, out_planes=out_p, gin_planes=gin_p[1:])
        b = poison.assert_pure(run)
        assert torch.equal(b["out"], b["out_planes"]) and torch.equal(b["gin"], b["gin_planes"])


# ---- regularisers --------------------------------------------------------------------------------------------------------------------------
REG_P = [1, 85, 4099]  # 2048 blocks of 256 triangles would saturate at 524 288; these fill 1, 1 and 17 blocks of the fixed grid


@functools.lru_cache(None)
def reg_inputs(P):
    g = torch.Generator().manual_seed(100 + P)
    vertex = torch.randn(P, 3, 3, generator=g).to(DEV)
    opacity = torch.rand(P, 1, generator=g).to(DEV)
    nearest = torch.randint(0, 3 * P, (3 * P,), generator=g, dtype=torch.int64)
    nearest[: max(1, (3 * P) // 2)] = 2 % (3 * P)  # one vertex is the nearest of many
    if P > 1:
        nearest[-1] = 3 * P + 5                    # one index out of range: its term is NaN, nothing is read out of bounds
    return vertex, opacity, nearest.to(torch.int32).to(DEV)


def regularisers(P, ws):
    L = lib()
    vertex, opacity, nearest = reg_inputs(P)
    n, npre = L.tsl_reg_workspace_bytes(), L.tsl_reg_prepared_bytes(P)
    ws = buf(n, U8) if ws is None else ws
    prepared, go = buf(npre, U8), torch.tensor([2.0], device=DEV)
    ok(L.tsl_reg_prepare(P, ptr(nearest), ptr(prepared), npre, stream()))
    res = {}
    for w_s, wo, wv in [(a, b, c) for a in (0.0, 0.3) for b in (0.0, 0.5) for c in (0.0, 0.7)]:
        for mode in (1, 2):
            out, dv, do = buf(4, F32), buf((P, 3, 3), F32), buf((P, 1), F32)
            ok(L.tsl_reg_forward(P, ptr(vertex), ptr(opacity), ptr(nearest), w_s, wo, mode, wv, ptr(ws), n, ptr(out), stream()))
            ok(L.tsl_reg_backward(P, ptr(vertex), ptr(opacity), ptr(nearest), ptr(prepared), npre, w_s, wo, mode, wv, ptr(go), ptr(dv), ptr(do),
                                  stream()))
            key = f"s{w_s}o{wo}v{wv}m{mode}"
            res[key + "out"], res[key + "dv"], res[key + "do"] = out, dv, do
    return res


def test_regularisers():
    base = check_family(regularisers, lambda P: lib().tsl_reg_workspace_bytes(), REG_P, 4099, 1)
    for P, b in base.items():  # out[1..3] of a term that is off is exactly +0.0, both opacity modes
        for key, raw_out in b.items():
            if not key.endswith("out"):
                continue
            out = raw_out.view(F32)
            for name, slot in (("s0.0", 1), ("o0.0", 2), ("v0.0", 3)):
                if name in key:
                    assert raw_out[4 * slot:4 * slot + 4].tolist() == [0, 0, 0, 0], (P, key, slot, out)


def test_regularisers_through_the_wrapper():
    from diff_recon_hip.regularizers import triangle_regularization
    vertex, opacity, nearest = reg_inputs(85)
    near = nearest.clone()
    near[-1] = 0

    def run(pattern):  # the wrapper allocates workspace, prepared buffer, outputs and both gradients with torch.empty
        v, o = vertex.clone().requires_grad_(True), opacity.clone().requires_grad_(True)
        total, parts = triangle_regularization(v, o, near, w_scaling=0.3, w_opacity=0.5, opacity_mode="quad", w_vertex=0.7)
        total.backward()
        return dict(total=total, parts=parts, dv=v.grad, do=o.grad)
    poison.assert_pure(run)


def colour_affine(shape, ws):
    h, w = shape
    L = lib()
    img, go = rnd(9, 3, h, w, lo=-0.2, hi=1.2), rnd(10, 3, h, w, lo=-1.0, hi=1.0)
    weight, bias = (torch.eye(3) + 0.1 * torch.arange(9.0).reshape(3, 3) / 9).to(DEV), torch.tensor([0.01, -0.02, 0.03], device=DEV)
    n = L.tsl_reg_workspace_bytes()
    ws = buf(n, U8) if ws is None else ws
    out, dimg, dW, db = buf((3, h, w), F32), buf((3, h, w), F32), buf(9, F32), buf(3, F32)
    ok(L.tsl_color_affine_forward(ptr(img), h, w, ptr(weight), ptr(bias), ptr(out), stream()))
    ok(L.tsl_color_affine_backward(ptr(img), h, w, ptr(weight), ptr(bias), ptr(go), ptr(ws), n, ptr(dimg), ptr(dW), ptr(db), stream()))
    return dict(out=out, dimg=dimg, dW=dW, db=db)


def test_colour_affine():
    check_family(colour_affine, lambda s: lib().tsl_reg_workspace_bytes(), [(5, 7), (130, 70)], (130, 70), (5, 7))


# ---- k-NN (unit: the 1024-point box) ---------------------------------------------------------------------------------------------------------
def knn_mean(P, ws):
    L = lib()
    pts = rnd(11, P, 3)
    n = L.tsk_workspace_bytes(P)
    ws = buf(n, U8) if ws is None else ws
    mean = buf(P, F32)
    ok(L.tsk_mean_dist3(P, ptr(pts), ptr(mean), ptr(ws), n, stream()))
    return dict(mean=mean)


def knn_nearest(case, ws):
    P, group = case
    L = lib()
    pts = rnd(12, P, 3)
    n = L.tsk_workspace_bytes(P)
    ws = buf(n, U8) if ws is None else ws
    nearest = buf(P, I32)
    ok(L.tsk_nearest_other(P, group, ptr(pts), ptr(nearest), ptr(ws), n, stream()))
    return dict(nearest=nearest)


def test_knn():
    check_family(knn_mean, lambda P: lib().tsk_workspace_bytes(P), [1, 3, 1000, 1025, 5000], 5000, 3)
    cases = [(3, 3), (999, 3), (1026, 3), (5001, 3), (4096, 1024)]
    check_family(knn_nearest, lambda c: lib().tsk_workspace_bytes(c[0]), cases, (5001, 3), (3, 3))


# ---- geometry scores -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def glib():
    import importlib
    return importlib.import_module("diff_recon_hip.mesh_distance")._lib  # (the package also exports a FUNCTION of that name)


def gok(rc):
    assert rc == 0, f"error {rc}: {glib().tsg_last_error().decode()}"


def nearest_cross(case, ws):
    Q, R = case
    G = glib()
    q, r = rnd(13, Q, 3), rnd(14, R, 3)
    n = G.tsg_cross_workspace_bytes(Q, R)
    ws = buf(n, U8) if ws is None else ws
    idx, d2 = buf(Q, I32), buf(Q, F32)
    gok(G.tsg_nearest_cross(Q, ptr(q), R, ptr(r), ptr(idx), ptr(d2), None, ptr(ws), n, stream()))
    return dict(idx=idx, d2=d2)


@functools.lru_cache(None)
def soup(F, seed=15):
    g = torch.Generator().manual_seed(seed + F)
    centre = torch.rand(F, 1, 3, generator=g)
    return (centre + 0.05 * torch.randn(F, 3, 3, generator=g)).reshape(-1, 3).to(DEV), torch.arange(3 * F, dtype=torch.int32).reshape(F, 3).to(DEV)


def sample_surface(case, ws):
    F, N = case
    G = glib()
    v, f = soup(F)
    n = G.tsg_sample_workspace_bytes(F)
    ws = buf(n, U8) if ws is None else ws
    area, pts, face = buf(F, F64), buf((N, 3), F32), buf(N, I32)
    gok(G.tsg_face_areas(3 * F, F, ptr(v), ptr(f), None, ptr(area), stream()))
    gok(G.tsg_sample_surface(3 * F, F, ptr(v), ptr(f), ptr(area), N, 1234, ptr(pts), ptr(face), ptr(ws), n, stream()))
    return dict(area=area, pts=pts, face=face)


def test_geometry_scores():
    cases = [(1, 1), (1000, 1025), (1025, 1000)]
    check_family(nearest_cross, lambda c: glib().tsg_cross_workspace_bytes(*c), cases, (1025, 1000), (1, 1))
    cases = [(F, N) for F in (1, 300, 1025) for N in (1, 1000)]
    check_family(sample_surface, lambda c: glib().tsg_sample_workspace_bytes(c[0]), cases, (1025, 1000), (1, 1))


def test_geometry_scores_through_the_wrappers():
    import importlib
    md = importlib.import_module("diff_recon_hip.mesh_distance")
    q, r = rnd(13, 1000, 3), rnd(14, 1025, 3)
    v, f = soup(300)
    poison.assert_pure(lambda p: md.nearest_points(q, r))
    poison.assert_pure(lambda p: (lambda s: (s.points, s.face))(md.sample_mesh_surface(v, f, 1000, seed=5)))


# ---- weld ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def weld_inputs(F):
    v, f = soup(F, seed=16)
    v, f = v.clone(), f.clone()
    V = 3 * F
    for a, b in ((0, 1), (2, V - 1), (V // 2, V // 3)):  # a few vertices coincide exactly
        v[b] = v[a]
    f[F - 1, 2] = V + 7                                # one face with an index outside [0, V)
    return v, f


def weld_chain(F, ws):
    L = lib()
    V = 3 * F
    v, f = weld_inputs(F)
    n = L.ts2d_weld_workspace_bytes(V, F)
    ws = buf(n, U8) if ws is None else ws
    res = {}
    label = buf(V, I32)
    ok(L.ts2d_weld_labels(V, ptr(v), 0.0, ptr(label), ptr(ws), n, stream()))
    res["label"] = label
    for mode in (0, 1):
        remap, outv, count = buf(V, I32), buf((V, 3), F32), buf(1, I32)
        ok(L.ts2d_weld_compact(V, ptr(label), ptr(v), mode, ptr(remap), ptr(outv), ptr(count), ptr(ws), n, stream()))
        res[f"remap{mode}"], res[f"outv{mode}"], res[f"count{mode}"] = remap, outv, count
    faces, keep, counts, comp = buf((F, 3), I32), buf(F, U8), buf(4, I64), buf(V, I32)
    ok(L.ts2d_weld_remap_faces(V, F, ptr(f), ptr(remap), ptr(faces), ptr(keep), stream()))
    ok(L.ts2d_weld_edge_census(V, F, ptr(faces), ptr(keep), ptr(counts), ptr(ws), n, stream()))
    ok(L.ts2d_weld_face_components(V, F, ptr(faces), ptr(keep), ptr(comp), ptr(ws), n, stream()))
    res.update(faces=faces, keep=keep, counts=counts, comp=comp)
    return res


def test_weld_chain():
    sizes = [1, 341, 342, 2000]  # V = 3 F straddles the 1024-point box at 341 / 342
    base = check_family(weld_chain, lambda F: lib().ts2d_weld_workspace_bytes(3 * F, F), sizes, 2000, 1)
    for F, b in base.items():
        V = 3 * F
        count = int(b["count0"].view(I32)[0])
        assert count == int(b["count1"].view(I32)[0]) and 0 < count <= V - (2 if F > 1 else 1)
        for mode in (0, 1):  # "the rest 0": every byte of the rows V' .. V - 1
            assert not b[f"outv{mode}"][12 * count:].any(), (F, mode)
        assert b["keep"].view(U8)[F - 1] == 0 and b["faces"].view(I32)[3 * (F - 1):].tolist() == [-1, -1, -1]


# ---- model update --------------------------------------------------------------------------------------------------------------------------
def select_rows(P, ws):
    L = lib()
    g = torch.Generator().manual_seed(17 + P)
    mask = (torch.rand(P, generator=g) < 0.4).to(U8).to(DEV)
    n = L.tsm_select_scratch_bytes(P)
    ws = buf(n, U8) if ws is None else ws
    pos, count = buf(P, I32), C.c_uint32(0xFFFFFFFF)
    ok(L.tsm_select_rows(P, ptr(mask), 1, ptr(pos), ptr(ws), n, C.byref(count), stream()))
    assert count.value == int(mask.sum())
    return dict(pos=pos, count=count.value)


def test_select_rows():
    # 1024 rows per block; at 300 000 rows the block that arrives last walks 293 block sums in two rounds of 256
    check_family(select_rows, lambda P: lib().tsm_select_scratch_bytes(P), [1, 1023, 1024, 1025, 300_000], 300_000, 1)


def test_scatter_gather_rows_leave_the_other_rows_alone():
    L = lib()
    P, words = 1025, 9
    g = torch.Generator().manual_seed(18)
    src = torch.randn(P, words, generator=g).to(DEV)
    mask = (torch.rand(P, generator=g) < 0.4).to(U8).to(DEV)
    with poison.PoisonedEmpty("zero"):
        n = L.tsm_select_scratch_bytes(P)
        pos, count = buf(P, I32), C.c_uint32(0)
        ok(L.tsm_select_rows(P, ptr(mask), 1, ptr(pos), ptr(buf(n, U8)), n, C.byref(count), stream()))
    k = count.value
    idx = torch.arange(P - 1, -1, -3, dtype=torch.int32, device=DEV)  # 342 rows
    for pattern in poison.ORDER:
        with poison.PoisonedEmpty(pattern) as pe:
            row0 = 5
            dst, dst2 = buf((k + 11, words), F32), buf((idx.numel() + 11, words), F32)
            ok(L.tsm_scatter_rows(P, 4 * words, ptr(pos), ptr(src), ptr(dst), row0, stream()))
            ok(L.tsm_gather_rows(idx.numel(), 4 * words, ptr(idx), ptr(src), ptr(dst2), row0, stream()))
            assert torch.equal(poison.raw(dst[row0:row0 + k]), poison.raw(src[mask.bool()]))
            assert torch.equal(poison.raw(dst2[row0:row0 + idx.numel()]), poison.raw(src[idx.long()]))
            for d, m in ((dst, k), (dst2, idx.numel())):  # the rows the call does not select keep the pattern bit for bit
                rest = torch.cat([d[:row0].reshape(-1), d[row0 + m:].reshape(-1)])
                assert torch.equal(poison.raw(rest), poison.pattern_bytes(pattern, rest.numel() * 4)), pattern
            pe.check_guards()


def test_elementwise_model_updates():
    """Outputs fully written; the rows a masked update does not select keep their bits (they are inputs: compared with a clone)."""
    L = lib()
    for P in (1, 255, 257):
        g = torch.Generator().manual_seed(19 + P)
        vertex, opacity = torch.randn(P, 3, 3, generator=g).to(DEV), torch.randn(P, generator=g).to(DEV)
        accum, denom = torch.rand(P, generator=g).to(DEV) * 4, torch.randint(0, 6, (P,), generator=g).float().to(DEV)
        radii = (torch.rand(P, generator=g) * 40).to(DEV)
        parents = torch.randint(0, P, (max(1, P // 2),), generator=g, dtype=torch.int32).to(DEV)
        clip_mask = (torch.rand(P, generator=g) < 0.5).to(U8).to(DEV)

        def run(pattern):
            res = {}
            code, a, d = buf(P, U8), accum.clone(), denom.clone()
            ok(L.tsm_grow_classify(P, ptr(vertex), ptr(a), ptr(d), 2.0, 0.5, 1.5, ptr(code), stream()))
            res.update(code=code, accum=a, denom=d)
            c1, c2 = buf((parents.numel(), 3, 3), F32), buf((parents.numel(), 3, 3), F32)
            ok(L.tsm_split_vertex(parents.numel(), ptr(parents), ptr(vertex), ptr(c1), ptr(c2), stream()))
            res.update(child1=c1, child2=c2)
            for mode, (a_, b_) in enumerate(((0.4, 0.0), (0.6, 0.0), (20.0, 1.5), (1.5, 0.0))):
                m = buf(P, U8)
                ok(L.tsm_update_mask(P, mode, ptr(opacity), ptr(vertex), ptr(radii), a_, b_, ptr(m), stream()))
                res[f"mask{mode}"] = m
            for mode, param in ((0, opacity), (1, vertex)):
                p, e1, e2 = param.clone(), torch.ones_like(param), torch.full_like(param, 2.0)
                ok(L.tsm_clip(P, mode, ptr(clip_mask), 0.25, ptr(p), ptr(e1), ptr(e2), stream()))
                keep = ~clip_mask.bool()
                assert torch.equal(poison.raw(p[keep]), poison.raw(param[keep])) and bool((e1[keep] == 1).all()) and bool((e2[keep] == 2).all())
                res[f"clip{mode}"], res[f"clip{mode}m1"], res[f"clip{mode}m2"] = p, e1, e2
            o, e1, e2 = opacity.clone(), buf(P, F32), buf(P, F32)
            ok(L.tsm_opacity_reset(P, 0.01, ptr(o), ptr(e1), ptr(e2), stream()))
            assert not poison.raw(e1).any() and not poison.raw(e2).any()
            res.update(reset=o)
            return res
        poison.assert_pure(run)


def test_max_vertex_distance_and_state_digest():
    L = lib()
    campos = torch.tensor([0.5, -1.0, 2.0], device=DEV)
    for n in (0, 1, 1000):
        v = rnd(20, n, 3)

        def run(pattern):
            out = buf(1, F32)
            ok(L.tsm_max_vertex_distance(n, ptr(v), ptr(campos), ptr(out), stream()))
            return out
        b = poison.assert_pure(run)["0"]
        if n == 0:
            assert b.tolist() == [0, 0, 0, 0]  # "0 for n_vertices == 0"
        else:
            assert abs(float(b.view(F32)[0]) - float((campos - v).norm(dim=1).max())) < 1e-5
    segs = [rnd(21, 5), torch.zeros(0, device=DEV), rnd(22, 4099), torch.zeros(0, device=DEV), rnd(23, 16384 + 3)]

    def digest(pattern):
        d = buf(len(segs), I64)
        bases = (C.c_void_p * len(segs))(*[ptr(s) for s in segs])
        words = (C.c_uint64 * len(segs))(*[s.numel() for s in segs])
        ok(L.tsm_state_digest(len(segs), bases, words, ptr(d), stream()))
        return d
    d = poison.assert_pure(digest)["0"].view(I64)
    assert d[1] == 0 and d[3] == 0 and d[0] != 0 and d[2] != 0 and d[4] != 0  # "an empty segment has digest 0"


# ---- optimizer: no workspace, so only "nothing else is touched" applies ---------------------------------------------------------------------
def test_optimizer_writes_only_its_slices():
    """Parameters, gradients and moments of odd lengths sit inside one poisoned arena at offsets 4 bytes off a 16-byte boundary; after the
    steps every word of the arena outside them still holds the pattern, and what the steps computed does not depend on the pattern."""
    from diff_triangle_rasterization_2D._abi import _RowSlice, _ShFactoredStep, _Slice
    L = lib()
    first = {}
    for pattern in poison.ORDER:
        for P in (37, 65):
            with poison.PoisonedEmpty(pattern) as pe:
                arena = buf(1 << 16, F32)
                used = torch.zeros(arena.numel(), dtype=torch.bool, device=DEV)
                cursor, seed = [1], [1000 * P]

                def take(n, scale=1.0, positive=False):
                    o = cursor[0]
                    cursor[0] = o + n + 9
                    cursor[0] += (1 - cursor[0]) % 4
                    seed[0] += 1
                    g = torch.Generator().manual_seed(seed[0])
                    init = torch.randn(n, generator=g) * scale
                    v = arena[o:o + n]
                    v.copy_((init.abs() if positive else init).to(DEV))
                    used[o:o + n] = True
                    assert v.data_ptr() % 16 == 4
                    return v

                def group(n):  # parameter, gradient, first and second moment
                    return take(n), take(n, 0.1), take(n, 0.01), take(n, 1e-4, positive=True)

                M = 16
                vtx, opa, sh1, dc, rest = group(9 * P), group(P), group(3 * M * P), group(3 * P), group(3 * (M - 1) * P)
                campos, colour = torch.tensor([0.3, -0.2, 5.0], device=DEV), rnd(30 + P, P, 3, lo=-1.0, hi=1.0)
                slices = (_Slice * 3)(
                    _Slice(ptr(vtx[0]), ptr(vtx[1]), ptr(vtx[2]), ptr(vtx[3]), 9 * P, 1e-3, 0.5, 1.0, 0.0, 0, 0, 0),
                    _Slice(ptr(opa[0]), ptr(opa[1]), ptr(opa[2]), ptr(opa[3]), P, 2e-3, 0.5, 0.5, 0.0, 0, 0, 0),
                    _Slice(ptr(sh1[0]), ptr(sh1[1]), ptr(sh1[2]), ptr(sh1[3]), 3 * M * P, 1e-3, 0.5, 1.0, 5e-5, 0, 3 * M, 3))
                ok(L.tso_adam_step(slices, 3, 0.9, 0.999, 1e-15, stream()))

                def factored(p_dc, m_dc, v_dc, p_rest, m_rest, v_rest, dc_stride, rest_stride):
                    st = _ShFactoredStep()
                    st.P, st.M, st.sh_degree, st.V = P, M, 2, 1
                    st.vertex, st.campos, st.dL_dcolor = ptr(vtx[0]), ptr(campos), ptr(colour)
                    st.param_dc, st.exp_avg_dc, st.exp_avg_sq_dc = p_dc, m_dc, v_dc
                    st.param_rest, st.exp_avg_rest, st.exp_avg_sq_rest = p_rest, m_rest, v_rest
                    st.dc_stride, st.rest_stride = dc_stride, rest_stride
                    st.step_size_dc, st.bias2_sqrt_dc, st.step_size_rest, st.bias2_sqrt_rest, st.grad_scale = 1e-3, 0.5, 5e-5, 0.5, 1.0
                    st.num_rows = 2
                    st.rows[0] = _RowSlice(ptr(vtx[0]), ptr(vtx[1]), ptr(vtx[2]), ptr(vtx[3]), 9, 1e-3, 0.5, 1.0)
                    st.rows[1] = _RowSlice(ptr(opa[0]), ptr(opa[1]), ptr(opa[2]), ptr(opa[3]), 1, 2e-3, 0.5, 1.0)
                    ok(L.tso_adam_step_sh_factored(C.byref(st), 0.9, 0.999, 1e-15, stream()))
                # ONE (P, 16, 3) tensor: dc = base, rest = base + 3 floats, both strides 3 M (the 64-triangles-per-workgroup path) ...
                factored(ptr(sh1[0]), ptr(sh1[2]), ptr(sh1[3]), ptr(sh1[0]) + 12, ptr(sh1[2]) + 12, ptr(sh1[3]) + 12, 3 * M, 3 * M)
                # ... and the reference's two tensors f_dc (P, 1, 3) / f_rest (P, 15, 3)
                factored(ptr(dc[0]), ptr(dc[2]), ptr(dc[3]), ptr(rest[0]), ptr(rest[2]), ptr(rest[3]), 3, 3 * (M - 1))
                outside = arena[~used]
                assert torch.equal(poison.raw(outside), poison.pattern_bytes(pattern, 4 * outside.numel())), (pattern, P)
                inside = poison.raw(arena[used])
                assert torch.equal(first.setdefault(P, inside), inside), (pattern, P)
                pe.check_guards()


# ---- opaque mesh renderer ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def mesh_inputs(F, W, H):
    import synthetic
    s = synthetic.scene(F, W, H, 0, seed=31 + F, edge_px=8.0, with_grads=False)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    faces = torch.arange(3 * F, dtype=torch.int32).reshape(F, 3).clone()
    if F > 1:
        faces[F // 2, 1] = 3 * F + 5  # an index outside [0, V): the face is not drawn
    return dict(view=dev(s["viewmatrix"]), tanx=s["tanfovx"], tany=s["tanfovy"], vertices=dev(s["vertex"].reshape(-1, 3)), faces=faces.to(DEV),
                colour=rnd(32, F, 3, lo=-0.1, hi=1.1), background=torch.tensor([0.1, 0.2, 0.3], device=DEV), target=rnd(33, 3, H, W))


def mesh_render(case, ws):
    from diff_triangle_rasterization_2D._abi import _Camera, _State
    F, W, H = case
    L = lib()
    m = mesh_inputs(F, W, H)
    cam = _Camera(W, H, m["tanx"], m["tany"], ptr(m["view"]), None, None)
    ng, ni = L.ts2d_mesh_geometry_state_bytes(F), L.ts2d_image_state_bytes(W, H)
    geo, img = (buf(ng, U8), buf(ni, U8)) if ws is None else ws[:2]
    st = _State(ptr(geo), geo.numel(), None, 0, ptr(img), img.numel())
    n = C.c_int64(-1)
    ok(L.ts2d_mesh_bin(C.byref(cam), 0.01, 3 * F, ptr(m["vertices"]), F, ptr(m["faces"]), C.byref(st), C.byref(n), stream()))
    N = n.value
    if N > 0:
        binning = buf(L.ts2d_binning_state_bytes(N, W, H), U8) if ws is None else ws[2]
        st.binning, st.binning_bytes = ptr(binning), binning.numel()
    res = dict(N=N)
    for counted in (False, True):
        render, mask, depth, face = buf((3, H, W), F32), buf((H, W), F32), buf((H, W), F32), buf((H, W), I32)
        if counted:
            visits = torch.zeros(1, dtype=I64, device=DEV)  # caller-cleared
            ok(L.ts2d_mesh_render_counted(C.byref(cam), F, ptr(m["colour"]), ptr(m["background"]), N, C.byref(st), ptr(render), ptr(mask), ptr(depth),
                                          ptr(face), ptr(visits), stream()))
            res["visits"] = visits
        else:
            ok(L.ts2d_mesh_render(C.byref(cam), F, ptr(m["colour"]), ptr(m["background"]), N, C.byref(st), ptr(render), ptr(mask), ptr(depth), ptr(face),
                                  stream()))
        k = "c" if counted else ""
        res.update({"render" + k: render, "mask" + k: mask, "depth" + k: depth, "face" + k: face})
    census = torch.zeros((F, 4), dtype=I64, device=DEV)  # caller-cleared: an input
    ok(L.ts2d_mesh_census_add(W, H, F, ptr(res["face"]), ptr(m["target"]), None, ptr(census), stream()))
    res["census"] = census
    return res


def test_mesh_renderer():
    L = lib()
    cases = [(F, W, H) for F in (1, 500, 12_289) for (W, H) in ((129, 5), (160, 120))]
    base = {c: poison.assert_pure(lambda pattern, c=c: mesh_render(c, None)) for c in cases}
    for c, b in base.items():
        for k in ("render", "mask", "depth", "face"):
            assert torch.equal(b[k], b[k + "c"]), (c, k)
    assert any(b["N"] > 0 for b in base.values())
    large, small = (12_289, 160, 120), (1, 129, 5)
    with poison.PoisonedEmpty("nan") as pe:  # one set of state buffers: large -> small -> large
        ws = (buf(L.ts2d_mesh_geometry_state_bytes(large[0]), U8), buf(L.ts2d_image_state_bytes(large[1], large[2]), U8),
              buf(L.ts2d_binning_state_bytes(max(1, base[large]["N"], base[small]["N"]), large[1], large[2]), U8))
        for c in (large, small, large):
            diff = poison._first_difference(base[c], poison._snapshot(mesh_render(c, ws), None))
            assert diff is None, f"state buffers reused for {c} after another mesh: {diff}"
            pe.check_guards()


# ---- rasterizer, 2D and 3D, through the module ---------------------------------------------------------------------------------------------
# Float atomics: the forward adds a triangle's per-tile contribution sums to contrib_sum with float atomic adds (ts2d_group.h,
# global_stats_add), and the backward blend kernels add every pixel group's partial gradients to the 64-byte gradient records with float
# atomic adds, from which the per-triangle kernel forms dL_dvertex, dL_dcenter2D, dL_dshs / dL_dfeature and dL_dopacity.  The order of
# those adds changes from run to run, so these outputs cannot be bit-stable; they are held to the bars of tests/test_parity_gpu.py against
# the CPU oracle, must be finite, and exactly zero in every row with radii == 0.  contrib_max is a maximum (integer atomicMax on the bit
# pattern): order-independent, compared bit for bit with everything else.
ATOMIC = ("contrib_sum", "dL_dvertex", "dL_dcenter2D", "dL_dshs", "dL_dfeature", "dL_dopacity")
_hint_key = [0x70757269]


class RasterCase:
    def __init__(self, s, variant, rich, back, use_feature):
        import helpers
        self.s, self.variant, self.rich, self.back, self.use_feature = s, variant, rich, back, use_feature
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.rs = helpers.hip_settings(s, rich, back, False, DEV)
        self.vertex, self.opacity = dev(s["vertex"]), dev(s["opacity"])
        self.colour = dev(s["feature"] if use_feature else s["shs"])
        self.P, self.W, self.H = self.vertex.shape[0], s["image_width"], s["image_height"]
        self.C = self.colour.shape[1] if use_feature else 3
        self.c2d = torch.zeros((self.P, 2), device=DEV)
        self.grads = [dev(s["dL_dout_feature"])] + ([dev(s["dL_dout_depth"]), dev(s["dL_dout_normal"])] if rich else [])
        self.N = None

    def forward_sizes(self, binning_instances):
        """What the extension's forward allocates, in its order (bindings/ts2d_torch_ext.cpp): the outputs, then the three state buffers."""
        L, P, W, H = lib(), self.P, self.W, self.H
        sizes = [4 * self.C * H * W, 4 * P] + ([4 * H * W, 12 * H * W, 4 * P, 4 * P] if self.rich else [])
        sizes += [L.ts2d_geometry_state_bytes(P), L.ts2d_image_state_bytes(W, H)]
        sizes.append(L.ts2d_binning_state_bytes(binning_instances, W, H))  # (allocated for num_rendered == 0 as well: an empty state)
        return sizes

    def backward_sizes(self):
        P = self.P
        M = 0 if self.use_feature else self.colour.shape[1]
        return [36 * P, 8 * P, 4 * P] + ([12 * P * M] if M else []) + [4 * P * self.C, lib().ts2d_backward_scratch_bytes(P)]

    def run(self, pattern, capacity=None):
        """One forward + backward through the autograd module with every block it allocates poisoned beforehand; asserts that the three state
        buffers the step used ARE poisoned blocks."""
        import helpers
        from diff_triangle_rasterization_2D import _C as native
        import diff_triangle_rasterization_2D as pkg2
        import diff_triangle_rasterization_3D as pkg3
        pkg = pkg3 if self.variant == 3 else pkg2
        _hint_key[0] += 1
        native.set_capacity_hint_key(_hint_key[0])  # no history: the binning buffer is sized from num_rendered, as the test sizes its block
        vertex, opacity, colour = (t.detach().requires_grad_(True) for t in (self.vertex, self.opacity, self.colour))
        c2d = self.c2d.detach().requires_grad_(True)
        kw = dict(feature=colour) if self.use_feature else dict(shs=colour)
        torch.cuda.synchronize()
        held = None
        if pattern is not None:
            held = poison.poison_blocks(self.forward_sizes(self.N if capacity is None else capacity), pattern)
        try:
            out = pkg.TriangleRasterizer(self.rs)(vertex, c2d, opacity, **kw)
        finally:
            native.set_capacity_hint_key(0)  # the calling thread's default again
        node = out[0].grad_fn
        saved = node.saved_tensors
        if held is not None:
            held.assert_used(saved[5:8])
        res = dict(num_rendered=node.num_rendered, buffers=saved[5:8], out_feature=out[0].detach(), radii=out[1])
        if self.rich:
            res.update(depth=out[2].detach(), normal=out[3].detach(), contrib_sum=out[4], contrib_max=out[5])
        if capacity is not None:
            return res
        if pattern is not None:
            poison.poison_blocks(self.backward_sizes(), pattern)
        torch.autograd.backward([out[0], out[2], out[3]] if self.rich else [out[0]], self.grads)
        res.update(dL_dvertex=vertex.grad, dL_dcenter2D=c2d.grad, dL_dopacity=opacity.grad)
        res["dL_dfeature" if self.use_feature else "dL_dshs"] = colour.grad
        fields = ["ranges", "point_offsets", "n_contrib"] + (["keys", "vals"] if node.num_rendered > 0 else [])
        for name in fields:
            res["state_" + name] = torch.from_numpy(np.ascontiguousarray(helpers.hip_state(res, self.s, name)))
        del res["buffers"]
        return res


def raster_pure(case, oracle):
    """The harness of poison.assert_pure for the module: a probe for num_rendered, two runs on zero-filled blocks (determinism), then the
    patterns in order.  `oracle`: dict of the float-atomic outputs' reference values, or None = the zero-filled run (P = 600 000)."""
    import helpers
    import test_parity_gpu as T2
    case.N = case.run(None)["num_rendered"]

    def split(res):
        exact = {k: (poison.raw(v) if isinstance(v, torch.Tensor) else v) for k, v in res.items() if k not in ATOMIC}
        soft = {k: v.detach().cpu().numpy() for k, v in res.items() if k in ATOMIC}
        return exact, soft

    def check_soft(soft, radii, ref, what):
        culled = radii == 0
        for k, v in soft.items():
            assert np.isfinite(v).all(), (what, k)
            assert not v[culled].any(), (what, k, "a row with radii == 0 is not exactly zero")
            tol = T2.IMG_TOL if k == "contrib_sum" else T2.GRAD_TOL
            err = helpers.rel_l2(v.reshape(ref[k].shape), ref[k])
            print(f"purity {what} {k}: rel L2 {err:.3e} (bar {tol:g})")
            assert err < tol, (what, k, err)

    base, base_soft = split(case.run("zero"))
    radii = base["radii"].view(I32).numpy()
    diff = poison._first_difference(base, split(case.run("zero"))[0])
    if diff:
        raise poison.DeterminismError(f"two runs on zero-filled blocks disagree -- {diff}")
    ref = base_soft if oracle is None else oracle
    check_soft(base_soft, radii, ref, "zero")
    for pattern in poison.ORDER:
        exact, soft = split(case.run(pattern))
        diff = poison._first_difference(base, exact)
        if diff:
            raise poison.PoisonLeak(f"pattern {pattern} changes the result -- {diff}")
        check_soft(soft, radii, ref, pattern)
    return base, base_soft


def oracle_of(case):
    import helpers
    s = case.s
    of = helpers.oracle_forward(s, case.rich, case.back, use_feature=case.use_feature, variant=case.variant)
    ob = helpers.oracle_backward(s, of, case.rich, use_feature=case.use_feature)
    ref = {k: ob[k] for k in ATOMIC if k in ob and ob[k] is not None}
    if case.rich:
        ref["contrib_sum"] = of["contrib_sum"]
    return of, ref


# Six cases of the fuzz sweep: for each of (2D | 3D) x (rich_info with SH, no rich_info with SH, feature mode with rich_info) the seed below
# 40 with the most triangles, the lowest such seed among equals -- chosen from the configurations alone.
FUZZ_SEEDS = [24, 4, 12, 9, 31, 1]


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_rasterizer_fuzz_case(seed):
    import test_fuzz_gpu
    case = RasterCase(*test_fuzz_gpu._case(seed))
    of, ref = oracle_of(case)
    base, _ = raster_pure(case, ref)
    assert base["num_rendered"] == of["num_rendered"] > 0
    assert np.array_equal(base["radii"].view(I32).numpy(), of["radii"].reshape(-1))


def test_fuzz_seeds_cover_the_modes():
    import test_fuzz_gpu
    modes = {(v, rich, feat) for _, v, rich, _, feat in (test_fuzz_gpu._case(seed) for seed in FUZZ_SEEDS)}
    assert modes == {(2, True, False), (2, False, False), (2, True, True), (3, True, False), (3, False, False), (3, True, True)}


def test_rasterizer_sampled_splitter_depth_order():
    """P = 10 000: above the one-launch depth order (9 216), the sampled-splitter form with its scratch inside `offsets` and `sv[1]`."""
    import synthetic
    case = RasterCase(synthetic.scene(10_000, 64, 64, 3, seed=41, edge_px=2.0), 2, True, False, False)
    of, ref = oracle_of(case)
    base, _ = raster_pure(case, ref)
    assert base["num_rendered"] == of["num_rendered"] > 0


def test_rasterizer_lsd_depth_order():
    """P = 600 000: above the sampled-splitter form (500 000), the ticket-free LSD passes and the tile sort's.  Compared with its own run on
    zero-filled blocks only, not the oracle."""
    import synthetic
    case = RasterCase(synthetic.scene(600_000, 64, 64, 0, seed=42, edge_px=1.5), 2, True, False, False)
    base, _ = raster_pure(case, None)
    assert base["num_rendered"] > 0


def culled_scene():
    import synthetic
    s = synthetic.scene(300, 64, 48, 1, seed=43)
    s["vertex"] = s["vertex"].copy()
    s["vertex"][:, :, 0] += 1.0e5  # far outside the frustum: every triangle is culled, num_rendered == 0 and nobody but emission clears the ranges
    return s


@pytest.mark.parametrize("variant", [2, 3])
def test_rasterizer_every_triangle_culled(variant):
    case = RasterCase(culled_scene(), variant, True, False, False)
    base, soft = raster_pure(case, None)
    assert base["num_rendered"] == 0 and not base["radii"].any()
    for k, v in soft.items():
        assert not v.any(), k
    bg = np.broadcast_to(case.s["background"][:, None, None], (3, case.H, case.W))
    assert np.array_equal(base["out_feature"].view(F32).numpy().reshape(3, case.H, case.W), bg)


def test_sync_free_forward_below_its_capacity():
    """ts2d_forward with a capacity below the true count: nothing is emitted, the image is the background and every statistic zero, whatever
    the state buffers held."""
    import diff_triangle_rasterization_2D as pkg
    import synthetic
    s = synthetic.scene(300, 64, 48, 1, seed=44)
    s["background"] = np.array([0.25, 0.5, 0.75], np.float32)
    case = RasterCase(s, 2, True, False, False)
    N = case.run(None)["num_rendered"]
    cap = N // 2
    assert cap >= 1
    pkg.set_instance_capacity(cap)
    try:
        runs = {}
        for pattern in ("zero",) + poison.ORDER:
            res = case.run(pattern, capacity=cap)
            out = res["out_feature"]
            over, true_count = pkg.forward_overflowed(None)
            assert bool(over) and int(true_count) == N, (pattern, over, true_count)
            del res["buffers"]
            runs[pattern] = {k: (poison.raw(v) if isinstance(v, torch.Tensor) else v) for k, v in res.items()}
            assert res["num_rendered"] == cap
            assert torch.equal(out.cpu(), torch.tensor([0.25, 0.5, 0.75])[:, None, None].expand(3, case.H, case.W)), pattern
            assert not res["contrib_sum"].any() and not res["contrib_max"].any(), pattern
            diff = poison._first_difference(runs["zero"], runs[pattern])
            assert diff is None, (pattern, diff)
    finally:
        pkg.set_instance_capacity(None)


@pytest.mark.parametrize("D,M", [(1, 16), (3, 16), (0, 1)])
def test_sh_grad_expand(D, M):
    L = lib()
    for P in (1, 257):
        for V in (1, 3):
            vertex, campos, colour = rnd(50 + P, P, 9, lo=-2.0, hi=2.0), rnd(51 + V, V, 3, lo=3.0, hi=5.0), rnd(52 + P * V, V, P, 3, lo=-1.0, hi=1.0)

            def run(pattern):
                out = buf((P, M, 3), F32)
                ok(L.ts2d_sh_grad_expand(P, D, M, V, ptr(vertex), ptr(campos), ptr(colour), ptr(out), stream()))
                return out
            b = poison.assert_pure(run)["0"].view(F32).reshape(P, M, 3)
            assert not poison.raw(b[:, (D + 1) ** 2:]).any()  # the tail coefficients: exactly +0.0
            assert b[:, :(D + 1) ** 2].abs().sum() > 0


@pytest.mark.parametrize("variant_flag", [0x0, 0x10])
def test_forward_without_triangles(variant_flag):
    """P == 0 through the C ABI (the Python module returns zeros without calling the library): "every element of every non-NULL output is
    written" -- the background, whatever the image state and the outputs held."""
    from diff_triangle_rasterization_2D._abi import _Camera, _ForwardOut, _Geometry, _State
    import synthetic
    L = lib()
    W, H = 33, 20
    c = synthetic.camera(W, H)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    view, proj, campos, bg = dev(c["viewmatrix"]), dev(c["projmatrix"]), dev(c["campos"]), torch.tensor([0.25, 0.5, 0.75], device=DEV)
    cam = _Camera(W, H, c["tanfovx"], c["tanfovy"], ptr(view), ptr(proj), ptr(campos))
    geom = _Geometry(0, 0, 1, 3, 1.0, 1.0, 7.0, ptr(bg), None, None, None, None, None)

    def run(pattern):
        n = L.ts2d_image_state_bytes(W, H)
        image, out, depth, normal = buf(n, U8), buf((3, H, W), F32), buf((H, W), F32), buf((3, H, W), F32)
        st = _State(None, 0, None, 0, ptr(image), n)
        fo = _ForwardOut(ptr(out), ptr(depth), ptr(normal), None, None)
        ok(L.ts2d_forward_render(C.byref(cam), C.byref(geom), 0x2 | 0x8 | variant_flag, 0, C.byref(st), C.byref(fo), stream()))  # RICH_INFO | USE_SHS
        return dict(out=out, depth=depth, normal=normal)
    b = poison.assert_pure(run)
    assert torch.equal(b["out"].view(F32).reshape(3, H, W), bg.cpu()[:, None, None].expand(3, H, W))


# ---- the rasterizer through the C ABI: guard bands around the state buffers, and ONE set of them for large -> small -> large ----------------
@functools.lru_cache(None)
def cabi_scene(P, W, H):
    import synthetic
    s = synthetic.scene(P, W, H, 2, seed=60 + P, edge_px=6.0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return s, {k: dev(s[k]) for k in ("viewmatrix", "projmatrix", "campos", "background", "vertex", "shs", "opacity", "dL_dout_feature",
                                      "dL_dout_depth", "dL_dout_normal")}


def raster_cabi(size, ws, soft_log):
    from diff_triangle_rasterization_2D._abi import _BackwardOut, _Camera, _ForwardOut, _Geometry, _LossGrads, _State
    P, W, H = size
    L = lib()
    s, d = cabi_scene(P, W, H)
    M, flags = d["shs"].shape[1], 0x2 | 0x8  # RICH_INFO | USE_SHS
    cam = _Camera(W, H, s["tanfovx"], s["tanfovy"], ptr(d["viewmatrix"]), ptr(d["projmatrix"]), ptr(d["campos"]))
    geom = _Geometry(P, s["sh_degree"], M, 3, s["gamma"], 1.0, s["background_depth"], ptr(d["background"]), ptr(d["vertex"]), ptr(d["shs"]), None,
                     ptr(d["opacity"]), None)
    geo = buf(L.ts2d_geometry_state_bytes(P), U8) if ws is None else ws[0]
    img = buf(L.ts2d_image_state_bytes(W, H), U8) if ws is None else ws[1]
    st = _State(ptr(geo), geo.numel(), None, 0, ptr(img), img.numel())
    radii, n = buf(P, I32), C.c_int64(-1)
    ok(L.ts2d_forward_bin(C.byref(cam), C.byref(geom), flags, ptr(radii), C.byref(st), C.byref(n), stream()))
    N = n.value
    if N > 0:
        binning = buf(L.ts2d_binning_state_bytes(N, W, H), U8) if ws is None else ws[2]
        st.binning, st.binning_bytes = ptr(binning), binning.numel()
    out, depth, normal, csum, cmax = buf((3, H, W), F32), buf((H, W), F32), buf((3, H, W), F32), buf(P, F32), buf(P, F32)
    fo = _ForwardOut(ptr(out), ptr(depth), ptr(normal), ptr(csum), ptr(cmax))
    ok(L.ts2d_forward_render(C.byref(cam), C.byref(geom), flags, N, C.byref(st), C.byref(fo), stream()))
    scratch = buf(L.ts2d_backward_scratch_bytes(P), U8) if ws is None else ws[3]
    dv, dc, dsh, dft, dop = buf((P, 3, 3), F32), buf((P, 2), F32), buf((P, M, 3), F32), buf((P, 3), F32), buf(P, F32)
    loss = _LossGrads(ptr(d["dL_dout_feature"]), ptr(d["dL_dout_depth"]), ptr(d["dL_dout_normal"]))
    bo = _BackwardOut(ptr(dv), ptr(dc), ptr(dsh), ptr(dft), ptr(dop))
    ok(L.ts2d_backward(C.byref(cam), C.byref(geom), flags, N, ptr(radii), C.byref(st), C.byref(loss), ptr(scratch), scratch.numel(), C.byref(bo),
                       stream()))
    soft_log.append(dict(radii=radii.cpu().numpy(), contrib_sum=csum.cpu().numpy(), dL_dvertex=dv.cpu().numpy(), dL_dcenter2D=dc.cpu().numpy(),
                         dL_dshs=dsh.cpu().numpy(), dL_dfeature=dft.cpu().numpy(), dL_dopacity=dop.cpu().numpy()))
    return dict(N=N, radii=radii, out=out, depth=depth, normal=normal, contrib_max=cmax)


def test_rasterizer_state_buffers_through_the_c_abi():
    """The two-call forward and the backward on state buffers, scratch and outputs that the test owns: guard bands show that the *_bytes queries
    are honest, and ONE set of buffers serves a large scene, a tiny one and the large one again (a view change, a densification) without being
    poisoned again.  The float-atomic outputs (see above) are held to the parity bars against the run on fresh zero-filled buffers."""
    import helpers
    import test_parity_gpu as T2
    L = lib()
    sizes = [(4000, 128, 96), (3, 33, 31), (65, 100, 16)]
    large, small = sizes[0], sizes[1]

    def check_soft(log, what):
        ref = log[0]
        for i, run in enumerate(log):
            culled = run["radii"] == 0
            for k, v in run.items():
                if k == "radii":
                    continue
                assert np.isfinite(v).all() and not v[culled].any(), (what, i, k)
                assert helpers.rel_l2(v, ref[k]) < (T2.IMG_TOL if k == "contrib_sum" else T2.GRAD_TOL), (what, i, k)

    base, logs = {}, {}
    for size in sizes:
        logs[size] = []
        base[size] = poison.assert_pure(lambda pattern, size=size: raster_cabi(size, None, logs[size]))
        assert base[size]["N"] > 0
        check_soft(logs[size], size)
    with poison.PoisonedEmpty("nan") as pe:
        ws = (buf(L.ts2d_geometry_state_bytes(large[0]), U8), buf(L.ts2d_image_state_bytes(large[1], large[2]), U8),
              buf(L.ts2d_binning_state_bytes(max(b["N"] for b in base.values()), large[1], large[2]), U8),
              buf(L.ts2d_backward_scratch_bytes(large[0]), U8))
        for size in (large, small, large):
            log = [logs[size][0]]
            diff = poison._first_difference(base[size], poison._snapshot(raster_cabi(size, ws, log), None))
            assert diff is None, f"state buffers reused for {size} after another scene: {diff}"
            check_soft(log, ("reused", size))
            pe.check_guards()
