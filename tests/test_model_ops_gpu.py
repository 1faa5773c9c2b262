"""GPU tests of the model-update operators (csrc/model_update.hip, include/ts_model.h, diff_recon_hip/model_update.py) against plain
references at training sizes.  tests/test_model_update_gpu.py pins the rules against the reference's own methods on a 300-row fixture,
which is one compaction block (1024 rows); here every operator is compared with torch at the sizes and inputs where these kernels can go
wrong: the block-to-block hand-off of the compaction plan (and the carry of its elected block above 256 blocks = 262 144 rows), row
moves of every width with NaN payloads and -0.0, the structural rules at 1 M triangles with their Adam moments, decisions placed on
and one float32 ulp either side of their thresholds, and the per-iteration statistics over several views.

References: row movement is torch's own indexing on the GPU, compared bit for bit through an int32 view; arithmetic is either torch's
float32 GPU expression of the documented rule (masks, clipping, reset) or a float64 evaluation (statistics).  Every plan returned by
select_rows is checked against torch.cumsum BEFORE it is used to write rows."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MB = 1024  # rows per compaction block (model_update.hip)
PARAMS = ("vertex", "opacity", "f_dc", "f_rest")
STATS = ("gradient_accum", "gradient_denom", "max_radii2D", "contrib_sum", "contrib_max", "contrib_denom")


def _bits(t):
    import torch
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype in (torch.float32, torch.int32) else t


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _ulp_up(x: float) -> float:
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def _ulp_down(x: float) -> float:
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


def _check_plan(mask, match, pos, count, what=""):
    """pos / count of select_rows against torch: count = number of rows equal to `match`, pos = exclusive running count on them, -1
    elsewhere.  Runs before any plan is used to write, so a wrong plan fails here instead of writing out of bounds."""
    import torch
    sel = mask.view(torch.uint8) == match if mask.dtype == torch.bool else mask == match
    want_count = int(sel.sum())
    assert count == want_count, (what, count, want_count)
    run = torch.cumsum(sel.to(torch.int64), 0) - 1
    want = torch.where(sel, run, torch.full_like(run, -1)).to(torch.int32)
    assert pos.dtype == torch.int32 and pos.shape == sel.shape
    if not torch.equal(pos, want):
        bad = (pos != want).nonzero().flatten()
        first = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} wrong positions, first at row {first} (block {first // MB}): "
                             f"got {int(pos[first])}, want {int(want[first])}")


# ---- 1. select_rows: the stable compaction plan -------------------------------------------------------------------------------------------
SIZES = [1, 3, 1023, 1024, 1025, 4097, 262_143, 262_144, 262_145, 263_169, 1_000_003, 5_000_000]
MASKS = ["none", "all", "half", "sparse", "dense", "first", "last", "block_ends", "alternate_blocks"]


def _mask(kind, n, seed):
    import torch
    i = torch.arange(n, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "none":
        return torch.zeros(n, device="cuda", dtype=torch.bool)
    if kind == "all":
        return torch.ones(n, device="cuda", dtype=torch.bool)
    if kind in ("half", "sparse", "dense"):
        p = {"half": 0.5, "sparse": 1e-4, "dense": 1 - 1e-4}[kind]
        return torch.rand(n, device="cuda", generator=g) < p
    if kind == "first":
        return i == 0
    if kind == "last":
        return i == n - 1
    if kind == "block_ends":  # the last row of every block, the partial last block included
        return (i % MB == MB - 1) | (i == n - 1)
    if kind == "alternate_blocks":
        return (i // MB) % 2 == 0
    raise ValueError(kind)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("n", SIZES)
def test_select_rows_plan_of_a_mask_equals_the_running_count(n, kind):
    """Above 256 blocks the elected block walks the block sums in several chunks of 256 and carries the running total from one to the next."""
    from diff_recon_hip.model_update import select_rows
    mask = _mask(kind, n, seed=n)
    pos, count = select_rows(mask)
    _check_plan(mask, 1, pos, count, f"{kind} n={n}")


@pytest.mark.parametrize("n", [1, 1025, 262_145, 1_000_003, 5_000_000])
def test_select_rows_plan_of_a_code_array_equals_the_running_count(n):
    """densification selects on its uint8 grow codes with select_rows(code, 1) and (code, 2); 3 never occurs."""
    import torch
    from diff_recon_hip.model_update import select_rows
    g = torch.Generator(device="cuda").manual_seed(7 + n)
    code = torch.randint(0, 3, (n,), device="cuda", generator=g, dtype=torch.uint8)
    code[(torch.rand(n, device="cuda", generator=g) < 0.9)] = 0  # mostly untouched rows, like a densification step
    for match in (0, 1, 2, 3):
        pos, count = select_rows(code, match)
        _check_plan(code, match, pos, count, f"code n={n} match={match}")
    pos, count = select_rows(code != 2)  # the kept rows of densification
    _check_plan(code != 2, 1, pos, count, f"code != 2 n={n}")


def test_select_rows_handoffs_under_uneven_load():
    """mask_count_kernel's hand-off (write-through store of the block count, drained, a ticket; the last-arriving block loads the counts
    and prefixes them) repeated while a second stream keeps some CUs busy with copies and matrix products, so that producers and the
    elected block meet on busy and idle CUs.  A fixed number of plans, each compared with torch.cumsum of its mask."""
    import torch
    from diff_recon_hip.model_update import select_rows
    side = torch.cuda.Stream()
    big = torch.empty((64 << 20,), device="cuda", dtype=torch.float32).fill_(1.0)
    a = torch.randn((2048, 2048), device="cuda")
    sizes = [262_145, 1_000_003, 5_000_000, 263_169, 2_000_001, 4_100_001]
    kinds = ["half", "sparse", "alternate_blocks", "dense", "block_ends", "last"]
    failures = []
    for it in range(24):
        n = sizes[it % len(sizes)]
        kind = kinds[(it // 2) % len(kinds)]
        mask = _mask(kind, n, seed=100 + it)
        torch.cuda.current_stream().synchronize()  # the mask exists before the neighbour load starts
        with torch.cuda.stream(side):  # uneven neighbour load of varying length
            for _ in range(1 + it % 4):
                big[: (16 << 20) * (1 + it % 3)].mul_(1.0001)
                a = (a @ a).clamp_(-1, 1)
        pos, count = select_rows(mask)
        try:
            _check_plan(mask, 1, pos, count, f"plan {it}: {kind} n={n}")
        except AssertionError as e:
            failures.append(str(e))
    torch.cuda.synchronize()
    assert not failures, failures


# ---- 2. scatter_rows / gather_rows ------------------------------------------------------------------------------------------------------
WIDTHS = [1, 3, 9, 24, 45, 48]  # opacity / statistics, f_dc, vertex or f_rest at SH 1, f_rest at SH 2 and 3, the single shs tensor
SENTINEL = 0x5A5A5A5A


def _rows(n, w, dtype, seed):
    """(n, w) rows of `dtype` whose words include NaNs with payloads (quiet and signalling, both signs), -0.0, +-inf and denormals."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    if dtype == torch.int32:
        return torch.randint(-2 ** 31, 2 ** 31 - 1, (n, w), device="cuda", generator=g, dtype=torch.int32)
    x = torch.randn((n, w), device="cuda", generator=g)
    b = x.view(torch.int32)
    specials = torch.tensor([0x7FC00123, -0x003FFFFF, 0x7F800001, -0x80000000, 0x7F800000, -0x00800000, 0x00000001], device="cuda",
                            dtype=torch.int32)  # qNaN+payload, -qNaN, sNaN, -0.0, +inf, -inf, smallest denormal
    at = torch.randint(0, n * w, (min(n * w, 4096),), device="cuda", generator=g)
    b.view(-1)[at] = specials[torch.arange(at.numel(), device="cuda") % specials.numel()]
    return x


@pytest.mark.parametrize("dtype", ["float32", "int32"])
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("n", [262_145, 1_000_003])
def test_scatter_and_gather_rows_move_rows_bit_for_bit(n, w, dtype):
    """scatter_rows == src[mask] into rows dst_row0.. of a sentinel-filled output; gather_rows == src[idx] with indices that repeat,
    descend and include the last row; rows outside the written range keep the sentinel."""
    import torch
    from diff_recon_hip.model_update import gather_rows, scatter_rows, select_rows
    dt = getattr(torch, dtype)
    src = _rows(n, w, dt, seed=n * 64 + w)
    g = torch.Generator(device="cuda").manual_seed(w)
    mask = torch.rand(n, device="cuda", generator=g) < 0.37
    mask[-1] = True
    pos, count = select_rows(mask)
    _check_plan(mask, 1, pos, count, "scatter plan")
    want = src.view(torch.int32)[mask]
    for row0 in (0, 5):
        out = torch.full((row0 + count + 3, w), SENTINEL, device="cuda", dtype=torch.int32).view(dt)
        scatter_rows(src, pos, out, row0)
        ob = out.view(torch.int32)
        assert torch.equal(ob[row0:row0 + count], want), ("scatter", row0)
        assert (ob[:row0] == SENTINEL).all() and (ob[row0 + count:] == SENTINEL).all(), ("scatter outside", row0)
    k = 50_000
    idx = torch.cat((torch.randint(0, n, (k,), device="cuda", generator=g),      # random, with repeats
                     torch.arange(n - 1, n - 1 - k, -1, device="cuda"),           # descending from the last row
                     torch.tensor([n - 1, n - 1, 0, 0, n // 2], device="cuda"))).to(torch.int32)
    m = idx.numel()
    want = src.view(torch.int32).index_select(0, idx.long())
    for row0 in (0, 9, n):  # n: the clone rows of densification start after the kept rows
        out = torch.full((row0 + m + 2, w), SENTINEL, device="cuda", dtype=torch.int32).view(dt)
        gather_rows(src, idx, out, row0)
        ob = out.view(torch.int32)
        assert torch.equal(ob[row0:row0 + m], want), ("gather", row0)
        assert (ob[:row0] == SENTINEL).all() and (ob[row0 + m:] == SENTINEL).all(), ("gather outside", row0)


# ---- 3. the structural rules at 1 M triangles -----------------------------------------------------------------------------------------
def _mean_side(v):
    """get_scaling (VanillaTS_model.py:72-76) as torch evaluates it: mean of the side lengths |v2 - v1|, |v0 - v2|, |v1 - v0|."""
    import torch
    sides = torch.stack(((v[:, 2] - v[:, 1]).norm(dim=1), (v[:, 0] - v[:, 2]).norm(dim=1), (v[:, 1] - v[:, 0]).norm(dim=1)), dim=1)
    return sides, sides.mean(dim=1)


def _children(v):
    """_grow_points' split geometry (:270-283): cut the longest side (torch.argmax: first maximum) at its centre."""
    import torch
    sides, _ = _mean_side(v)
    l = torch.argmax(sides, dim=1)
    p1, p2 = (l + 1) % 3, (l + 2) % 3
    r = torch.arange(v.shape[0], device=v.device)
    c = (v[r, p1] + v[r, p2]) / 2
    return torch.stack((v[r, l], v[r, p1], c), dim=1), torch.stack((v[r, l], c, v[r, p2]), dim=1)


def _big_model(P, sh_degree, seed):
    """A model-like object with the reference's attribute names (as tests/test_model_update_gpu.py::_model builds it): the four
    parameters, Adam state with non-zero moments after one step, the six statistics, and the rule configuration."""
    import torch
    from types import SimpleNamespace as NS
    g = torch.Generator(device="cuda").manual_seed(seed)
    m = NS()
    centre = torch.rand((P, 1, 3), device="cuda", generator=g) * 50
    m._vertex = torch.nn.Parameter(centre + torch.randn((P, 3, 3), device="cuda", generator=g) * 0.2)
    opacity = torch.randn((P, 1), device="cuda", generator=g) * 2
    opacity[:8, 0] = torch.tensor([100.0, -100.0, math.inf, -math.inf, math.nan, -0.0, 0.0, 20.0], device="cuda")
    m._opacity = torch.nn.Parameter(opacity)
    m._f_dc = torch.nn.Parameter(torch.rand((P, 1, 3), device="cuda", generator=g))
    m._f_rest = torch.nn.Parameter(torch.rand((P, (sh_degree + 1) ** 2 - 1, 3), device="cuda", generator=g))
    m.optimizer = torch.optim.Adam([{"params": [getattr(m, "_" + n)], "lr": 1e-3, "name": n} for n in PARAMS], lr=0.0, eps=1e-15)
    for n in PARAMS:
        getattr(m, "_" + n).grad = torch.randn(getattr(m, "_" + n).shape, device="cuda", generator=g)
    m.optimizer.step()
    for n in PARAMS:
        getattr(m, "_" + n).grad = None
    m.gradient_denom = torch.randint(0, 10, (P,), device="cuda", generator=g).float()
    m.gradient_accum = torch.rand((P,), device="cuda", generator=g) * m.gradient_denom * 0.5
    m.max_radii2D = torch.randint(0, 80, (P,), device="cuda", generator=g).float()
    m.contrib_sum = torch.rand((P,), device="cuda", generator=g) * 4
    m.contrib_max = torch.rand((P,), device="cuda", generator=g)
    m.contrib_denom = torch.randint(0, 10, (P,), device="cuda", generator=g).float()
    it = NS(start_iter=0, end_iter=1000, hold_iter=1000, interval_iter=100)
    m.config = NS(model_update=NS(
        densification=NS(**vars(it), min_view_count=4, split_num=2, split_scale_threshold=0.45),
        opacity_pruning=NS(**vars(it)), opacity_clipping=NS(**vars(it)),
        scale_pruning=NS(**vars(it), radii_threshold=70.0, scale_threshold=0.7),
        scale_clipping=NS(**vars(it)), opacity_reset=NS(**vars(it), reset_value=0.3)))
    m.grad_threshold_scheduler = lambda step: 0.21
    m.opacity_pruning_scheduler = lambda step: 0.25
    m.opacity_clipping_scheduler = lambda step: 0.9
    m.scale_max_scheduler = lambda step: 0.6
    return m


def _snapshot(m):
    snap = {}
    for n in PARAMS:
        p = getattr(m, "_" + n)
        st = m.optimizer.state[p]
        snap[n] = (p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    for n in STATS:
        snap[n] = getattr(m, n).clone()
    return snap


def _expect_rows(snap, rows):
    """Every tensor of the snapshot through `rows(t, kind)`, kind in ("param", "moment", "stat")."""
    out = {}
    for n in PARAMS:
        p, ea, es = snap[n]
        out[n] = (rows(p, "param", n), rows(ea, "moment", n), rows(es, "moment", n))
    for n in STATS:
        out[n] = rows(snap[n], "stat", n)
    return out


def _compare(m, want, rule, close=()):
    """Parameters (still registered in the optimizer, requiring grad), both moments and the statistics against `want`: bit for bit, except
    the parameters named in `close`, which must show the same inf / NaN pattern and agree to the golden test's tolerance."""
    import torch
    for k, n in enumerate(PARAMS):
        p = getattr(m, "_" + n)
        assert m.optimizer.param_groups[k]["params"][0] is p and p.requires_grad, (rule, n)
        st = m.optimizer.state[p]
        for got, exp, part in ((p.detach(), want[n][0], "param"), (st["exp_avg"], want[n][1], "exp_avg"),
                               (st["exp_avg_sq"], want[n][2], "exp_avg_sq")):
            assert got.shape == exp.shape, (rule, n, part, tuple(got.shape), tuple(exp.shape))
            if part == "param" and n in close:
                fin = torch.isfinite(exp)
                assert torch.equal(fin, torch.isfinite(got)) and torch.equal(torch.isnan(exp), torch.isnan(got)), (rule, n, "non-finite pattern")
                assert torch.equal(got[~fin & ~torch.isnan(exp)], exp[~fin & ~torch.isnan(exp)]), (rule, n, "infinities")
                torch.testing.assert_close(got[fin], exp[fin], rtol=2e-6, atol=2e-7, msg=f"{rule}/{n}")
            else:
                assert _same_bits(got, exp), (rule, n, part)
    for n in STATS:
        assert _same_bits(getattr(m, n), want[n]), (rule, n)


RULES = ["prune_points", "densification", "opacity_pruning", "opacity_clipping", "scale_pruning", "scale_clipping", "opacity_reset"]


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("sh_degree", [3, 0])
def test_structural_rules_at_one_million_triangles_equal_their_torch_restatement(sh_degree, rule):
    """Each rule on a 1 M-triangle model (SH 3, and SH 0 where f_rest is (P, 0, 3)) against a torch statement of the rule: kept rows in
    order, then clones, then first children, then second children; new rows with zero moments and zero statistics; clipped rows with
    zero moments.  Row movement and split midpoints are exact; the clip rescale and the reset agree with torch's float32 evaluation to
    rtol 2e-6 / atol 2e-7 with the same inf / NaN pattern (the model's opacities include +-100, +-inf, NaN and -0.0)."""
    import torch
    import diff_recon_hip as D
    P = 1_000_003
    m = _big_model(P, sh_degree, seed=11 + sh_degree)
    snap = _snapshot(m)
    v, op = snap["vertex"][0], snap["opacity"][0]
    _, scaling = _mean_side(v)
    close = ()
    if rule == "prune_points":
        g = torch.Generator(device="cuda").manual_seed(4)
        prune = torch.rand(P, device="cuda", generator=g) < 0.3
        assert D.prune_points(m, prune) == P - int(prune.sum())
        want = _expect_rows(snap, lambda t, kind, n: t[~prune])
    elif rule in ("opacity_pruning", "scale_pruning"):
        if rule == "opacity_pruning":
            prune = (torch.sigmoid(op) < 0.25).squeeze(-1)
        else:
            prune = (snap["max_radii2D"] > 70.0) | (scaling > 0.7)
        assert 0 < int(prune.sum()) < P
        assert getattr(D, rule)(m, 100) == int(prune.sum())
        want = _expect_rows(snap, lambda t, kind, n: t[~prune])
    elif rule == "densification":
        den, acc = snap["gradient_denom"], snap["gradient_accum"]
        select = den >= 4
        grow = select & (acc > 0.21 * den)
        large = scaling > 0.45
        clone, split = grow & ~large, grow & large
        n_c, n_s = int(clone.sum()), int(split.sum())
        assert n_c > 1000 and n_s > 1000, (n_c, n_s)
        c1, c2 = _children(v[split])
        keep = ~split

        def rows(t, kind, n):
            if kind == "stat":
                if n in ("gradient_accum", "gradient_denom"):
                    t = torch.where(select, torch.zeros_like(t), t)
                return torch.cat((t[keep], torch.zeros((n_c + 2 * n_s,), device="cuda")))
            if kind == "moment":
                return torch.cat((t[keep], torch.zeros((n_c + 2 * n_s,) + tuple(t.shape[1:]), device="cuda")))
            if n == "vertex":
                return torch.cat((t[keep], t[clone], c1, c2))
            return torch.cat((t[keep], t[clone], t[split], t[split]))

        assert D.densification(m, 100) == (n_c + n_s, n_c, n_s)
        want = _expect_rows(snap, rows)
    elif rule == "opacity_clipping":
        clip = (torch.sigmoid(op) > 0.9).squeeze(-1)
        assert D.opacity_clipping(m, 100) == int(clip.sum()) > 0

        def rows(t, kind, n):
            if n != "opacity" or kind == "stat":
                return t
            t = t.clone()
            t[clip] = 10.0 if kind == "param" else 0.0
            return t

        want = _expect_rows(snap, rows)
    elif rule == "scale_clipping":
        clip = scaling > 0.6
        assert D.scale_clipping(m, 100) == int(clip.sum()) > 0
        vc = v[clip]
        centre = vc.mean(dim=1, keepdim=True)
        rescaled = (vc - centre) * (0.6 / scaling[clip]).view(-1, 1, 1) + centre

        def rows(t, kind, n):
            if n != "vertex" or kind == "stat":
                return t
            t = t.clone()
            t[clip] = rescaled if kind == "param" else 0.0
            return t

        want = _expect_rows(snap, rows)
        close = ("vertex",)
    else:  # opacity_reset: inverse_sigmoid(min(sigmoid(opacity), reset_value)); every row's moments restart at zero
        x = torch.minimum(torch.sigmoid(op), torch.full_like(op, 0.3))
        reset = torch.log(x / (1 - x))
        assert torch.isnan(reset[4, 0]) and reset[3, 0] == -math.inf and reset[1, 0] == -math.inf  # NaN stays NaN, -inf / -100 give -inf
        assert D.opacity_reset(m, 100) == P

        def rows(t, kind, n):
            if n != "opacity" or kind == "stat":
                return t
            return reset if kind == "param" else torch.zeros_like(t)

        want = _expect_rows(snap, rows)
        close = ("opacity",)
    _compare(m, want, rule, close)


# ---- 4. decisions at ties and one ulp either side of the thresholds -------------------------------------------------------------------
def _tie_triangles():
    """Triangles whose side lengths are exact (integer coordinates, scaled by powers of two) with tied longest sides in every position,
    the equilateral corner triangle of create_from_pcd, integer sides whose mean (50/3) is not a float32, and a single point."""
    import itertools
    import torch
    base = [
        [[0, 0, 0], [16, 0, 0], [8, 15, 0]],   # 16, 17, 17: mean 50/3
        [[0, 0, 0], [10, 0, 0], [5, 12, 0]],   # 10, 13, 13
        [[0, 0, 0], [6, 0, 0], [3, 4, 0]],     # 6, 5, 5
        [[0, 0, 0], [24, 0, 0], [12, 5, 0]],   # 24, 13, 13: mean 50/3
        [[0, 0, 0], [3, 0, 0], [0, 4, 0]],     # 3, 4, 5
        [[1, 0, 0], [0, 1, 0], [0, 0, 1]],     # equilateral, sides sqrt(2)
        [[0, 0, 0], [2, 0, 0], [1, 1, 0]],     # 2, sqrt 2, sqrt 2
        [[3, 3, 3], [3, 3, 3], [3, 3, 3]],     # every side 0
    ]
    tris = []
    for t in base:
        for perm in itertools.permutations(range(3)):
            for scale, shift in ((1.0, 0.0), (0.25, 7.0), (1024.0, -3.0)):
                tris.append([[c * scale + shift for c in t[k]] for k in perm])
    return torch.tensor(tris, device="cuda", dtype=torch.float32)


def test_split_vertex_follows_argmax_first_maximum_on_tied_sides():
    import torch
    from diff_recon_hip.model_update import _lib
    from diff_triangle_rasterization_2D._C import stream as _stream
    v = _tie_triangles()
    n = v.shape[0]
    sides, _ = _mean_side(v)
    assert (sides.max(dim=1).values == sides.sort(dim=1).values[:, 1]).sum() >= n // 2  # half the rows have tied longest sides
    parents = torch.arange(n - 1, -1, -1, device="cuda", dtype=torch.int32)  # descending parents
    c1 = torch.full((n, 3, 3), float("nan"), device="cuda")
    c2 = torch.full((n, 3, 3), float("nan"), device="cuda")
    assert _lib.tsm_split_vertex(n, parents.data_ptr(), v.data_ptr(), c1.data_ptr(), c2.data_ptr(), _stream()) == 0
    w1, w2 = _children(v[parents.long()])
    assert _same_bits(c1, w1) and _same_bits(c2, w2), (c1 != w1).any(dim=(1, 2)).nonzero().flatten().tolist()


def _update_mask(mode, opacity, vertex, max_radii, a, b=0.0):
    import torch
    from diff_recon_hip.model_update import _lib
    from diff_triangle_rasterization_2D._C import stream as _stream
    out = torch.empty((vertex.shape[0],), device="cuda", dtype=torch.uint8)
    assert _lib.tsm_update_mask(vertex.shape[0], mode, opacity.data_ptr(), vertex.data_ptr(), max_radii.data_ptr(), float(a), float(b),
                                out.data_ptr(), _stream()) == 0
    return out.bool()


def test_opacity_masks_on_and_around_their_thresholds():
    """Modes 0 (sigmoid(opacity) < a) and 1 (> a) on 8192 consecutive float32 opacities around the logit of each threshold, so that torch's
    sigmoid lands on the threshold and on its neighbours; thresholds at the scheduled value and one ulp either side of a sigmoid value
    that occurs."""
    import torch
    for a in (0.25, 0.9, 0.005):
        x0 = np.float32(math.log(a / (1 - a)))
        xs = (torch.tensor([x0], dtype=torch.float32).view(torch.int32) + torch.arange(-4096, 4096, dtype=torch.int32)).view(torch.float32)
        op = xs.cuda().view(-1, 1).contiguous()
        s = torch.sigmoid(op).squeeze(-1)
        mid = float(s[4096])
        vertex = torch.zeros((op.shape[0], 3, 3), device="cuda")
        radii = torch.zeros((op.shape[0],), device="cuda")
        for thr in (a, _ulp_down(a), _ulp_up(a), mid, _ulp_down(mid), _ulp_up(mid)):
            t32 = float(np.float32(thr))
            assert ((s < t32).any() and (s > t32).any()), (a, thr)
            assert torch.equal(_update_mask(0, op, vertex, radii, thr), s < t32), ("mode 0", a, thr)
            assert torch.equal(_update_mask(1, op, vertex, radii, thr), s > t32), ("mode 1", a, thr)
        assert (s == mid).sum() >= 1


def test_scale_masks_on_and_around_their_thresholds():
    """Modes 2 (max_radii2D > a or mean side > b) and 3 (mean side > a) with the thresholds placed on torch's mean side of each exact
    triangle and one ulp either side, and max_radii2D on and one ulp either side of the radius threshold."""
    import torch
    v = _tie_triangles()
    n = v.shape[0]
    _, scaling = _mean_side(v)
    op = torch.zeros((n, 1), device="cuda")
    r0 = 50.0
    radii = torch.tensor([r0, _ulp_down(r0), _ulp_up(r0), 0.0], device="cuda").repeat((n + 3) // 4)[:n].contiguous()
    for t in sorted(set(scaling.tolist())):
        for thr in (t, _ulp_down(t), _ulp_up(t)):
            assert torch.equal(_update_mask(3, op, v, radii, thr), scaling > thr), ("mode 3", thr)
            assert torch.equal(_update_mask(2, op, v, radii, r0, thr), (radii > r0) | (scaling > thr)), ("mode 2", thr)
            assert torch.equal(_update_mask(2, op, v, radii, _ulp_down(r0), thr), (radii > _ulp_down(r0)) | (scaling > thr)), ("mode 2 r-", thr)


def test_mean_side_and_longest_side_of_inexact_triangles_follow_torch():
    """The same decisions on triangles whose side lengths round: training-like triangles, and corner triangles of create_from_pcd scaled and
    moved by inexact amounts, whose three sides nearly tie.  The kernels form side lengths and mean as torch's GPU norm and mean do, so mode 3
    agrees with torch with the threshold on a row's own mean side and one ulp either side, and split_vertex picks torch.argmax's side."""
    import torch
    from diff_recon_hip.model_update import _lib
    from diff_triangle_rasterization_2D._C import stream as _stream
    P = 1_000_003
    g = torch.Generator(device="cuda").manual_seed(77)
    half = P // 2
    train = torch.rand((half, 1, 3), device="cuda", generator=g) * 50 + torch.randn((half, 3, 3), device="cuda", generator=g) * 0.2
    corner = torch.eye(3, device="cuda").expand(P - half, 3, 3)
    corner = corner * (torch.rand((P - half, 1, 1), device="cuda", generator=g) * 0.7 + 0.01) \
        + torch.randn((P - half, 1, 3), device="cuda", generator=g) * 20
    v = torch.cat((train, corner)).contiguous()
    _, scaling = _mean_side(v)
    op = torch.zeros((P, 1), device="cuda")
    radii = torch.zeros((P,), device="cuda")
    rows = torch.randint(0, P, (12,), device="cuda", generator=g).tolist() + [0, half, P - 1]
    for k in rows:
        t = float(scaling[k])
        for thr in (t, _ulp_down(t), _ulp_up(t)):
            got, want = _update_mask(3, op, v, radii, thr), scaling > thr
            assert torch.equal(got, want), (k, thr, (got != want).nonzero().flatten()[:8].tolist())
    parents = torch.arange(P, device="cuda", dtype=torch.int32)
    c1, c2 = torch.empty_like(v), torch.empty_like(v)
    assert _lib.tsm_split_vertex(P, parents.data_ptr(), v.data_ptr(), c1.data_ptr(), c2.data_ptr(), _stream()) == 0
    w1, w2 = _children(v)
    bad = ((c1 != w1) | (c2 != w2)).flatten(1).any(dim=1)
    assert not bad.any(), bad.nonzero().flatten()[:8].tolist()


def test_grow_classify_on_and_around_its_thresholds():
    """_densification's selection and _grow_points' classification with gradient_accum equal to torch's grad_threshold * gradient_denom and
    one ulp either side, gradient_denom on and one ulp either side of min_view_count, and the mean side on and one ulp either side of the
    split threshold; the selected rows' accumulators are reset."""
    import torch
    from diff_recon_hip.model_update import _lib
    from diff_triangle_rasterization_2D._C import stream as _stream
    v = _tie_triangles()
    _, scaling = _mean_side(v)
    mvc = 4.0
    dens = torch.tensor([_ulp_down(mvc), mvc, _ulp_up(mvc), mvc + 1, 0.0, 7.0], device="cuda")
    for grad_thr in (0.21, 0.0002, 1e-30):
        for split_thr in sorted(set(scaling.tolist()))[1::3]:
            for st in (split_thr, _ulp_down(split_thr), _ulp_up(split_thr)):
                n = v.shape[0] * dens.numel() * 3
                vert = v.repeat(dens.numel() * 3, 1, 1).contiguous()
                den = dens.repeat_interleave(v.shape[0]).repeat(3).contiguous()
                prod = grad_thr * den  # torch's float32 product of the threshold and the count
                step = torch.tensor([-1, 0, 1], device="cuda", dtype=torch.int32).repeat_interleave(v.shape[0] * dens.numel())
                acc = (prod.view(torch.int32) + step * (prod != 0).int()).view(torch.float32).contiguous()
                acc0, den0 = acc.clone(), den.clone()
                code = torch.empty((n,), device="cuda", dtype=torch.uint8)
                assert _lib.tsm_grow_classify(n, vert.data_ptr(), acc.data_ptr(), den.data_ptr(), mvc, grad_thr, st, code.data_ptr(),
                                              _stream()) == 0
                select = den0 >= mvc
                grow = select & (acc0 > grad_thr * den0)
                large = scaling.repeat(dens.numel() * 3) > st
                want = torch.where(grow, torch.where(large, 2, 1), 0).to(torch.uint8)
                assert torch.equal(code, want), (grad_thr, st, (code != want).nonzero().flatten()[:8].tolist())
                assert _same_bits(acc, torch.where(select, torch.zeros_like(acc0), acc0))
                assert _same_bits(den, torch.where(select, torch.zeros_like(den0), den0))


# ---- 5. training_statistic --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rich", [True, False])
@pytest.mark.parametrize("V", [1, 3, 8])
def test_training_statistic_equals_the_sequential_float64_rule(V, rich):
    """VanillaTS_model.py:347-363 applied view after view in float64, against one launch over V views of 1 000 003 triangles: radii with
    zeros, rows invisible in every view (untouched bit for bit), one NaN center2D gradient that must reach gradient_accum like the
    reference's `+=`.  gradient_accum to rtol 1e-6, everything else exact; without rich_info contrib_sum / contrib_max stay as they were."""
    import torch
    from diff_recon_hip.model_update import _lib
    from diff_triangle_rasterization_2D._C import stream as _stream
    P = 1_000_003
    g = torch.Generator(device="cuda").manual_seed(31 * V + rich)
    radii = torch.randint(0, 6, (V, P), device="cuda", generator=g, dtype=torch.int32)
    radii[torch.rand((V, P), device="cuda", generator=g) < 0.3] = 0
    hidden = torch.zeros(P, device="cuda", dtype=torch.bool)
    hidden[::7] = True
    hidden[-1] = True
    radii[:, hidden] = 0
    nan_row = 12_345
    radii[:, nan_row] = 3
    grad = torch.randn((V, P, 2), device="cuda", generator=g) * 3
    grad[V // 2, nan_row, 1] = float("nan")
    csum = torch.rand((V, P), device="cuda", generator=g) * 4
    cmax = torch.rand((V, P), device="cuda", generator=g)
    state = {"gradient_accum": torch.rand(P, device="cuda", generator=g) * 10,
             "gradient_denom": torch.randint(0, 20, (P,), device="cuda", generator=g).float(),
             "max_radii2D": torch.randint(0, 8, (P,), device="cuda", generator=g).float(),
             "contrib_sum": torch.rand(P, device="cuda", generator=g) * 4,
             "contrib_max": torch.rand(P, device="cuda", generator=g),
             "contrib_denom": torch.randint(0, 20, (P,), device="cuda", generator=g).float()}
    before = {k: t.clone() for k, t in state.items()}
    ref = {k: t.double() for k, t in state.items()}
    for v in range(V):
        vis = radii[v] > 0
        ref["gradient_accum"][vis] += grad[v][vis].double().norm(dim=-1)
        ref["gradient_denom"][vis] += 1
        if rich:
            ref["contrib_sum"][vis] = torch.maximum(ref["contrib_sum"][vis], csum[v][vis].double())
            ref["contrib_max"][vis] = torch.maximum(ref["contrib_max"][vis], cmax[v][vis].double())
        ref["contrib_denom"][vis] += 1
        ref["max_radii2D"][vis] = torch.maximum(ref["max_radii2D"][vis], radii[v][vis].double())
    rc = _lib.tsm_training_statistic(P, V, radii.data_ptr(), grad.data_ptr(), csum.data_ptr() if rich else None,
                                     cmax.data_ptr() if rich else None, *(state[k].data_ptr() for k in STATS), _stream())
    assert rc == 0
    for k in STATS:
        assert _same_bits(state[k][hidden], before[k][hidden]), ("invisible rows moved", k)
    if not rich:
        assert _same_bits(state["contrib_sum"], before["contrib_sum"]) and _same_bits(state["contrib_max"], before["contrib_max"])
    acc, want = state["gradient_accum"], ref["gradient_accum"]
    assert torch.isnan(acc[nan_row]) and torch.equal(torch.isnan(acc), torch.isnan(want))
    fin = ~torch.isnan(want)
    rel = ((acc[fin].double() - want[fin]).abs() / want[fin].abs().clamp_min(1e-30)).max()
    assert rel <= 1e-6, float(rel)
    for k in STATS[1:]:
        assert torch.equal(state[k].double(), ref[k]), k
