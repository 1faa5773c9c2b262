"""Image-parallel training end to end (diff_recon_hip/multirank.py, examples/train_synthetic.py --world N) on the GPU: the state-digest kernel
against its host restatement, two ranks (two processes sharing the test box's one GPU over gloo) through the whole schedule of structural
updates with the replica guard on every iteration, parity against the one-process loop, and the guard catching a one-ulp corruption.

Every multi-rank run goes through train(world=N): fresh spawned children under a queue / join timeout, the first child that ends non-zero fails
the run and the others are ended; nothing is retried.  At most two ranks (plus this process) hold the GPU at a time.

Measured on an MI355X (profiles/multirank_parity.json; the bounds below are computed by the tests when they run, none is
hard-coded).  Short runs: s = 7e-9 .. 6e-7 (vertex), 1.5e-6 .. 1.7e-6 (raw opacity), 1.8e-7 .. 2.4e-7 (colour); the two-rank and world-1
distances inside max(4 s, 1e-6) in every run.  Long run, dense, final triangle count: 0.3 % .. 0.8 % from either one-process run (bound: relative
spread + 1 %), in every run.

KNOWN TO FAIL INTERMITTENTLY: the long run's final-loss bound in test_two_ranks_stay_bit_identical_through_every_structural_update[dense-False].
Seven runs, (spread of the two one-process final losses, larger distance of the two-rank final loss): (4.4e-5, 6.8e-5) (3.7e-5, 6.5e-5)
(5.8e-5, 1.8e-4) (3.6e-5, 1.6e-4) (2.9e-6, 1.7e-4) (2.0e-4, 2.7e-4) (7.0e-6, 3.1e-5) -- 1.5, 1.7, 3.1, 4.4, 61, 1.4 and 4.5 spreads against a bound
of 4: three failures, all with the replicas bit-identical and P inside its bound.  The final losses seen are one distribution (one process 0.02246 .. 0.02277, two
ranks 0.02248 .. 0.02270); the yardstick is a spread estimated from two draws, which can come out arbitrarily small.  The bound is kept as specified."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

MASK = (1 << 64) - 1
LONG = dict(iters=160, triangles=4000, width=160, height=112, views=3, views_per_step=2)  # test_training_loop_gpu.py's configuration
SHORT = dict(iters=5, triangles=4000, width=160, height=112, views=3, views_per_step=2, updates=False)
RULES = {"densification", "opacity_pruning", "scale_clipping", "contribution_pruning", "opacity_reset"}
_RECORD = {}


def _record(key, value):
    """Figures of this run: printed (pytest -s) and, when TS2D_PARITY_OUT names a file, kept there as JSON."""
    _RECORD[key] = value
    print(f"[multirank] {key}: {value}")
    path = os.environ.get("TS2D_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


# ---- 1. the digest kernel -------------------------------------------------------------------------------------------------------------
def _both(named):
    import diff_recon_hip as D
    got = D.state_digest(named).cpu()
    want = D.state_digest_reference({k: v.cpu() for k, v in named.items()})
    return got, want


def _rand_words(n, seed, dev):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    return torch.from_numpy(w.view(np.int32).copy()).to(dev)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4097, 5_000_001])
def test_digest_equals_the_reference_exactly_for_word_count(n):
    dev = torch.device("cuda", 0)
    x = _rand_words(n, 100 + n % 97, dev)
    got, want = _both({"x": x})
    assert got.dtype == torch.int64 and got.shape == (1,) and torch.equal(got, want), (n, hex(int(got[0]) & MASK), hex(int(want[0]) & MASK))
    again, _ = _both({"x": x})
    assert torch.equal(again, got)  # two launches, the same bits: no dependence on scheduling or atomic order
    if n == 0:
        assert int(got[0]) == 0


@pytest.mark.parametrize("segments", [1, 7, 32])
def test_digest_of_many_segments_in_one_call(segments):
    import diff_recon_hip as D
    assert D.MAX_DIGEST_SEGMENTS == 32
    dev = torch.device("cuda", 0)
    sizes = [(37 * k * k + 5 * k) % 9001 for k in range(segments)]  # includes an empty one (k = 0) and odd counts
    if segments == 32:
        sizes[5], sizes[6], sizes[20] = 4_100_000, 0, 5_000_001  # more chunks than the grid has blocks: every block walks across segment borders
    named = {f"s{k}": _rand_words(n, 7 + k, dev) for k, n in enumerate(sizes)}
    got = D.digest_segments(list(named.values()), list(named.keys())).cpu()  # ONE call of the entry point
    want = D.state_digest_reference({k: v.cpu() for k, v in named.items()})
    assert torch.equal(got, want), [(k, n) for (k, n), g, w in zip(zip(named, sizes), got, want) if g != w]


def test_one_segment_past_the_maximum_is_an_error_and_more_are_split_by_state_digest():
    import diff_recon_hip as D
    dev = torch.device("cuda", 0)
    named = {f"s{k}": _rand_words(10 + k, k, dev) for k in range(33)}
    with pytest.raises(RuntimeError, match=r"num_segments must be in 0\.\.32"):
        D.digest_segments(list(named.values()))
    got, want = _both(named)  # the dict form takes any number: two calls
    assert torch.equal(got, want)


def test_digest_sees_bit_patterns_of_every_dtype():
    import diff_recon_hip as D
    dev = torch.device("cuda", 0)
    tiny = np.array([1, 2, 0x007FFFFF, 0x80000001], dtype=np.uint32).view(np.float32)  # denormals
    nans = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001], dtype=np.uint32).view(np.float32)  # NaNs that differ only in payload / sign
    named = {
        "f32": torch.randn(1000, 3, 3, device=dev),
        "i32": torch.arange(-500, 501, device=dev, dtype=torch.int32),
        "u8": torch.arange(0, 256, device=dev, dtype=torch.uint8).repeat(3),  # 768 bytes
        "zeros": torch.zeros(5, device=dev), "negzeros": -torch.zeros(5, device=dev),
        "denormal": torch.from_numpy(tiny.copy()).to(dev), "nan": torch.from_numpy(nans.copy()).to(dev),
        "inf": torch.tensor([float("inf"), float("-inf")], device=dev),
        "unaligned": torch.randn(1001, device=dev)[1:],  # base 4 bytes past a 16-byte boundary: the word-by-word path
    }
    got, want = _both(named)
    assert torch.equal(got, want)
    d = dict(zip(named, got.tolist()))
    assert d["zeros"] != d["negzeros"]
    one = lambda t: int(D.state_digest({"x": t})[0])
    a = torch.from_numpy(nans.copy()).to(dev)
    b = a.clone()
    b.view(torch.int32)[1] ^= 1  # a NaN payload bit
    assert one(a) != one(b) and one(a) == one(a.clone())
    with pytest.raises(ValueError, match="multiple of 4"):
        D.state_digest({"x": torch.zeros(6, device=dev, dtype=torch.uint8)})
    with pytest.raises(ValueError, match="contiguous"):
        D.state_digest({"x": torch.zeros(4, 4, device=dev).t()})


# ---- the one-process yardstick: the parent commit's loop, run twice -------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _params_of_model(m):
    return {"vertex": m._vertex.detach().cpu().numpy(), "opacity": m._opacity.detach().cpu().numpy(),
            "colour": torch.cat([m._f_dc, m._f_rest], 1).detach().cpu().numpy()}


def _params_of_state(state):
    return {"vertex": state["vertex"], "opacity": state["opacity"], "colour": np.concatenate([state["f_dc"], state["f_rest"]], 1)}


@pytest.fixture(scope="module")
def short_runs():
    """train(views_per_step=2, updates=False), 5 iterations, twice with the same seed: the loop's own run-to-run spread `s` per parameter
    (float atomics in the backward make it non-zero in general)."""
    import train_synthetic
    runs = [_params_of_model(train_synthetic.train("2D", log=None, **SHORT)[1]) for _ in range(2)]
    s = {k: _rel(runs[0][k], runs[1][k]) for k in runs[0]}
    _record("short.s", s)
    return runs, s


@pytest.fixture(scope="module")
def long_runs():
    """The whole schedule, twice, one process: spread of the final loss and of the final triangle count."""
    import train_synthetic
    out = []
    for _ in range(2):
        losses, m, _ = train_synthetic.train("2D", log=None, **LONG)
        out.append((losses[-1], m._vertex.shape[0]))
    _record("long.one_process.final_loss", [o[0] for o in out])
    _record("long.one_process.final_P", [o[1] for o in out])
    return out


def _assert_short_parity(tag, state, short_runs):
    """Criterion 4: every parameter of the run within max(4 s, 1e-6) of EITHER one-process run.  4 s: two samples estimate a spread poorly;
    1e-6 ~ 16 fp32 ulps: the floor for a backward that happens to be deterministic."""
    runs, s = short_runs
    mine = _params_of_state(state)
    dist = {k: [_rel(mine[k], r[k]) for r in runs] for k in mine}
    _record(f"short.{tag}.distance", dist)
    for k in mine:
        bound = max(4.0 * s[k], 1e-6)
        assert all(d <= bound for d in dist[k]), (tag, k, dist[k], bound)


def _assert_replicas_identical(summary):
    a, b = summary.ranks[0], summary.ranks[1]
    assert a["rows"] == b["rows"]                                    # (i) P after every iteration
    assert a["guard_checks"] == b["guard_checks"] == len(a["rows"])  # (ii) the guard ran on every iteration and never raised
    assert sorted(a["state"]) == sorted(b["state"])
    names = set(a["state"])
    for p in ("vertex", "opacity"):
        assert {p, p + ".exp_avg", p + ".exp_avg_sq"} <= names
    assert {"gradient_accum", "gradient_denom", "max_radii2D", "contrib_sum", "contrib_max", "contrib_denom"} <= names
    for k in a["state"]:                                             # (iii) the tensors themselves, bit for bit
        x, y = a["state"][k], b["state"][k]
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), k
    assert a["log"] == b["log"] and a["losses"] == b["losses"]


def _assert_long_run(tag, losses, summary, long_runs, compare):
    kinds = {name for _, name, _, _ in summary.log}
    assert RULES <= kinds, kinds                                     # the five rules fired: not a vacuous pass
    grown = sum(res[0] for _, name, res, _ in summary.log if name == "densification")
    assert all(l == l for l in losses) and min(losses[-10:]) < 0.8 * losses[0], (losses[0], losses[-10:])  # (iv)
    assert grown > 0
    assert summary.gamma > 3.9 and summary.active_sh_degree == 2
    # against the one-process loop, only what survives 160 iterations of amplified ulps: the final loss within 4 x the spread of the two
    # one-process final losses of either of them, the final triangle count within their relative spread + 1 % of either.  The figures are
    # recorded for every run; they are a pass criterion for the dense exchange, the run this comparison is defined for (the bound is a
    # statistical one -- a third draw against a spread estimated from two -- and is not spent on every variant)
    (la, pa), (lb, pb) = long_runs
    loss_spread, p_spread = abs(la - lb), abs(pa - pb) / (0.5 * (pa + pb))
    P = summary.num_triangles
    fig = dict(final_loss=losses[-1], final_P=P, loss_spread=loss_spread, loss_distance=[abs(losses[-1] - la), abs(losses[-1] - lb)],
               P_relative_spread=p_spread, P_relative_distance=[abs(P - pa) / pa, abs(P - pb) / pb])
    _record(f"long.{tag}", fig)
    if not compare:
        return
    assert all(d <= 4.0 * loss_spread for d in fig["loss_distance"]), fig
    assert all(d <= p_spread + 0.01 for d in fig["P_relative_distance"]), fig


# ---- the statistics of gathered views are those of the one-process loop, bit for bit ---------------------------------------------------
def test_statistics_of_gathered_views_equal_sequential_single_view_updates_bit_for_bit():
    """What keeps a rank on the one-process loop's trajectory: the views a rank gathers go into the running statistics in view order, each added
    to the accumulator itself -- (acc + a) + b like two update() calls, not acc + (a + b), which differs in the last bit and flips borderline
    densification decisions 160 iterations later.  Repeated over several steps so that the accumulators are non-trivial."""
    from diff_recon_hip import DensificationStats
    from diff_recon_hip.model_update import _lib, _STATE
    P, V, steps = 20_000, 4, 6
    g = torch.Generator(device="cuda").manual_seed(11)
    a, b = DensificationStats(P, "cuda"), DensificationStats(P, "cuda")
    for _ in range(steps):
        radii = torch.randint(0, 3, (V, P), device="cuda", generator=g, dtype=torch.int32)
        grad = torch.randn((V, P, 2), device="cuda", generator=g) * 1e-3
        csum, cmax = torch.rand((V, P), device="cuda", generator=g), torch.rand((V, P), device="cuda", generator=g)
        for v in range(V):
            c2d = torch.zeros((P, 2), device="cuda", requires_grad=True)
            c2d.grad = grad[v].clone()
            a.update({"radii": radii[v], "center2D": c2d, "contrib_sum": csum[v], "contrib_max": cmax[v]})
        rc = _lib.tsm_training_statistic(P, V, radii.data_ptr(), grad.data_ptr(), csum.data_ptr(), cmax.data_ptr(), b.gradient_accum.data_ptr(),
                                         b.gradient_denom.data_ptr(), b.max_radii2D.data_ptr(), b.contrib_sum.data_ptr(), b.contrib_max.data_ptr(),
                                         b.contrib_denom.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    for k in _STATE:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


# ---- 2. / 3. two ranks through the whole schedule -------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange,single_sh", [("dense", False), ("factored_sh", False), ("factored_sh", True)])
def test_two_ranks_stay_bit_identical_through_every_structural_update(exchange, single_sh, long_runs):
    import train_synthetic
    losses, summary, _ = train_synthetic.train("2D", log=None, world=2, exchange=exchange, check_every=1, collect=True, single_sh=single_sh, **LONG)
    assert summary.world == 2 and len(summary.ranks) == 2
    _assert_replicas_identical(summary)
    _assert_long_run(f"{exchange}{'.single_sh' if single_sh else ''}", losses, summary, long_runs, compare=exchange == "dense")


# ---- 4. two ranks against one process, 5 iterations -----------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", ["dense", "factored_sh"])
def test_two_ranks_match_the_one_process_loop(exchange, short_runs):
    import train_synthetic
    _, summary, _ = train_synthetic.train("2D", log=None, world=2, exchange=exchange, check_every=1, collect=True, **SHORT)
    a, b = summary.ranks
    assert all(a["state"][k].tobytes() == b["state"][k].tobytes() for k in a["state"])
    _assert_short_parity(f"two_ranks.{exchange}", a["state"], short_runs)


# ---- 5. divergence is caught ----------------------------------------------------------------------------------------------------------
def _one_ulp_on_rank_1(iteration, m, rank):
    """Test-only on_iteration hook (runs in the children): after iteration 3 -- no rule fires before iteration 6 of this schedule -- rank 1
    moves ONE raw opacity by one ulp.  A wrong number, nothing else: the GPU is not disturbed.  Which one: the guard looks again after the next
    Adam step, and a step that carries the value across a power of two rounds on a grid twice as coarse, where one ulp can vanish (the replicas
    would then BE identical again, and rightly pass).  Raw opacities start at 0 and move by at most about lr = 0.05 a step; one whose magnitude
    lies in (0.13, 0.17) stays below 0.25 after the next step, so the ulp survives it."""
    if iteration == 3 and rank == 1:
        with torch.no_grad():
            o = m._opacity.data
            i = int(torch.nonzero((o[:, 0].abs() > 0.13) & (o[:, 0].abs() < 0.17))[0])
            o[i, 0] = torch.nextafter(o[i, 0], torch.full((), float("inf"), device=o.device))


def test_one_ulp_on_one_rank_is_caught_on_both():
    import diff_recon_hip as D
    import train_synthetic
    cfg = dict(LONG, iters=40)
    with pytest.raises(D.ReplicaDivergence) as info:
        train_synthetic.train("2D", log=None, world=2, check_every=1, on_iteration=_one_ulp_on_rank_1, **cfg)
    e = info.value
    assert e.exitcodes == [0, 0]                               # both children ended in an orderly way
    assert sorted(e.reports) == [0, 1]                         # raised on both ranks ...
    for rank in (0, 1):
        assert e.reports[rank] == (4, ["opacity"], [1])        # ... at the next check, naming `opacity` and nothing else, blaming rank 1


def test_without_the_corruption_the_same_run_passes_its_checks():
    """The control of the test above: same schedule, no hook."""
    import train_synthetic
    _, summary, _ = train_synthetic.train("2D", log=None, world=2, check_every=1, **dict(LONG, iters=8))
    assert [r["guard_checks"] for r in summary.ranks] == [8, 8]


# ---- 6. world size 1 through the same loop --------------------------------------------------------------------------------------------
def test_world_of_one_through_the_loop_matches_the_one_process_loop(short_runs):
    import train_synthetic
    _, summary, _ = train_synthetic.train("2D", log=None, world=1, check_every=1, collect=True, **SHORT)
    assert summary.world == 1 and summary.ranks[0]["guard_checks"] == 0  # nothing to compare at world size 1: no digest, no collective
    _assert_short_parity("world_1", summary.ranks[0]["state"], short_runs)
