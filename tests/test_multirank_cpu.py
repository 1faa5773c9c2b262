"""Host-side checks of image-parallel training's replica guard (diff_recon_hip/multirank.py), no GPU: the numpy restatement of the state
digest against its definition (include/ts_model.h: tsm_state_digest), the ReplicaGuard protocol over gloo with two CPU ranks, and the
argument check of `train(world=N)`."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def mr(hip_lib_built):
    from diff_recon_hip import multirank
    return multirank


def _u64(t):
    return int(t) & MASK


def _ref(mr, words):
    w = np.asarray(words, dtype=np.uint32)
    return _u64(mr.state_digest_reference({"x": torch.from_numpy(w.view(np.int32).copy())})[0])


def _mix64(z):  # the splitmix64 finaliser on Python integers: the definition written out a second time, independent of numpy's wrap-around
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def _pair_terms(words):
    w = list(int(x) for x in words) + ([0] if len(words) & 1 else [])
    return [_mix64((w[2 * j] | (w[2 * j + 1] << 32)) ^ (((j + 1) * 0x9E3779B97F4A7C15) & MASK)) for j in range(len(w) // 2)]


def test_fixed_values(mr):
    """Computed from the definition by a throw-away script, not by the function under test."""
    assert _ref(mr, []) == 0
    assert _ref(mr, [0x00000000]) == 0xE220A8397B1DCDAF
    assert _ref(mr, [0x80000000]) == 0x25493CC63225736C  # -0.0f: the bit pattern counts, not the value
    z = mr.state_digest_reference({"p": torch.zeros(1), "n": -torch.zeros(1), "e": torch.zeros(0)})
    assert z.dtype == torch.int64 and [_u64(v) for v in z] == [0xE220A8397B1DCDAF, 0x25493CC63225736C, 0]


def test_reference_follows_the_definition_term_by_term(mr):
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 7, 64, 65, 1001):  # odd counts: the missing last high half is 0
        w = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        assert _ref(mr, w) == sum(_pair_terms(w)) & MASK
    w = rng.integers(0, 1 << 32, size=5, dtype=np.uint64).astype(np.uint32)
    assert _ref(mr, w) == _ref(mr, list(w) + [0]) != _ref(mr, list(w) + [0, 0])  # a zero high half is the padding; a further PAIR is a further term


def test_one_flipped_bit_and_a_swap_of_two_pairs_change_the_digest(mr):
    rng = np.random.default_rng(6)
    w = rng.integers(0, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32)
    base = _ref(mr, w)
    for word, bit in ((0, 0), (1, 31), (4095, 7), (2048, 16)):
        v = w.copy()
        v[word] ^= np.uint32(1 << bit)
        assert _ref(mr, v) != base
    v = w.copy()
    v[[10, 11, 20, 21]] = w[[20, 21, 10, 11]]  # pairs 5 and 10 change places: a plain sum of mixed values would not notice, the index key does
    assert (w[10], w[11]) != (w[20], w[21]) and _ref(mr, v) != base


def test_digest_is_the_sum_of_the_partial_sums_over_any_split_of_the_pair_range(mr):
    """What makes the GPU result independent of block shape, grid size and atomic order."""
    rng = np.random.default_rng(7)
    w = rng.integers(0, 1 << 32, size=2 * 777 + 1, dtype=np.uint64).astype(np.uint32)
    terms = _pair_terms(w)
    total = _ref(mr, w)
    for cuts in ([0, 778], [0, 1, 778], [0, 256, 512, 778], sorted({0, 778, *rng.integers(0, 778, size=40).tolist()})):
        parts = [sum(terms[a:b]) & MASK for a, b in zip(cuts[:-1], cuts[1:])]
        for order in (parts, parts[::-1]):
            acc = 0
            for p in order:
                acc = (acc + p) & MASK
            assert acc == total


def test_reference_refuses_what_the_kernel_refuses(mr):
    with pytest.raises(ValueError, match="multiple of 4"):
        mr.state_digest_reference({"x": torch.zeros(6, dtype=torch.uint8)})
    with pytest.raises(ValueError, match="contiguous"):
        mr.state_digest_reference({"x": torch.zeros(4, 4).t()})
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the device digest has no host path
        mr.state_digest({"x": torch.zeros(4)})


# ---- ReplicaGuard over gloo, two CPU ranks, the reference digest injected ----------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _guard_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path[:0] = [ROOT, os.path.join(ROOT, "triangle-splatting_amd")]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from diff_recon_hip import multirank as mr
        calls = [0]
        real = dist.all_gather_into_tensor

        def counted(*a, **kw):
            calls[0] += 1
            return real(*a, **kw)

        mr.dist.all_gather_into_tensor = counted  # every collective of the guard goes through this name
        g = torch.Generator().manual_seed(3)
        state = {"vertex": torch.randn(50, 3, 3, generator=g), "opacity": torch.randn(50, 1, generator=g), "max_radii2D": torch.zeros(50)}
        guard = mr.ReplicaGuard(every=5, digest_fn=mr.state_digest_reference)
        out = {}
        # off schedule: nothing at all
        ran = [guard.check(it, state, 50) for it in (1, 2, 3, 4, 6)]
        out["off_schedule"] = (ran, calls[0])
        # on schedule and forced: one collective each, equal state passes
        ran = [guard.check(5, state, 50), guard.check(7, state, 50, force=True)]
        out["on_schedule"] = (ran, calls[0], guard.checks)
        # one ulp in one tensor on rank 1
        bad = {k: v.clone() for k, v in state.items()}
        if rank == 1:
            bad["opacity"][17, 0] = torch.nextafter(bad["opacity"][17, 0], torch.tensor(float("inf")))
        try:
            guard.check(10, bad, 50)
            out["ulp"] = None
        except mr.ReplicaDivergence as e:
            out["ulp"] = (e.iteration, e.names, e.ranks)
        # -0.0 against 0.0: equal as numbers, different as bits
        bad = {k: v.clone() for k, v in state.items()}
        if rank == 1:
            bad["max_radii2D"][3] = -0.0
        try:
            guard.check(15, bad, 50)
            out["negzero"] = None
        except mr.ReplicaDivergence as e:
            out["negzero"] = (e.iteration, e.names, e.ranks)
        # a differing row count, same tensors
        try:
            guard.check(20, state, 50 + rank)
            out["rows"] = None
        except mr.ReplicaDivergence as e:
            out["rows"] = (e.iteration, e.names, e.ranks)
        out["calls"] = calls[0]
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_replica_guard_over_gloo_world_2(hip_lib_built):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_guard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    res = dict(q.get(timeout=10) for _ in range(2))
    for rank in (0, 1):  # every rank sees the same verdicts
        out = res[rank]
        assert out["off_schedule"] == ([False] * 5, 0)                    # no collective off schedule
        assert out["on_schedule"] == ([True, True], 2, 2)                 # one collective per check
        assert out["ulp"] == (10, ["opacity"], [1])                       # that tensor only, on both ranks
        assert out["negzero"] == (15, ["max_radii2D"], [1])
        assert out["rows"] == (20, ["num_rows"], [1])
        assert out["calls"] == 5


def test_guard_does_nothing_in_a_world_of_one(mr):
    guard = mr.ReplicaGuard(every=1, digest_fn=lambda named: (_ for _ in ()).throw(AssertionError("digested at world size 1")))
    assert guard.check(1, {"x": torch.zeros(4)}, 4) is False and guard.check(2, {"x": torch.zeros(4)}, 4, force=True) is False
    assert guard.checks == 0


def test_train_refuses_a_world_that_does_not_divide_the_views_before_any_process_starts(hip_lib_built, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import multiprocessing
    import train_synthetic
    started = []
    monkeypatch.setattr(multiprocessing.context.SpawnProcess, "start", lambda self: started.append(self))
    monkeypatch.setattr(torch.cuda, "device_count", lambda: (_ for _ in ()).throw(AssertionError("the GPU was asked about")))
    with pytest.raises(ValueError, match="multiple"):
        train_synthetic.train(world=3, views_per_step=4)
    assert not started
