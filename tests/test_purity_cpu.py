"""The poison harness itself (tests/poison.py), on CPU tensors: pattern tiling, the torch.empty patch and its restoration, the guard bands,
and the positive control -- assert_pure flags a function that reads its workspace before writing it, and passes a pure one."""
import pytest
import torch

import poison


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 7, 8, 13, 4099])
@pytest.mark.parametrize("pattern", list(poison.PATTERNS))
def test_pattern_tiles_odd_lengths(pattern, n):
    b = poison.pattern_bytes(pattern, n)
    assert b.dtype == torch.uint8 and b.numel() == n
    word = poison.PATTERNS[pattern].to_bytes(4, "little")
    assert bytes(b.tolist()) == (word * (n // 4 + 1))[:n]


def test_patterns_read_as_intended():
    with poison.PoisonedEmpty("ones"):
        assert torch.empty(5, dtype=torch.int32).tolist() == [1] * 5
    with poison.PoisonedEmpty("float1"):
        assert torch.empty(2, 3).tolist() == [[1.0] * 3] * 2
    with poison.PoisonedEmpty("nan"):
        assert torch.empty((3,), dtype=torch.float32).isnan().all()
    with poison.PoisonedEmpty("allbits"):
        assert torch.empty(3, dtype=torch.int64).tolist() == [-1] * 3
        assert torch.empty(3, dtype=torch.uint8).tolist() == [255] * 3
    with poison.PoisonedEmpty("zero"):
        assert torch.empty(4, dtype=torch.float64).tolist() == [0.0] * 4


def test_poisoned_empty_shapes_and_alignment():
    with poison.PoisonedEmpty("nan") as pe:
        for args, shape in (((3,), (3,)), ((2, 5), (2, 5)), (((4, 1),), (4, 1)), ((torch.Size([2, 2]),), (2, 2)), ((0,), (0,)), (((),), ())):
            t = torch.empty(*args, dtype=torch.float32)
            assert tuple(t.shape) == shape and t.is_contiguous()
            assert t.data_ptr() % 16 == 0  # the guard keeps the alignment of the parent allocation
        t = torch.empty(7, dtype=torch.uint8)
        assert t.tolist() == [0x00, 0x00, 0xC0, 0x7F, 0x00, 0x00, 0xC0]  # an odd tail is cut, not dropped
        assert len(pe.records) == 7
        pe.check_guards()


def test_poisoned_empty_restores_torch_empty():
    real = torch.empty
    with poison.PoisonedEmpty("ones"):
        assert torch.empty is not real
        with poison.PoisonedEmpty("nan"):  # nested: the inner one wins, then the outer one is back
            assert torch.empty(1).isnan().all()
        assert torch.empty(1, dtype=torch.int32).item() == 1
    assert torch.empty is real
    with pytest.raises(RuntimeError, match="boom"):
        with poison.PoisonedEmpty("ones"):
            raise RuntimeError("boom")
    assert torch.empty is real


@pytest.mark.parametrize("where", ["after", "before"])
def test_write_one_byte_outside_is_reported(where):
    with poison.PoisonedEmpty("float1") as pe:
        t = torch.empty(5, dtype=torch.uint8)  # 5 bytes: the guard starts at an odd address
        t.fill_(7)                             # writing all of the tensor is fine
        pe.check_guards()
        parent = pe.records[0][0]
        parent[poison.GUARD + 5 if where == "after" else poison.GUARD - 1] = 0
        with pytest.raises(poison.GuardError, match="byte offset 5 " if where == "after" else "byte offset -1 "):
            pe.check_guards()


# ---- the positive control: a two-stage sum whose finisher reads more partials than the first stage wrote --------------------------------------
SLOTS = 8


def leaky_sum(x):
    ws = torch.empty(SLOTS, dtype=torch.int32, device=x.device)
    nb = min(SLOTS, x.numel())
    ws[:nb] = x.reshape(-1)[:nb * (x.numel() // nb)].reshape(nb, -1).sum(1)
    return ws.sum()  # wrong: reads SLOTS partials, nb were written


def pure_sum(x):
    ws = torch.empty(SLOTS, dtype=torch.int32, device=x.device)
    nb = min(SLOTS, x.numel())
    ws[:nb] = x.reshape(-1)[:nb * (x.numel() // nb)].reshape(nb, -1).sum(1)
    return ws[:nb].sum()


def check_positive_control(device):
    """Shared with tests/test_purity_gpu.py, which runs it once on the device."""
    # counts, not floats: 0x00000001 read as a float is a denormal that a float sum swallows
    small, large = torch.arange(1, 4, dtype=torch.int32, device=device), torch.arange(1, 17, dtype=torch.int32, device=device)
    poison.assert_pure(lambda p: pure_sum(small))
    poison.assert_pure(lambda p: pure_sum(large))
    poison.assert_pure(lambda p: leaky_sum(large))  # a saturated grid writes every partial: the leak does not show
    with pytest.raises(poison.PoisonLeak, match="pattern ones"):  # stops at the first pattern
        poison.assert_pure(lambda p: leaky_sum(small))
    tried = []
    with pytest.raises(poison.PoisonLeak):
        poison.assert_pure(lambda p: (tried.append(p), leaky_sum(small))[1])
    assert tried == ["zero", "zero", "ones"]  # no later pattern is tried after a difference

    def overrun(p):
        out = torch.empty(4, dtype=torch.float32, device=device)
        out.fill_(2.0)
        torch.as_strided(out, (5,), (1,))[4] = 2.0  # one element past the extent: inside the parent allocation, in the guard
        return out
    with pytest.raises(poison.GuardError, match="after"):
        poison.assert_pure(overrun)

    state = {"n": 0}

    def flaky(p):
        state["n"] += 1
        return torch.full((2,), float(state["n"]), device=device)
    with pytest.raises(poison.DeterminismError):
        poison.assert_pure(flaky)

    # raw bytes: -0.0 against +0.0 and a NaN payload both count
    with pytest.raises(poison.PoisonLeak):
        poison.assert_pure(lambda p: torch.tensor([0.0 if p == "zero" else -0.0], device=device))
    payload = torch.tensor([0x7FC00001], dtype=torch.int32, device=device).view(torch.float32)  # a NaN, but not the pattern's
    with pytest.raises(poison.PoisonLeak, match="pattern nan"):
        poison.assert_pure(lambda p: torch.empty(1, device=device) if p == "nan" else payload)


def test_positive_control_cpu():
    check_positive_control("cpu")


def test_filled_registers_with_the_active_context():
    with pytest.raises(AssertionError):
        poison.filled(4, torch.float32)
    with poison.PoisonedEmpty("ones") as pe:
        a = poison.filled((2, 3), torch.int32)
        b = poison.filled(3, torch.float32, "nan")
        assert a.tolist() == [[1] * 3] * 2 and b.isnan().all()
        assert len(pe.records) == 2
        torch.as_strided(b, (1,), (1,), 3)[0] = 0.0
        with pytest.raises(poison.GuardError):
            pe.check_guards()


def test_poison_blocks_skips_empty_sizes():
    other = torch.zeros(4)  # alive throughout: its address cannot be one of the blocks'
    held = poison.poison_blocks([0, 16, 0, 33], "allbits", device="cpu")
    assert len(held.ptrs) == 2
    with pytest.raises(AssertionError, match="not one of"):
        held.assert_used([other])
    held.assert_used([torch.zeros(0)])  # an empty buffer has no block
