"""The replay harness itself (tests/replay.py), on CPU tensors, where a tape of the dispatched operators stands in for the graph: it passes
an honest unit and rejects the torch-only positive controls.  tests/test_graph_replay_gpu.py runs the same controls once on the device."""
import pytest
import torch

import poison
import replay


def check_positive_controls(device):
    """Shared with tests/test_graph_replay_gpu.py."""
    a, b = replay.control_cases(device)
    base_a, base_b, n = replay.assert_replays(replay.honest_unit, a, b, differ=("total",))
    assert n == len(replay.SEQUENCE) * len(replay.PATTERNS) == 8
    assert base_a["total"].view(torch.int64).tolist() == [12] and base_b["total"].view(torch.int64).tolist() == [6]
    assert base_a["out"].view(torch.int32).tolist() == [2 * i for i in range(-3, 13)]

    with pytest.raises(replay.ReplayMismatch, match=r"replay 1 of 4 \(inputs A, captured on B, poison ones"):  # stops at the first replay
        replay.assert_replays(replay.host_value_unit(decoy_count=6), a, b)
    with pytest.raises(replay.ReplayMismatch, match=r"poison ones.*out: 1 of 64 bytes differ, the first at byte 60 \(0x00 against 0x01\)"):
        replay.assert_replays(replay.unwritten_tail_unit, a, b)

    # the cases must differ, and where the test says so: a graph that ignored its inputs would pass otherwise
    with pytest.raises(replay.VacuousCases, match="equal in every output"):
        replay.assert_replays(replay.honest_unit, a, {"x": a["x"].clone()})
    same_total = {"x": a["x"].flip(0)}
    with pytest.raises(replay.VacuousCases, match="output total"):
        replay.assert_replays(replay.honest_unit, a, same_total, differ=("total",))
    replay.assert_replays(replay.honest_unit, a, same_total)

    tried = []

    def wrong_on_allbits(inputs):  # the wild pattern is tried, and only after the in-range one passed
        out = replay.honest_unit(inputs)
        tried.append(poison._active[-1].pattern)
        if tried[-1] == "allbits":
            out["spare"] = torch.empty((2,), dtype=torch.int32, device=device)
        else:
            out["spare"] = torch.zeros((2,), dtype=torch.int32, device=device)
        return out
    with pytest.raises(replay.ReplayMismatch, match="poison allbits.*spare"):
        replay.assert_replays(wrong_on_allbits, a, b)
    assert tried == ["zero", "zero", "ones", "allbits"]

    def overrun(inputs):
        out = replay.honest_unit(inputs)
        n = out["out"].numel()
        torch.as_strided(out["out"], (n + 1,), (1,))[n:].fill_(1)  # one element past the extent: inside the parent allocation, in the guard
        return out
    with pytest.raises(poison.GuardError, match="after"):
        replay.assert_replays(overrun, a, b)

    def raises(inputs):
        raise RuntimeError("the call's own message")
    with pytest.raises(RuntimeError, match="the call's own message"):
        replay.assert_replays(raises, a, b)
    assert torch.empty is poison._empty  # every exit restored it


def test_positive_controls_cpu():
    check_positive_controls(torch.device("cpu"))


def test_tape_replays_what_the_host_saw_at_the_recording():
    x = torch.tensor([1, 2, 3])
    tape = replay._Tape()
    with tape:
        n = int(x.sum().item())  # a host read: 6 is baked in
        y = x * 2 + n
    assert y.tolist() == [8, 10, 12]
    x.copy_(torch.tensor([10, 20, 30]))
    tape.replay()
    assert y.tolist() == [26, 46, 66]  # the operators ran again on the new data, with the old 6


def test_cases_must_agree_in_shape_and_dtype():
    a = {"x": torch.zeros(4, dtype=torch.int32)}
    with pytest.raises(AssertionError, match="shape, dtype or device"):
        replay.assert_replays(replay.honest_unit, a, {"x": torch.zeros(5, dtype=torch.int32)})
    with pytest.raises(AssertionError, match="different inputs"):
        replay.assert_replays(replay.honest_unit, a, {"y": torch.zeros(4, dtype=torch.int32)})
