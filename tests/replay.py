"""Replaying entry points from a captured graph against eager runs (tests/test_graph_replay_gpu.py; DESIGN.md "Stream order of the mesh
entry points").

The mesh and geometry headers promise that every call is enqueued on `stream` and neither allocates nor synchronises with the host.  An eager
run on the current stream cannot show a launch on another stream, a host read or a clear that runs out of order; a graph that was captured
once and is replayed on other data can:

    assert_replays(call, case_a, case_b)    the harness: eager baselines of both cases, one capture on the decoy B, replays on A, B, B, A

`call(inputs)` takes a dict of input tensors, runs one or more sync-free entry points on the current stream and returns the dict of their
documented outputs, to their capacity.  It allocates outputs and workspaces with torch.empty (or poison.filled): the capture runs under
poison.PoisonedEmpty, so the fills are nodes of the graph and every replay starts from poisoned outputs, poisoned workspaces and whole guard
bands.  On CPU tensors a tape of the dispatched operators stands in for the graph (what the host computed while the tape was recorded is
baked into it, as in a capture), so that the harness and its torch-only positive controls run without a device."""
from __future__ import annotations

import torch
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils._pytree import tree_flatten

import poison

PATTERNS = ("ones", "allbits")  # poison.ORDER's idea: the in-range pattern first, the wild one only after every replay on it matched
SEQUENCE = "ABBA"               # what the static inputs hold at the four replays; B is what they held at the capture


class ReplayMismatch(AssertionError):
    """A replay of the captured graph disagrees with the eager run on the same inputs."""


class VacuousCases(AssertionError):
    """The two cases do not differ where the test says they must: a replay on stale data would pass."""


class _Tape(TorchDispatchMode):
    """The stand-in for a graph on the CPU: records every operator dispatched while it is active; replay() runs them again on the same tensor
    objects (an operator that returned a new tensor is run again and its result copied into the tensor it returned at the recording)."""

    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        self.ops.append((func, args, kwargs or {}, out))
        return out

    def replay(self):
        for func, args, kwargs, old in self.ops:
            new = func(*args, **kwargs)
            for o, n in zip(tree_flatten(old)[0], tree_flatten(new)[0]):
                if isinstance(o, torch.Tensor) and o is not n and o.numel() and o.data_ptr() != n.data_ptr():  # not an in-place result or a view
                    o.copy_(n)


def _capture(call, static, pattern, device):
    """(replay function, outputs, the PoisonedEmpty whose guards cover them): `call(static)` captured once on one side stream."""
    if device.type != "cuda":
        tape = _Tape()
        with poison.PoisonedEmpty(pattern) as pe, tape:
            out = call(static)
        return tape.replay, out, pe
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with poison.PoisonedEmpty(pattern) as pe:
            with torch.cuda.graph(graph, stream=side):  # an error or an exception of the call ends the capture and reaches the test
                out = call(static)
    torch.cuda.current_stream(device).wait_stream(side)

    def replay():
        graph.replay()
        torch.cuda.synchronize(device)
    return replay, out, pe


def _eager(call, case, outputs):
    with poison.PoisonedEmpty("zero") as pe:
        snap = poison._snapshot(call({k: t.clone() for k, t in case.items()}), outputs)  # the copy to the host synchronises
        pe.check_guards()
    assert snap, "assert_replays: the call returned no output to compare"
    return snap


def assert_replays(call, case_a, case_b, outputs=None, differ=(), patterns=PATTERNS):
    """`case_a`, `case_b`: dicts of input tensors with the same keys, shapes and dtypes, both valid inputs of the unit; B is the decoy the
    graph is captured on.  `outputs`: the names to compare (all by default).  `differ`: names of outputs -- the totals that cleared counters
    feed -- that must differ between the eager runs of A and B (VacuousCases otherwise; the eager runs must differ somewhere in any case).
    For each pattern of `patterns`, in order and only after the one before matched: capture call(static inputs holding B) under
    PoisonedEmpty(pattern) on one side stream, then rewrite the static inputs in place to A, B, B, A and replay after each; every output is
    compared with the eager run of the same case as raw bytes, to its capacity, and the guards are checked (ReplayMismatch, poison.GuardError).
    Returns (snapshot of A, snapshot of B, number of replays that matched)."""
    assert case_a.keys() == case_b.keys(), "the two cases name different inputs"
    for k in case_a:
        assert case_a[k].shape == case_b[k].shape and case_a[k].dtype == case_b[k].dtype and case_a[k].device == case_b[k].device, \
            f"input {k}: the two cases differ in shape, dtype or device"
    device = next(iter(case_a.values())).device
    base = {"A": _eager(call, case_a, outputs), "B": _eager(call, case_b, outputs)}
    if poison._first_difference(base["A"], base["B"]) is None:
        raise VacuousCases("the eager runs of the two cases are equal in every output")
    for name in differ:
        if poison._first_difference({name: base["A"][name]}, {name: base["B"][name]}) is None:
            raise VacuousCases(f"output {name} is the same for both cases")
    cases = {"A": case_a, "B": case_b}
    replays = 0
    for pattern in patterns:
        static = {k: t.clone() for k, t in case_b.items()}
        replay, out, pe = _capture(call, static, pattern, device)
        for i, which in enumerate(SEQUENCE):
            for k, t in static.items():
                t.copy_(cases[which][k])
            replay()
            diff = poison._first_difference(base[which], poison._snapshot(out, outputs))
            if diff:
                raise ReplayMismatch(f"replay {i + 1} of {len(SEQUENCE)} (inputs {which}, captured on B, poison {pattern} = "
                                     f"{poison.PATTERNS[pattern]:#010x}) differs from the eager run -- {diff}")
            pe.check_guards()
            replays += 1
        del replay, out, pe, static
    return base["A"], base["B"], replays


# ---- positive controls: three fake units in plain torch that the harness must reject, and the honest one it must pass ----------------------
def honest_unit(inputs):
    x = inputs["x"]
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    total = torch.empty((1,), dtype=torch.int64, device=x.device)
    torch.mul(x, 2, out=out)
    torch.sum(x > 0, dim=0, keepdim=True, out=total)
    return {"out": out, "total": total}


def host_value_unit(decoy_count):
    """Zeroes `out` behind a count that it works out on the host: right in every eager run; a graph holds the count of the inputs it was
    captured on.  (A read-back inside a device capture is an error of its own, so there the unit uses the count its last eager run read,
    which the harness made on the same decoy; the tape of the CPU path records the read-back itself.)  `decoy_count`: the count of the
    decoy B, which the unit must hold at the capture -- were the harness to order its eager runs otherwise, the control would be rejected
    for holding A's count on B's graph, the wrong reason, and this says so first."""
    state = {}

    def unit(inputs):
        x = inputs["x"]
        out = honest_unit(inputs)
        if not (x.is_cuda and torch.cuda.is_current_stream_capturing()):
            state["n"] = int((x > 0).sum().item())
        else:
            assert state.get("n") == decoy_count, f"the control holds the count {state.get('n')} at the capture, not the decoy's {decoy_count}"
        out["out"][state["n"]:].zero_()
        return out
    return unit


def unwritten_tail_unit(inputs):
    """Leaves the last element of `out` as it found it."""
    x = inputs["x"]
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    total = torch.empty((1,), dtype=torch.int64, device=x.device)
    torch.mul(x[:-1], 2, out=out[:-1])
    torch.sum(x > 0, dim=0, keepdim=True, out=total)
    return {"out": out, "total": total}


def other_stream_unit(other):
    """Does the second half of its work on `other`, a stream that is not capturing: that half runs at once, on what the inputs hold at the
    capture, and is missing from the graph.  Device only.  No event and no fork: the capture never sees the other stream."""
    def unit(inputs):
        x = inputs["x"]
        half = x.shape[0] // 2
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        total = torch.empty((1,), dtype=torch.int64, device=x.device)
        torch.mul(x[:half], 2, out=out[:half])
        with torch.cuda.stream(other):
            torch.mul(x[half:], 2, out=out[half:])
        torch.sum(x > 0, dim=0, keepdim=True, out=total)
        return {"out": out, "total": total}
    return unit


def control_cases(device):
    a = torch.arange(-3, 13, dtype=torch.int32, device=device)  # 12 positive
    b = torch.arange(-9, 7, dtype=torch.int32, device=device)   # 6 positive
    return {"x": a}, {"x": b}
