"""Poisoned buffers for the purity tests (tests/test_purity_cpu.py, tests/test_purity_gpu.py; DESIGN.md "Purity of the entry points").

Every entry point of include/*.h works in caller-provided memory it must not trust: the result is a function of the documented inputs only,
every documented output is fully written, and no byte outside a declared extent is touched.  A fresh allocation reads as zeros and hides a
read of a slot that nobody wrote in this call; the helpers here hand the library buffers full of another pattern instead:

    PoisonedEmpty(pattern)           replaces torch.empty: what the Python wrappers allocate comes back filled and between two guard bands
    poison_blocks(sizes, pattern)    fills blocks of the caching allocator and frees them, for buffers the C++ extension allocates
    filled(shape, dtype, pattern)    one guarded, filled tensor for a direct C-ABI call (registered with the active PoisonedEmpty)
    assert_pure(call)                the harness: determinism on zeros first, then the patterns in a fixed order, raw-byte comparison
"""
from __future__ import annotations

import math

import torch

# 32-bit words, tiled little-endian from the first byte of a buffer
PATTERNS = {"zero": 0x00000000, "ones": 0x00000001, "float1": 0x3F800000, "nan": 0x7FC00000, "allbits": 0xFFFFFFFF}
# the order assert_pure tries them in: an in-range index / count first, a wild one last
ORDER = ("ones", "float1", "nan", "allbits")
GUARD = 512     # bytes either side; a multiple of 16, so the 16- and 8-byte alignment the fast paths test for is that of a plain allocation
CANARY = 0xA5   # no byte of any pattern


class GuardError(AssertionError):
    """A byte outside the extent of a poisoned tensor was written."""


class DeterminismError(AssertionError):
    """Two runs on zero-filled buffers disagree: not a poison finding."""


class PoisonLeak(AssertionError):
    """A documented output depends on what a workspace or an output held on entry."""


def pattern_bytes(pattern, nbytes, device="cpu"):
    """uint8 tensor of `nbytes` bytes: the pattern's word tiled from byte 0, the last word cut where the length is no multiple of 4."""
    word = PATTERNS[pattern]
    unit = torch.tensor(list(word.to_bytes(4, "little")), dtype=torch.uint8, device=device)
    return unit.repeat((nbytes + 3) // 4)[:nbytes]


def fill(t, pattern):
    """Fills the bytes of the contiguous tensor `t` with the pattern, in place; returns t.  Allocates nothing on the tensor's device (whole
    words by fill_, the odd tail byte by byte), so that it does not disturb an allocator whose free blocks a test is arranging."""
    assert t.is_contiguous()
    n = t.numel() * t.element_size()
    if n == 0:
        return t
    flat = t.reshape(-1).view(torch.uint8)
    word = PATTERNS[pattern]
    if flat.data_ptr() % 4:  # a view that starts off a word boundary: through a staging copy
        flat.copy_(pattern_bytes(pattern, n, t.device))
        return t
    n4 = n // 4
    if n4:
        flat[:4 * n4].view(torch.int32).fill_(word - (1 << 32) if word >= 1 << 31 else word)
    for i, b in enumerate(word.to_bytes(4, "little")[:n - 4 * n4]):
        flat[4 * n4 + i:4 * n4 + i + 1].fill_(b)
    return t


def raw(t):
    """The bytes of a tensor as a CPU uint8 tensor (NaN payloads and the sign of zero count)."""
    t = t.detach().contiguous().reshape(-1)
    return t.view(torch.uint8).cpu() if t.numel() else torch.zeros(0, dtype=torch.uint8)


_empty = torch.empty  # the real one, bound before any patch
_active = []          # the PoisonedEmpty contexts entered, innermost last


class PoisonedEmpty:
    """with PoisonedEmpty("nan") as pe: ...   torch.empty returns tensors filled with the pattern; each is a view into a parent allocation
    that carries GUARD bytes of CANARY before and after it.  pe.check_guards() asserts every canary intact."""

    def __init__(self, pattern):
        assert pattern in PATTERNS, pattern
        self.pattern = pattern
        self.records = []  # (parent, nbytes, shape, dtype)
        self._saved = None

    def __enter__(self):
        self._saved = torch.empty
        torch.empty = self._poisoned_empty
        _active.append(self)
        return self

    def __exit__(self, *exc):
        torch.empty = self._saved
        _active.remove(self)
        return False

    def allocate(self, shape, dtype=None, device=None):
        dtype = dtype or torch.get_default_dtype()
        shape = tuple(int(x) for x in shape)
        nbytes = math.prod(shape) * _empty((), dtype=dtype).element_size()
        parent = _empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device=device)
        parent.fill_(CANARY)
        body = fill(parent[GUARD:GUARD + nbytes], self.pattern)
        self.records.append((parent, nbytes, shape, dtype))
        return body.view(dtype).reshape(shape)

    def _poisoned_empty(self, *size, dtype=None, device=None, requires_grad=False, **kw):
        if kw.get("out") is not None or kw.get("layout", torch.strided) is not torch.strided or kw.get("pin_memory"):
            return _empty(*size, dtype=dtype, device=device, requires_grad=requires_grad, **kw)
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        t = self.allocate(size, dtype, device)
        return t.requires_grad_(True) if requires_grad else t

    def check_guards(self):
        for parent, nbytes, shape, dtype in self.records:
            for name, band, base in (("before", parent[:GUARD], -GUARD), ("after", parent[GUARD + nbytes:], nbytes)):
                bad = (band != CANARY).nonzero()
                if bad.numel():
                    first = int(bad[0]) + base
                    raise GuardError(f"{int(bad.numel())} guard bytes {name} a poisoned {dtype} tensor of shape {shape} ({nbytes} bytes, pattern "
                                     f"{self.pattern}) were written; the first at byte offset {first} from its start")


def filled(shape, dtype, pattern=None, device=None):
    """A guarded tensor filled with `pattern` (default: the active context's), registered with the innermost PoisonedEmpty so that its
    check_guards() covers it.  For buffers a test hands to the C ABI itself."""
    assert _active, "poison.filled needs an active PoisonedEmpty"
    pe = _active[-1]
    if isinstance(shape, int):
        shape = (shape,)
    t = pe.allocate(shape, dtype, device)
    if pattern is not None and pattern != pe.pattern:
        fill(t, pattern)
    return t


class PoisonedBlocks:
    def __init__(self, ptrs, pattern):
        self.ptrs, self.pattern = ptrs, pattern

    def assert_used(self, tensors):
        """Every non-empty tensor of `tensors` starts at a block that was poisoned: otherwise the test would pass vacuously."""
        for i, t in enumerate(tensors):
            if t.numel():
                assert t.data_ptr() in self.ptrs, (f"buffer {i} ({t.numel() * t.element_size()} bytes at {t.data_ptr():#x}) is not one of the "
                                                   f"{len(self.ptrs)} blocks poisoned with {self.pattern}")


def poison_blocks(byte_sizes, pattern, device="cuda"):
    """Allocates one uint8 tensor per entry of `byte_sizes` (zero sizes are left out), fills them with the pattern and frees them, so that the
    caching allocator hands the same blocks to the next requests of those sizes.  Returns the PoisonedBlocks holding their addresses."""
    blocks = [_empty(int(n), dtype=torch.uint8, device=device) for n in byte_sizes if int(n) > 0]  # all of them first, in the caller's order:
    for b in blocks:                                                                               # the requests that follow in the same
        fill(b, pattern)                                                                           # order then get the same blocks
    if blocks and blocks[0].is_cuda:
        torch.cuda.synchronize(blocks[0].device)
    held = PoisonedBlocks({b.data_ptr() for b in blocks}, pattern)
    del blocks
    return held


def _as_dict(out):
    if isinstance(out, dict):
        return out
    if isinstance(out, (tuple, list)):
        return {str(i): v for i, v in enumerate(out)}
    return {"0": out}


def _snapshot(out, names):
    d = _as_dict(out)
    return {k: (raw(v) if isinstance(v, torch.Tensor) else v) for k, v in d.items() if names is None or k in names}


def _first_difference(a, b):
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, torch.Tensor):
            if x.shape != y.shape:
                return f"{k}: {x.numel()} bytes against {y.numel()}"
            ne = (x != y).nonzero()
            if ne.numel():
                i = int(ne[0])
                return f"{k}: {int(ne.numel())} of {x.numel()} bytes differ, the first at byte {i} ({int(x[i]):#04x} against {int(y[i]):#04x})"
        elif x != y:
            return f"{k}: {x!r} against {y!r}"
    return None


def assert_pure(call, outputs=None, patterns=ORDER):
    """`call(pattern)` runs the operation once and returns its documented outputs (a tensor, a tuple or a dict of tensors and plain values);
    it runs inside PoisonedEmpty(pattern), so what it or the wrappers below it allocate with torch.empty or poison.filled is poisoned.
    `outputs`: the names (dict keys, or positions as strings) to compare; all by default.
    Twice on zeros (bit-equal, else DeterminismError), then `patterns` in order, each compared with the zero baseline as raw bytes; stops at
    the first difference (PoisonLeak).  Guards are checked after every run (GuardError).  Returns the baseline snapshot."""
    def run(pattern):
        with PoisonedEmpty(pattern) as pe:
            out = call(pattern)
            snap = _snapshot(out, outputs)  # the copy to the host synchronises
            pe.check_guards()
        return snap

    base = run("zero")
    assert base, "assert_pure: the call returned no output to compare"
    diff = _first_difference(base, run("zero"))
    if diff:
        raise DeterminismError(f"two runs on zero-filled buffers disagree -- {diff}")
    for pattern in patterns:
        diff = _first_difference(base, run(pattern))
        if diff:
            raise PoisonLeak(f"pattern {pattern} ({PATTERNS[pattern]:#010x}) changes the result -- {diff}")
    return base
