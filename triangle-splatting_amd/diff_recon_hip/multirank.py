"""Image-parallel training across ranks, end to end, with a guard that proves the replicas are still bit-identical.

Every rank holds the whole model (parameters, Adam moments, densification statistics), renders its share of a step's views, and the ranks
exchange what the one-process loop would have summed: the parameter gradients (SUM over the views, like the one-process loop -- not the mean:
the two must be the same algorithm) and the per-view statistics (all-gathered, rank order = view order).  Everything after the exchange is
replicated arithmetic on identical inputs, so the replicas must stay identical down to the last bit -- through every densification, pruning,
clipping and reset.  Replicas that drift do not crash: they differ by one ulp in one gradient, then by one triangle in one pruning decision,
and the next collective hangs or mixes rows.  `ReplicaGuard` turns that into an exception on every rank at the step where it happens.

    state_digest(named)            one 64-bit order-independent digest per tensor, on the device, ONE launch (include/ts_model.h: tsm_state_digest)
    state_digest_reference(named)  the numpy restatement of the digest's definition: host only, for tests
    ReplicaGuard                   digests + row count -> one all-gather -> ReplicaDivergence on every rank
    ImageParallelLoop              shard the views, backward, exchange ("dense" | "factored_sh"), FusedAdam, statistics of ALL views, structural
                                   rules, guard

Out of scope here: ShardedAdam inside this loop, RCCL tuning, the delayed exchange, graph replay of the multi-rank step.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist

from diff_triangle_rasterization_2D import _C as _native
from diff_triangle_rasterization_2D.parallel import (FactoredShExchange, GradBucket, ShGradSink, all_reduce_triangle_grads, factored_sh_grads,
                                                     shard_views)
from .model_update import _PARAM_GROUPS, _STATE, run_model_update

_lib = _native._lib

MAX_DIGEST_SEGMENTS = 32  # TSM_DIGEST_MAX_SEGMENTS, include/ts_model.h

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def _words_or_raise(name, t: torch.Tensor) -> int:
    if not t.is_contiguous():
        raise ValueError(f"state digest: {name!r} is not contiguous")
    nbytes = t.numel() * t.element_size()
    if nbytes % 4:
        raise ValueError(f"state digest: {name!r} holds {nbytes} bytes, not a multiple of 4")
    return nbytes // 4


def digest_segments(tensors: Sequence[torch.Tensor], names: Optional[Sequence[str]] = None) -> torch.Tensor:
    """ONE tsm_state_digest call over `tensors` (at most MAX_DIGEST_SEGMENTS; more is the library's error): int64 (len(tensors),) on their
    device, queued on the current stream, no host synchronisation."""
    n = len(tensors)
    if n == 0:
        raise ValueError("state digest: no tensors")
    names = list(names) if names is not None else [str(i) for i in range(n)]
    dev = tensors[0].device
    words = []
    for name, t in zip(names, tensors):
        _native.require_device("state_digest", t)
        if t.device != dev:
            raise ValueError(f"state digest: {name!r} lives on {t.device}, the others on {dev}")
        words.append(_words_or_raise(name, t))
    out = torch.empty((n,), device=dev, dtype=torch.int64)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() if w else None for t, w in zip(tensors, words)])
    counts = (C.c_uint64 * n)(*words)
    with torch.cuda.device(dev):
        _native._check(_lib.tsm_state_digest(n, ptrs, counts, out.data_ptr(), _native.stream()), "state_digest")
    return out


def state_digest(named: Dict[str, torch.Tensor]) -> torch.Tensor:
    """One order-independent 64-bit digest per entry of `named` (its order), as int64 on the device; no host synchronisation.  Bit patterns
    count (-0.0 differs from 0.0, NaN payloads are distinguished).  Equal on two ranks iff -- up to a 64-bit hash collision -- the tensors hold
    the same bits.  Non-contiguous tensors and byte sizes that are no multiple of 4 raise ValueError."""
    names, tensors = list(named.keys()), [t.detach() for t in named.values()]
    if len(tensors) <= MAX_DIGEST_SEGMENTS:
        return digest_segments(tensors, names)
    return torch.cat([digest_segments(tensors[i:i + MAX_DIGEST_SEGMENTS], names[i:i + MAX_DIGEST_SEGMENTS])
                      for i in range(0, len(tensors), MAX_DIGEST_SEGMENTS)])


def _digest_words(w: np.ndarray) -> int:
    """sum_j mix64(x_j ^ (j + 1) GOLDEN) mod 2^64 over the 64-bit pairs x_j = w[2j] | w[2j+1] << 32 of the uint32 words `w`."""
    if w.size == 0:
        return 0
    if w.size & 1:
        w = np.concatenate([w, np.zeros(1, np.uint32)])
    x = w[0::2].astype(np.uint64) | (w[1::2].astype(np.uint64) << np.uint64(32))
    z = x ^ (np.arange(1, x.size + 1, dtype=np.uint64) * _GOLDEN)  # array arithmetic on uint64 wraps mod 2^64
    z ^= z >> np.uint64(30)
    z *= _M1
    z ^= z >> np.uint64(27)
    z *= _M2
    z ^= z >> np.uint64(31)
    return int(z.sum(dtype=np.uint64))


def state_digest_reference(named: Dict[str, torch.Tensor]) -> torch.Tensor:
    """The definition of the digest (include/ts_model.h) restated with numpy on the host: int64 (len(named),) on the CPU.  For tests; the
    training loop never calls it."""
    out = []
    for name, t in named.items():
        t = t.detach()
        _words_or_raise(name, t)
        w = np.frombuffer(t.cpu().reshape(-1).numpy().tobytes(), dtype="<u4")  # raw bytes: no value conversion on the way
        out.append(_digest_words(w))
    return torch.from_numpy(np.array(out, dtype=np.uint64).view(np.int64).copy()) if out else torch.zeros((0,), dtype=torch.int64)


def _world(group) -> int:
    return dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1


def _rank(group) -> int:
    return dist.get_rank(group) if (dist.is_available() and dist.is_initialized()) else 0


class ReplicaDivergence(RuntimeError):
    """The replicas of the model no longer hold the same bits.  `iteration`; `names`: the entries whose digests differ between ranks
    ("num_rows" when the triangle counts do); `ranks`: the ranks that disagree with rank 0.  Raised on every rank of the group."""

    def __init__(self, iteration: int, names: List[str], ranks: List[int]):
        self.iteration, self.names, self.ranks = int(iteration), list(names), list(ranks)
        super().__init__(f"replicas diverged at iteration {iteration}: {', '.join(names)} differ(s) on rank(s) {ranks} from rank 0")


class ReplicaGuard:
    """Proves, while training, that the ranks' replicated state is bit-identical.

    check(iteration, named, num_rows, force=False): every `every` iterations and whenever `force`, digest `named` on the device, append
    `num_rows`, all-gather that small int64 vector and compare: ONE collective and ONE host read per check.  Nothing at all on the other
    iterations, and nothing in a world of one rank.  `force` must be decided identically on every rank (the loop forces a check after a step
    in which a structural rule fired, which depends on the iteration number alone).  `digest_fn` defaults to `state_digest`; the CPU tests of
    the protocol inject `state_digest_reference`."""

    def __init__(self, group=None, every: int = 50, digest_fn: Optional[Callable[[Dict[str, torch.Tensor]], torch.Tensor]] = None):
        if every < 1:
            raise ValueError("ReplicaGuard: every must be >= 1")
        self.group, self.every = group, int(every)
        self.digest_fn = digest_fn if digest_fn is not None else state_digest
        self.checks = 0

    def due(self, iteration: int, force: bool = False) -> bool:
        return _world(self.group) > 1 and (force or iteration % self.every == 0)

    def check(self, iteration: int, named: Dict[str, torch.Tensor], num_rows: int, force: bool = False) -> bool:
        """True when a check ran (and passed); raises ReplicaDivergence on every rank otherwise."""
        if not self.due(iteration, force):
            return False
        world = _world(self.group)
        names = list(named.keys())
        digests = self.digest_fn(named)
        mine = torch.cat([digests, torch.full((1,), int(num_rows), device=digests.device, dtype=torch.int64)])
        everyone = torch.empty((world * mine.numel(),), device=mine.device, dtype=torch.int64)
        dist.all_gather_into_tensor(everyone, mine, group=self.group)
        table = everyone.view(world, -1).cpu()  # the one host read
        self.checks += 1
        differs = table != table[0:1]
        if bool(differs.any()):
            cols = differs.any(dim=0).tolist()
            bad = [n for n, d in zip(names + ["num_rows"], cols) if d]
            raise ReplicaDivergence(iteration, bad, [r for r in range(world) if bool(differs[r].any())])
        return True


def replicated_state(model) -> Dict[str, torch.Tensor]:
    """What must be identical on every rank: every parameter of the model's optimizer with both of its Adam moments (once they exist) and the
    six densification statistics.  The triangle count travels beside the digests (ReplicaGuard.check: num_rows)."""
    named: Dict[str, torch.Tensor] = {}
    for gi, group in enumerate(model.optimizer.param_groups):
        for pi, p in enumerate(group["params"]):
            name = group.get("name", f"group{gi}") + (f".{pi}" if len(group["params"]) > 1 else "")
            named[name] = p.data
            st = model.optimizer.state.get(p)
            if st:
                named[name + ".exp_avg"], named[name + ".exp_avg_sq"] = st["exp_avg"], st["exp_avg_sq"]
    for name in _STATE:
        named[name] = getattr(model, name)
    return named


class ImageParallelLoop:
    """One optimisation step of image-parallel training.

        loop = ImageParallelLoop(model, render_and_loss, group=None, exchange="dense", guard=ReplicaGuard(every=50))
        loss = loop.step(iteration, views)          # `views`: the step's WHOLE view list, the same on every rank

    `model` carries what the structural rules need (diff_recon_hip.model_update: `_vertex / _opacity / _f_dc + _f_rest | _shs`, `optimizer` = a
    replicated FusedAdam with named groups, DensificationStats, `active_sh_degree`, `max_sh_degree`, `config.model_update`).
    `render_and_loss(view) -> (loss, render_pkg)` renders one view with the model's parameters.  The rank renders
    `shard_views(len(views), rank, world)`, backpropagates, and then
      * "dense": sums the parameter gradients over the ranks (one flat bucket, one collective);
      * "factored_sh": vertex and opacity as above; the backward passes run under `factored_sh_grads`, the factors (dL_dRGB, camera centre)
        of every rank's views travel through `FactoredShExchange` and the dense dL_dshs rebuilt locally from ALL of them becomes the colour
        parameters' `.grad` (split into f_dc / f_rest when the model carries two tensors).  The colour parameters must reach the rasterizer
        without an operation that changes their gradient (ShFactors' condition);
      * steps the model's own FusedAdam on every rank;
      * applies the statistics of ALL views on every rank and then the structural rules (`model_update(iteration, pkgs) -> fired rules`;
        default: run_model_update with all_views=True);
      * runs the guard over replicated_state(model) and the triangle count -- forced after a step in which a rule fired;
      * returns the step's loss summed over the ranks, on the device.
    No host synchronisation of its own outside guard checks."""

    def __init__(self, model, render_and_loss: Callable, group=None, exchange: str = "dense", guard: Optional[ReplicaGuard] = None,
                 model_update: Optional[Callable[[int, list], list]] = None):
        if exchange not in ("dense", "factored_sh"):
            raise ValueError(f"ImageParallelLoop: exchange must be 'dense' or 'factored_sh', not {exchange!r}")
        self.model, self.render_and_loss, self.group, self.exchange, self.guard = model, render_and_loss, group, exchange, guard
        self.world, self.rank = _world(group), _rank(group)
        self.model_update = model_update if model_update is not None else (
            lambda iteration, pkgs: run_model_update(self.model, iteration, pkgs, all_views=True, group=self.group))
        self._bucket: Optional[GradBucket] = None
        self._shx: Optional[FactoredShExchange] = None

    def _params(self) -> List[torch.Tensor]:
        return [p for g in self.model.optimizer.param_groups if g.get("name") in _PARAM_GROUPS for p in g["params"]]

    def _colour(self) -> List[torch.Tensor]:
        m = self.model
        return [m._shs] if getattr(m, "single_sh", False) or not hasattr(m, "_f_dc") else [m._f_dc, m._f_rest]

    def _reduce(self, params: List[torch.Tensor]):
        if self.world == 1:
            return
        for p in params:
            if p.grad is None:  # no view of this rank reached it: it still takes part in the sum
                p.grad = torch.zeros_like(p)
        shapes = [p.shape for p in params]
        if self._bucket is None or self._bucket.shapes != [torch.Size(s) for s in shapes]:  # the triangle count changed: a new flat buffer
            self._bucket = GradBucket(shapes, params[0].device, params[0].dtype, self.group, mean=False)
        all_reduce_triangle_grads(params, self.group, mean=False, bucket=self._bucket)

    def step(self, iteration: int, views: Sequence) -> torch.Tensor:
        m = self.model
        m.optimizer.zero_grad(set_to_none=True)
        factored = self.exchange == "factored_sh"
        sink = ShGradSink()
        pkgs, total = [], None
        for k in shard_views(len(views), self.rank, self.world):
            loss, pkg = self.render_and_loss(views[k])
            with factored_sh_grads(sink, enabled=factored):
                loss.backward()
            pkgs.append(pkg)
            total = loss.detach().clone() if total is None else total + loss.detach()
        if total is None:
            raise ValueError(f"ImageParallelLoop.step: rank {self.rank} of {self.world} got no view out of {len(views)}")
        colour = self._colour()
        if factored:
            vertex = m._vertex
            M = sum(c.shape[1] for c in colour)
            if self._shx is None:
                self._shx = FactoredShExchange(self.group, vertex.device)
            self._shx.start(sink, vertex.detach(), int(m.active_sh_degree), M, mean=False, uniform=True)
            self._reduce([p for p in self._params() if all(p is not c for c in colour)])
            dense = self._shx.wait()  # (P, M, 3): the sum over every view of every rank
            if len(colour) == 1:
                colour[0].grad = dense
            else:
                colour[0].grad, colour[1].grad = dense[:, :1].contiguous(), dense[:, 1:].contiguous()
        else:
            self._reduce(self._params())
        m.optimizer.step()
        fired = self.model_update(iteration, pkgs)
        if self.guard is not None and self.guard.due(iteration, force=bool(fired)):
            self.guard.check(iteration, replicated_state(m), m._vertex.shape[0], force=bool(fired))
        if self.world > 1:
            dist.all_reduce(total, op=dist.ReduceOp.SUM, group=self.group)
        return total
