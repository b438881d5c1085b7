"""Flat gradient sync for task-DDP: the replicas' gradients become their mean
in one streaming kernel per dtype group, in place, with no buffer tree.

Every replica's gradients already sit in one contiguous flat `G` per
(device, dtype) group (ops/fused_optim.py), so the exchange the tree protocol
spreads over ~110 leaves x (copy in, clone/add/div, copy out) is one launch
over R pointers. The definition, on every path:

    acc = G_0.float(); acc += G_1.float(); ...; acc += G_{R-1}.float()
    mean = (acc / R).to(dtype)          # one round, IEEE division
    G_i <- mean  for every i

i.e. a sequential fp32 sum in replica order. The tree protocol accumulates
in the parameter dtype instead, so for bf16 it rounds after every add.

Placement of the R buffers decides the path (per group):
- CPU / logical devices: torch math with the definition above;
- all on one GPU: one `grad_mean_multi` launch over the R `G`s;
- several GPUs (or `force_stage=True`): each replica that is not on the
  host (replica 0's device) owns one persistent staging row there; its `G`
  is copied in with one flat peer copy, one launch runs over the
  host-resident `G`s plus the rows, and each row is copied back.

BatchNorm running statistics are not gradients and stay per-replica.
"""

from typing import List

import torch

from ..ops.fused_optim import _FlatOptimizer
from ..ops.native import require_native
from ..utils.device import device_ctx, synchronize

MAX_REPLICAS = 16  # grad_mean_multi takes its pointers as kernel arguments


class _Group:
    """One dtype group across the replicas: the R flat G tensors, and for
    the staged path the host-side row of every remote replica."""

    def __init__(self, grads: List[torch.Tensor], force_stage: bool):
        self.grads = grads
        self.host = grads[0].device
        self.cpu = not grads[0].is_cuda
        self.stage = {}
        if self.cpu:
            return
        for i, g in enumerate(grads[1:], start=1):
            if force_stage or g.device != self.host:
                self.stage[i] = torch.zeros(
                    g.numel(), device=self.host, dtype=g.dtype)
        # what the kernel runs over: G itself where it lives on the host
        self.operands = [self.stage.get(i, g) for i, g in enumerate(grads)]


class FlatGradReducer:
    """Mean of the replicas' flat gradients, written back to every replica.

    `replicas` are task-DDP `Replica`s (anything with `.index` and
    `.optimizer`). `force_stage=True` treats replicas 1.. as remote even when
    they share replica 0's GPU, so the staged path runs on one GPU.
    """

    def __init__(self, replicas, force_stage: bool = False):
        replicas = list(replicas)
        if not 1 <= len(replicas) <= MAX_REPLICAS:
            raise ValueError(
                f"flat gradient sync takes 1..{MAX_REPLICAS} replicas, "
                f"got {len(replicas)}")
        layouts = []
        for r in replicas:
            if not isinstance(r.optimizer, _FlatOptimizer):
                raise ValueError(
                    f"replica {r.index}: flat gradient sync needs a flat "
                    f"optimizer (FusedSGDMomentum / FusedAdam), got "
                    f"{type(r.optimizer).__name__}")
            layouts.append([(g.dtype, g.numel) for g in r.optimizer.groups])
        for r, lay in zip(replicas, layouts):
            if lay != layouts[0]:
                raise ValueError(
                    f"replica {r.index}: flat group layout {lay} differs "
                    f"from replica {replicas[0].index}'s {layouts[0]}")
        self.force_stage = force_stage
        self.groups = [
            _Group([r.optimizer.groups[k].G for r in replicas], force_stage)
            for k in range(len(layouts[0]))
        ]
        # one non-finite flag per host GPU, set by the kernel
        self._flags = {}
        for grp in self.groups:
            if not grp.cpu and grp.host not in self._flags:
                self._flags[grp.host] = torch.zeros(
                    1, device=grp.host, dtype=torch.int32)
        self._cpu_nonfinite = False

    @torch.no_grad()
    def reduce(self) -> None:
        """Run once per step on the main thread, after every replica's
        backward has been synchronized."""
        for grp in self.groups:
            if grp.cpu:
                self._reduce_cpu(grp)
            else:
                self._reduce_gpu(grp)

    def _reduce_cpu(self, grp: _Group) -> None:
        acc = grp.grads[0].float().clone()
        for g in grp.grads[1:]:
            acc += g.float()
        mean = (acc / len(grp.grads)).to(grp.grads[0].dtype)
        if not bool(torch.isfinite(mean).all()):
            self._cpu_nonfinite = True
        for g in grp.grads:
            g.copy_(mean)

    def _reduce_gpu(self, grp: _Group) -> None:
        C = require_native("grad_mean_multi")
        with device_ctx(grp.host):
            for i, row in grp.stage.items():
                row.copy_(grp.grads[i], non_blocking=True)
            C.grad_mean_multi(grp.operands, self._flags[grp.host])
            for i, row in grp.stage.items():
                grp.grads[i].copy_(row, non_blocking=True)
        if grp.stage:
            synchronize(grp.host)

    def pop_nonfinite(self) -> bool:
        """True when a mean since the last call held an Inf/NaN; clears the
        record. Reads the device flag, which synchronizes."""
        bad = self._cpu_nonfinite
        self._cpu_nonfinite = False
        for flag in self._flags.values():
            if int(flag.item()):
                bad = True
                flag.zero_()
        return bad
