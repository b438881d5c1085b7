"""Bucketed gradient all-reduce overlapped with backward.

Replaces the reference's entire comm protocol (S1-S3 in SURVEY.md §2.5:
leaf-wise P2P copies into one HOST GPU + serial fold-reduce + scatter back)
with RCCL all-reduce over xGMI launched as soon as each bucket's gradients
are complete during backward.

MI355X sizing: 8 GPUs are fully connected by 7 point-to-point xGMI links
(≈153 GB/s each); ring collectives are per-link bound, so buckets must be
large enough to amortize per-collective latency but small enough to overlap
with the remaining backward — default 25 MB. The ~110 ResNet leaf tensors
are never sent as 110 messages: gradients live in ONE flat buffer (the
fused optimizer's G), and buckets are contiguous slices of it — zero
packing copies.
"""

import os
import threading
from typing import List

import torch
import torch.distributed as dist

from ..ops.fused_optim import _FlatOptimizer
from ..ops.step_state import subscribe_grad_written, unsubscribe_grad_written


class GradBucketer:
    """Slices a flat gradient buffer into buckets keyed to parameters and
    all-reduces each bucket when its last gradient lands during backward.

    Launch order is fixed (reverse parameter order ≈ backward completion
    order) and enforced identically on every rank: a bucket whose grads
    complete early is not launched until all its predecessors have been.
    """

    def __init__(
        self,
        optimizer: _FlatOptimizer,
        process_group=None,
        bucket_cap_mb: float = 25.0,
        average: bool = True,
    ):
        self.pg = process_group
        self.average = average
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        # FLUXDIST_DDP_FORCE=1: launch the collectives even at world 1.
        # RCCL 2.26 refuses two ranks of one communicator on one GPU
        # ("Duplicate GPU detected", tools/rccl_probe.py), so this is how
        # the async stream-ordered RCCL branch (in-flight works, bucket
        # launch order, wait ordering) is exercised inside a 1-GPU lease:
        # a 1-rank all_reduce runs real RCCL kernels and is the identity.
        self.force = os.environ.get("FLUXDIST_DDP_FORCE", "0") == "1"
        self._active = (self.world > 1) or (self.force and dist.is_initialized())
        self.buckets: List[dict] = []
        self._build(optimizer, bucket_cap_mb)
        self._works: List = []
        self._next_launch = 0
        self._lock = threading.Lock()   # notify may fire from engine threads

    def _build(self, optimizer: _FlatOptimizer, cap_mb: float):
        cap = int(cap_mb * 1e6)
        for g in optimizer.groups:
            elt = g.P.element_size()
            # reverse order: last registered params get grads first in backward
            order = list(range(len(g.params)))[::-1]
            cur_params, cur_lo, cur_hi, cur_bytes = [], None, None, 0
            def flush():
                nonlocal cur_params, cur_lo, cur_hi, cur_bytes
                if cur_params:
                    self.buckets.append(dict(
                        flat=g.G, lo=cur_lo, hi=cur_hi,
                        params=set(cur_params), pending=len(cur_params),
                        seen=set(),
                    ))
                cur_params, cur_lo, cur_hi, cur_bytes = [], None, None, 0
            for idx in order:
                p = g.params[idx]
                off = g.offsets[idx]
                n = p.numel()
                if cur_bytes and cur_bytes + n * elt > cap:
                    flush()
                cur_params.append(p)
                lo, hi = off, off + n
                cur_lo = lo if cur_lo is None else min(cur_lo, lo)
                cur_hi = hi if cur_hi is None else max(cur_hi, hi)
                cur_bytes += n * elt
            flush()
        self._param2bucket = {}
        for bi, b in enumerate(self.buckets):
            for p in b["params"]:
                self._param2bucket[id(p)] = bi
        self._ready = [False] * len(self.buckets)

    def attach(self):
        """Install post-accumulate-grad hooks on every bucketed parameter
        and subscribe to direct-grad notifications."""
        self._handles = []
        for b in self.buckets:
            for p in b["params"]:
                h = p.register_post_accumulate_grad_hook(self._on_grad)
                self._handles.append(h)
        subscribe_grad_written(self._on_direct)

    def detach(self):
        for h in getattr(self, "_handles", []):
            h.remove()
        self._handles = []
        unsubscribe_grad_written(self._on_direct)

    def _on_direct(self, p):
        if id(p) in self._param2bucket:
            self._on_grad(p)

    def _on_grad(self, p):
        bi = self._param2bucket[id(p)]
        b = self.buckets[bi]
        # Idempotent per step: a direct-grad param fires BOTH our notify AND
        # the post-accumulate hook (the engine still runs AccumulateGrad for
        # a None grad). Double-counting launched buckets early and the late
        # gradients were never all-reduced (caught by the 2-rank GPU test).
        if id(p) in b["seen"]:
            return
        b["seen"].add(id(p))
        b["pending"] -= 1
        if b["pending"] == 0:
            self._ready[bi] = True
            self._launch_ready()

    def _launch_ready(self):
        with self._lock:
            self._launch_ready_locked()

    def _launch_ready_locked(self):
        while self._next_launch < len(self.buckets) and self._ready[self._next_launch]:
            b = self.buckets[self._next_launch]
            if self._active:
                seg = b["flat"][b["lo"]:b["hi"]]
                if seg.is_cuda and dist.get_backend(self.pg) == "gloo":
                    # gloo's async CUDA collectives stage through host
                    # buffers that race when several are in flight
                    # (replica divergence measured in the 2-rank GPU
                    # test); run them synchronously — gloo is only the
                    # fallback transport, RCCL below keeps true overlap.
                    torch.cuda.current_stream(seg.device).synchronize()
                    dist.all_reduce(seg, op=dist.ReduceOp.SUM, group=self.pg)
                else:
                    self._works.append(
                        dist.all_reduce(seg, op=dist.ReduceOp.SUM,
                                        group=self.pg, async_op=True)
                    )
            self._next_launch += 1

    def finalize(self):
        """Wait for all in-flight collectives; average; reset for next step.

        Call after `loss.backward()` and before `optimizer.step()`.
        """
        # any bucket whose hooks never fired (frozen params) launches now
        for bi in range(self._next_launch, len(self.buckets)):
            self._ready[bi] = True
        self._launch_ready()
        for w in self._works:
            w.wait()
        self._works = []
        if self.average and self.world > 1:
            for b in self.buckets:
                b["flat"][b["lo"]:b["hi"]].div_(self.world)
        for bi, b in enumerate(self.buckets):
            b["pending"] = len(b["params"])
            b["seen"] = set()
            self._ready[bi] = False
        self._next_launch = 0

    def allreduce_now(self):
        """One-shot (non-overlapped) all-reduce of every flat grad buffer —
        used when hooks are unavailable (e.g. inside a hipGraph capture)."""
        if not self._active:
            return
        flats = {id(b["flat"]): b["flat"] for b in self.buckets}
        if any(f.is_cuda for f in flats.values()) \
                and dist.get_backend(self.pg) == "gloo":
            torch.cuda.synchronize()
        works = [dist.all_reduce(f, op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
                 for f in flats.values()]
        for w in works:
            w.wait()
        if self.average:
            for f in flats.values():
                f.div_(self.world)
        for bi, b in enumerate(self.buckets):
            b["pending"] = len(b["params"])
            b["seen"] = set()
            self._ready[bi] = False
        self._next_launch = 0
