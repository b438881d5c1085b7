#!/usr/bin/env python3
"""Task-DDP gradient sync: the tree protocol against flat sync, same box,
interleaved. Run on a GPU box.

  python tools/bench_task_sync.py step
      ResNet-34, 224^2, bf16, FusedSGDMomentum as logical fan-out on cuda:0,
      global batch 96 (R=2 x 48 and R=4 x 24). Modes: tree, flat, flat with
      force_stage. Every mode takes --warmup steps, then the timed steps run
      in --rounds interleaved windows (tree, flat, stage, tree, flat, ...).
      Prints images/s from the wall clock around whole steps (each step ends
      in a device synchronize) and the StageTimers split per mode.

      The split is host time per stage. Only stages that end in a
      synchronize hold their device work: fwd_bwd and optimizer do,
      allreduce does not in tree and direct flat mode (its kernels drain
      inside the optimizer stage), so compare allreduce + optimizer.

  python tools/bench_task_sync.py kernel
      grad_mean_multi alone on R buffers of the ResNet-34 flat length, HIP
      events, against an aten copy_ chain that moves the same bytes (R reads
      + R writes of n elements): the yardstick for "HBM-bound".
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fluxdistributed_amd.models import build_model  # noqa: E402
from fluxdistributed_amd.ops import FusedSGDMomentum, logit_cross_entropy  # noqa: E402
from fluxdistributed_amd.ops.native import require_native  # noqa: E402
from fluxdistributed_amd.parallel import FlatGradReducer  # noqa: E402
from fluxdistributed_amd.parallel.task_ddp import prepare_training, train  # noqa: E402
from fluxdistributed_amd.utils.precision import to_mixed_bf16  # noqa: E402

CL = torch.channels_last
DEV = "cuda:0"
MODES = ("tree", "flat", "flat_stage")
STAGES = ("fwd_bwd", "allreduce", "optimizer")


def make_state(model, R, mode):
    st = prepare_training(
        model, None, [DEV] * R,
        lambda m: FusedSGDMomentum(m.parameters(), lr=0.01, momentum=0.9),
        grad_sync="tree" if mode == "tree" else "flat")
    if mode == "flat_stage":
        st.reducer = FlatGradReducer(st.replicas, force_stage=True)
    return st


def bench_step(args):
    torch.manual_seed(0)
    model = build_model(args.model, num_classes=1000)
    model = to_mixed_bf16(model.to(memory_format=CL)).train()
    for R in args.replicas:
        per = args.batch // R
        gen = torch.Generator().manual_seed(R)
        mbs = [(torch.randn(per, 3, args.image, args.image, generator=gen)
                .bfloat16().to(DEV).contiguous(memory_format=CL),
                torch.randint(0, 1000, (per,), generator=gen).to(DEV))
               for _ in range(R)]
        states = {m: make_state(model, R, m) for m in MODES}

        def run(mode, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train(logit_cross_entropy, states[mode], steps=steps,
                  batches=lambda j: mbs, log_every=0, val_every=0)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        for m in MODES:
            run(m, args.warmup)
            states[m].timers.reset()
        per_round = max(1, args.steps // args.rounds)
        wall = {m: [] for m in MODES}
        for _ in range(args.rounds):
            for m in MODES:
                wall[m].append(run(m, per_round) / per_round)

        print(f"# {args.model} {args.image}^2 bf16, R={R} x {per} images on "
              f"{DEV}: {args.rounds} interleaved windows x {per_round} steps "
              f"after {args.warmup} warm-up steps")
        print(f"{'mode':11s} {'step ms: median [min..max]':>30s} "
              f"{'images/s':>9s} " + " ".join(f"{s + ' ms':>13s}" for s in STAGES))
        for m in MODES:
            ms = [t * 1e3 for t in wall[m]]
            med = statistics.median(ms)
            split = states[m].timers.summary()
            print(f"{m:11s} {med:12.2f} [{min(ms):7.2f}..{max(ms):7.2f}] "
                  f"{R * per / med * 1e3:9.1f} "
                  + " ".join(f"{split[s]['mean_ms']:13.3f}" for s in STAGES))
        base = statistics.median(wall["tree"])
        for m in MODES[1:]:
            d = (base - statistics.median(wall[m])) * 1e3
            print(f"tree - {m}: {d:+.3f} ms per step")
        del states
        torch.cuda.empty_cache()


def event_time(fn, iters):
    """Mean device milliseconds per call over `iters` back-to-back calls."""
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def bench_kernel(args):
    C = require_native("grad_mean_multi")
    probe = build_model(args.model, num_classes=1000)
    n = sum((p.numel() + 63) // 64 * 64 for p in probe.parameters()
            if p.requires_grad)
    print(f"# grad_mean_multi over R flat bf16 buffers of n={n} elements "
          f"({args.model}), device ms per call: median [min..max] of "
          f"{args.repeats} interleaved repeats x {args.iters} calls")
    print(f"{'R':>2s} {'MB moved':>9s} {'kernel':>24s} {'GB/s':>7s} "
          f"{'copy_ chain':>24s} {'GB/s':>7s} {'kernel/copy':>11s}")
    for R in args.replicas:
        bufs = [torch.randn(n, device=DEV).bfloat16() for _ in range(R)]
        dsts = [torch.empty_like(b) for b in bufs]
        flag = torch.zeros(1, device=DEV, dtype=torch.int32)

        def kernel():
            C.grad_mean_multi(bufs, flag)

        def copies():
            for d, s in zip(dsts, bufs):
                d.copy_(s)

        arms = {"kernel": kernel, "copy": copies}
        for fn in arms.values():
            for _ in range(10):
                fn()
        ts = {k: [] for k in arms}
        for _ in range(args.repeats):
            for k, fn in arms.items():
                ts[k].append(event_time(fn, args.iters))
        nbytes = 2 * R * n * 2          # R reads + R writes, 2 B each
        cols = []
        for k in ("kernel", "copy"):
            med = statistics.median(ts[k])
            cols.append(f"{med:9.4f} [{min(ts[k]):6.4f}..{max(ts[k]):6.4f}] "
                        f"{nbytes / med / 1e6:7.0f}")
        ratio = statistics.median(ts["kernel"]) / statistics.median(ts["copy"])
        print(f"{R:2d} {nbytes / 1e6:9.1f} {cols[0]} {cols[1]} {ratio:11.2f}")
        assert int(flag.item()) == 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["step", "kernel"])
    p.add_argument("--model", default="resnet34")
    p.add_argument("--batch", type=int, default=96, help="global batch")
    p.add_argument("--replicas", type=int, nargs="+", default=[2, 4])
    p.add_argument("--image", type=int, default=224)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--steps", type=int, default=20, help="timed steps per mode")
    p.add_argument("--rounds", type=int, default=4,
                   help="interleaved windows the timed steps are split into")
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--repeats", type=int, default=5)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    (bench_step if args.mode == "step" else bench_kernel)(args)


if __name__ == "__main__":
    main()
