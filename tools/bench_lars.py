#!/usr/bin/env python3
"""FusedLARS against FusedSGDMomentum, same box, interleaved. Run on a GPU box.

  python tools/bench_lars.py kernel
      The optimizer launches alone on the flat buffers of a mixed-bf16
      ResNet-34 (a bf16 group with fp32 masters and the fp32 BN group), HIP
      events around --iters back-to-back steps: `sgd_step` (2 launches)
      against LARS (2 norms + 1 fold + 2 step launches), in --repeats
      interleaved windows sgd, lars, sgd'. The two sgd windows are an A/A
      pair: their spread is the box's noise. Then each LARS phase alone
      (norms, fold, step), which is where the fold kernel's own time comes
      from. Bytes per bf16 element: sgd_step 20, LARS 26 (ratio 1.30).

  python tools/bench_lars.py step
      The whole eager ResNet-34 224^2 bs96 bf16 step (forward, loss,
      backward, optimizer) with `momentum` against `lars`, wall clock around
      --rounds interleaved windows, each ending in a device synchronize.
"""

import argparse
import copy
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fluxdistributed_amd.models import build_model  # noqa: E402
from fluxdistributed_amd.ops import (  # noqa: E402
    FusedLARS, FusedSGDMomentum, logit_cross_entropy,
)
from fluxdistributed_amd.ops.native import require_native  # noqa: E402
from fluxdistributed_amd.utils.precision import to_mixed_bf16  # noqa: E402

CL = torch.channels_last
DEV = "cuda:0"


def make(model, kind):
    m = copy.deepcopy(model)
    if kind == "lars":
        return m, FusedLARS(m.parameters(), lr=0.01, momentum=0.9,
                            max_grad_norm=10.0)
    return m, FusedSGDMomentum(m.parameters(), lr=0.01, momentum=0.9)


def event_time(fn, iters):
    """Mean device milliseconds per call over `iters` back-to-back calls."""
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def fmt(ts):
    return (f"{statistics.median(ts) * 1e3:8.1f} "
            f"[{min(ts) * 1e3:7.1f}..{max(ts) * 1e3:7.1f}]")


def bench_kernel(args):
    C = require_native("lars")
    torch.manual_seed(0)
    model = to_mixed_bf16(build_model(args.model, num_classes=1000)
                          .to(DEV).to(memory_format=CL))
    (_, sgd), (_, lars) = make(model, "momentum"), make(model, "lars")
    for opt in (sgd, lars):
        for g in opt.groups:
            g.G.copy_(torch.randn(g.numel, device=DEV) * 1e-3)
    n = {str(g.dtype): g.numel for g in lars.groups}
    plan = lars._plan
    print(f"# {args.model} flat layout {n}, {plan.S} segments, "
          f"{plan.total_chunks} chunks of <= {C.LARS_CHUNK}; device us per "
          f"optimizer step: median [min..max] of {args.repeats} interleaved "
          f"windows x {args.iters} steps")
    arms = {"sgd": sgd.step, "lars": lars.step, "sgd'": sgd.step}
    for fn in arms.values():
        for _ in range(10):
            fn()
    ts = {k: [] for k in arms}
    for _ in range(args.repeats):
        for k, fn in arms.items():
            ts[k].append(event_time(fn, args.iters))
    for k in arms:
        print(f"{k:5s} {fmt(ts[k])} us")
    med = {k: statistics.median(v) for k, v in ts.items()}
    aa = abs(med["sgd"] - med["sgd'"]) / min(med["sgd"], med["sgd'"])
    base = 0.5 * (med["sgd"] + med["sgd'"])
    print(f"lars / sgd = {med['lars'] / base:.3f}   "
          f"(A/A spread of the sgd windows: {aa * 100:.2f} %; byte ratio 1.30)")
    assert lars.skipped_steps() == 0

    hp = lars.param_groups[0]
    master = lambda g: g.master if g.master is not None else g.P  # noqa: E731

    def norms():
        for g, t, cb in zip(lars.groups, plan.tables, plan.chunk_bases):
            C.lars_norms(g.P, g.G, master(g), t, plan.partials, cb,
                         plan.total_chunks, plan.S)

    def fold():
        C.lars_fold(plan.partials, plan.seg_meta, lars._lr_t, plan.coef,
                    plan.stats, lars._skipped, hp["eta"], hp["weight_decay"],
                    hp["eps"], hp["max_grad_norm"])

    def step():
        for g, t in zip(lars.groups, plan.tables):
            C.lars_step(g.P, g.G, master(g), g.V, t, plan.seg_meta, plan.coef,
                        plan.stats, hp["momentum"], hp["weight_decay"])

    phases = {"norms": norms, "fold": fold, "step": step}
    ps = {k: [] for k in phases}
    for _ in range(args.repeats):
        for k, fn in phases.items():
            ps[k].append(event_time(fn, args.iters))
    print("# LARS phases alone, back to back (launch gaps included)")
    for k in phases:
        print(f"{k:5s} {fmt(ps[k])} us")


def bench_step(args):
    torch.manual_seed(0)
    model = to_mixed_bf16(build_model(args.model, num_classes=1000)
                          .to(DEV).to(memory_format=CL)).train()
    kinds = ("momentum", "lars", "momentum'")
    runs = {k: make(model, k.rstrip("'")) for k in kinds}
    x = torch.randn(args.batch, 3, args.image, args.image, device=DEV) \
        .bfloat16().contiguous(memory_format=CL)
    y = torch.randint(0, 1000, (args.batch,), device=DEV)

    def run(kind, steps):
        m, opt = runs[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = logit_cross_entropy(m(x), y)
            opt.zero_grad()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    for k in kinds:
        run(k, args.warmup)
    per = max(1, args.steps // args.rounds)
    wall = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k in kinds:
            wall[k].append(run(k, per))
    print(f"# {args.model} {args.image}^2 bf16 batch {args.batch}, eager "
          f"step: {args.rounds} interleaved windows x {per} steps after "
          f"{args.warmup} warm-up steps; ms per step: median [min..max]")
    for k in kinds:
        ms = [t * 1e3 for t in wall[k]]
        med = statistics.median(ms)
        print(f"{k:10s} {med:8.3f} [{min(ms):8.3f}..{max(ms):8.3f}] "
              f"{args.batch / med * 1e3:9.1f} images/s")
    med = {k: statistics.median(wall[k]) for k in kinds}
    base = 0.5 * (med["momentum"] + med["momentum'"])
    aa = abs(med["momentum"] - med["momentum'"]) / base
    print(f"lars - momentum: {(med['lars'] - base) * 1e3:+.3f} ms per step "
          f"({(med['lars'] / base - 1) * 100:+.2f} %; A/A spread "
          f"{aa * 100:.2f} %)")
    assert runs["lars"][1].skipped_steps() == 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["step", "kernel"])
    p.add_argument("--model", default="resnet34")
    p.add_argument("--batch", type=int, default=96)
    p.add_argument("--image", type=int, default=224)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--steps", type=int, default=40, help="timed steps per arm")
    p.add_argument("--rounds", type=int, default=4,
                   help="interleaved windows the timed steps are split into")
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--repeats", type=int, default=7)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    (bench_step if args.mode == "step" else bench_kernel)(args)


if __name__ == "__main__":
    main()
