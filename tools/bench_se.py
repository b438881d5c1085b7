"""Time the squeeze-and-excitation kernels at the SE-ResNeXt-50 Bottleneck
shapes (batch 96), next to add_relu_fwd on a tensor of the same size.

  python tools/bench_se.py [--batch 96] [--iters 50] [--only C]

Prints, per shape, the device-event time of se_fwd (3 launches), se_bwd (4
launches) and add_relu_fwd, and the plan. Per-kernel times come from running
this under `rocprofv3 --kernel-trace --stats` with --only, one shape a run.
Bytes per pass (bf16, T = N*HW*C*2): squeeze reads T; scale fwd reads 2T and
writes T, like add_relu_fwd; bwd reduce reads 3T; bwd apply reads 2T and
writes 2T.
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluxdistributed_amd.ops.native import require_native  # noqa: E402

SHAPES = [(256, 56), (512, 28), (1024, 14), (2048, 7)]


def _time(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3   # us


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=96)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--only", type=int, default=0, help="one C of the table")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_se needs a GPU")
    C_ = require_native("bench_se")
    N, bf = args.batch, torch.bfloat16
    for C, hw in SHAPES:
        if args.only and C != args.only:
            continue
        Cr = C // 16
        act = lambda: torch.randn(N, C, hw, hw, device="cuda", dtype=bf).contiguous(  # noqa: E731
            memory_format=torch.channels_last)
        u, idn, g = act(), act(), act()
        w1 = (torch.randn(Cr, C, device="cuda") / C ** 0.5).to(bf)
        w2 = (torch.randn(C, Cr, device="cuda") / Cr ** 0.5).to(bf)
        b1, b2 = torch.zeros(Cr, device="cuda", dtype=bf), torch.zeros(
            C, device="cuda", dtype=bf)
        out, s, h, z = C_.se_fwd(u, idn, w1, b1, w2, b2)
        T = u.numel() * 2
        row = dict(
            C=C, HW=hw * hw, Cr=Cr, tensor_MB=round(T / 1e6, 2),
            plan=C_.se_config(N, hw * hw, C, Cr),
            se_fwd_us=_time(lambda: C_.se_fwd(u, idn, w1, b1, w2, b2), args.iters),
            se_bwd_us=_time(lambda: C_.se_bwd(g, out, u, s, h, z, w1, w2), args.iters),
            add_relu_fwd_us=_time(lambda: C_.add_relu_fwd(u, idn), args.iters))
        row["add_relu_fwd_GBps"] = round(3 * T / row["add_relu_fwd_us"] / 1e3, 1)
        print(json.dumps(row))


if __name__ == "__main__":
    main()
