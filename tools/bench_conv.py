#!/usr/bin/env python3
"""Per-shape conv microbenchmark: fda conv_igemm vs the library (MIOpen).

Times fwd and dgrad for every ResNet-34 bs-96 body shape; prints a table
with effective TFLOP/s. Run on a GPU box:
    python tools/bench_conv.py [--batch 96] [--iters 50]
    python tools/bench_conv.py --mode dgrad --iters 200   # dgrad arms only
    python tools/bench_conv.py --mode wgrad --iters 200   # wgrad arms only
    python tools/bench_conv.py --dtype fp32   # conv_f32 kernels vs aten fp32
    python tools/bench_conv.py --groups       # conv_grouped vs the library
    python tools/bench_conv.py --depthwise    # conv_dw vs the library
    python tools/bench_conv.py --pointwise    # conv_pw vs the library
    python tools/bench_conv.py --stem-narrow  # conv_stem_narrow, narrow BN
"""

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fluxdistributed_amd.ops.native import require_native  # noqa: E402

# (C, H, W, K, R, stride, count_in_resnet34)
SHAPES = [
    (64, 56, 56, 64, 3, 1, 7),      # layer1 3x3 (6 full + conv2 of first)
    (64, 56, 56, 128, 3, 2, 1),     # layer2 entry
    (64, 56, 56, 128, 1, 2, 1),     # layer2 downsample
    (128, 28, 28, 128, 3, 1, 7),
    (128, 28, 28, 256, 3, 2, 1),
    (128, 28, 28, 256, 1, 2, 1),
    (256, 14, 14, 256, 3, 1, 11),
    (256, 14, 14, 512, 3, 2, 1),
    (256, 14, 14, 512, 1, 2, 1),
    (512, 7, 7, 512, 3, 1, 5),
]


def timeit(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def event_us(fn, iters, warmup=10):
    """Mean device time of one call in us (events around `iters` calls)."""
    for _ in range(warmup):
        fn()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def dgrad_arms(args):
    """Input-grad arms: plain, and with the deferred junction gradient
    (`accum`) added in the epilogue. Each figure is the median of
    --repeats timed blocks, with their min..max as the run-to-run spread."""
    C_ = require_native("conv_igemm_dgrad")
    n = args.batch
    print(f"# batch={n} dgrad, us per call: median (min..max) of "
          f"{args.repeats} blocks of {args.iters} calls")
    print(f"{'shape':34s} {'plain':>22s} {'with accum':>22s}")
    shapes = SHAPES if args.only < 0 else [SHAPES[args.only]]
    tot = [0.0, 0.0]
    for (c, h, w, k, r, s, cnt) in shapes:
        pad = r // 2
        P, Q = (h + 2 * pad - r) // s + 1, (w + 2 * pad - r) // s + 1
        gy = torch.randn(n, k, P, Q, device="cuda").bfloat16() \
            .contiguous(memory_format=torch.channels_last)
        wtt = torch.randn(r * r * c, k, device="cuda").bfloat16()
        acc = torch.randn(n, c, h, w, device="cuda").bfloat16() \
            .contiguous(memory_format=torch.channels_last)
        arms = [
            lambda: C_.conv_igemm_dgrad(gy, wtt, c, h, w, r, r, s, s, pad,
                                        pad, None),
            lambda: C_.conv_igemm_dgrad(gy, wtt, c, h, w, r, r, s, s, pad,
                                        pad, acc),
        ]
        cells = []
        # blocks of the arms in turn, so drift hits every arm alike
        ts = [[] for _ in arms]
        for _ in range(args.repeats):
            for i, fn in enumerate(arms):
                ts[i].append(event_us(fn, args.iters))
        for i, t in enumerate(ts):
            t.sort()
            med = t[len(t) // 2]
            tot[i] += med * cnt
            cells.append(f"{med:7.1f} ({t[0]:.1f}..{t[-1]:.1f})")
        name = f"{c}x{h}x{w} k{k} {r}x{r} s{s} x{cnt}"
        print(f"{name:34s} {cells[0]:>22s} {cells[1]:>22s}")
    print(f"{'TOTAL (weighted by layer count)':34s} {tot[0]:22.1f} {tot[1]:22.1f}")


def wgrad_arms(args):
    """Weight-grad arms: the kernel alone, accumulating into one workspace
    (conv_igemm_wgrad_into, as the train step calls it), and with the
    workspace allocation and zero fill on a shape the rule keeps on atomics
    or the slabs and the fp32 fold on one it does not (conv_igemm_wgrad), and
    the slab kernel plus the ordered bf16 fold into a flat-G slice
    (conv_igemm_wgrad_flush, the train step's call where
    conv_igemm_wgrad_mode says "slab"; timed on every shape). Figures as for
    --mode dgrad: the median of --repeats timed blocks and their min..max."""
    C_ = require_native("conv_igemm_wgrad_into")
    n = args.batch
    print(f"# batch={n} wgrad, us per call: median (min..max) of "
          f"{args.repeats} blocks of {args.iters} calls")
    print(f"{'shape':34s} {'kernel (into)':>22s} {'allocating form':>22s} "
          f"{'slabs + fold':>22s}  mode")
    shapes = SHAPES if args.only < 0 else [SHAPES[args.only]]
    tot = [0.0, 0.0, 0.0]
    for (c, h, w, k, r, s, cnt) in shapes:
        pad = r // 2
        P, Q = (h + 2 * pad - r) // s + 1, (w + 2 * pad - r) // s + 1
        gy = torch.randn(n, k, P, Q, device="cuda").bfloat16() \
            .contiguous(memory_format=torch.channels_last)
        x = torch.randn(n, c, h, w, device="cuda").bfloat16() \
            .contiguous(memory_format=torch.channels_last)
        ws = torch.zeros(k * r * r * c, device="cuda")
        g = torch.zeros(k * r * r * c, device="cuda", dtype=torch.bfloat16)
        arms = [
            lambda: C_.conv_igemm_wgrad_into(gy, x, ws, r, r, s, s, pad, pad),
            lambda: C_.conv_igemm_wgrad(gy, x, r, r, s, s, pad, pad),
            lambda: C_.conv_igemm_wgrad_flush(gy, x, g, r, r, s, s, pad, pad),
        ]
        cells = []
        # blocks of the arms in turn, so drift hits every arm alike
        ts = [[] for _ in arms]
        for _ in range(args.repeats):
            for i, fn in enumerate(arms):
                ts[i].append(event_us(fn, args.iters))
        for i, t in enumerate(ts):
            t.sort()
            med = t[len(t) // 2]
            tot[i] += med * cnt
            cells.append(f"{med:7.1f} ({t[0]:.1f}..{t[-1]:.1f})")
        name = f"{c}x{h}x{w} k{k} {r}x{r} s{s} x{cnt}"
        mode = C_.conv_igemm_wgrad_mode(n * P * Q, c, k, r, r)
        print(f"{name:34s} {cells[0]:>22s} {cells[1]:>22s} {cells[2]:>22s}"
              f"  {mode}")
    print(f"{'TOTAL (weighted by layer count)':34s} {tot[0]:22.1f} "
          f"{tot[1]:22.1f} {tot[2]:22.1f}")


def f32_arms(args):
    """fp32: the conv_f32 kernels against aten's fp32 conv (the library) on
    the same tensors, per shape and per leg. Device events around --iters
    calls after warm-up; each figure is the median of --repeats such blocks,
    the two arms of a leg taken in turn."""
    C_ = require_native("conv_f32_fwd")
    torch.backends.cudnn.benchmark = True
    n = args.batch
    print(f"# batch={n} fp32, us per call: median of {args.repeats} blocks of "
          f"{args.iters} calls; tile = conv_f32_config of fwd/dgrad/wgrad")
    print(f"{'shape':32s} {'fda_fwd':>9s} {'lib_fwd':>9s} | {'fda_dg':>9s} "
          f"{'lib_dg':>9s} | {'fda_wg':>9s} {'lib_wg':>9s}  fda_TF  tiles (nch)")
    shapes = SHAPES if args.only < 0 else [SHAPES[args.only]]
    tot = [0.0] * 6
    for (c, h, w, k, r, s, cnt) in shapes:
        pad = r // 2
        P, Q = (h + 2 * pad - r) // s + 1, (w + 2 * pad - r) // s + 1
        cl = torch.channels_last
        x = torch.randn(n, c, h, w, device="cuda").contiguous(memory_format=cl)
        wt = torch.randn(k, c, r, r, device="cuda").contiguous(memory_format=cl)
        gy = torch.randn(n, k, P, Q, device="cuda").contiguous(memory_format=cl)

        def lib_bwd(mask):
            return torch.ops.aten.convolution_backward(
                gy, x, wt, None, [s, s], [pad, pad], [1, 1], False, [0, 0], 1,
                mask)
        arms = [
            lambda: C_.conv_f32_fwd(x, wt, s, s, pad, pad),
            lambda: torch.nn.functional.conv2d(x, wt, None, s, pad),
            lambda: C_.conv_f32_dgrad(gy, wt, h, w, s, s, pad, pad),
            lambda: lib_bwd([True, False, False]),
            lambda: C_.conv_f32_wgrad(gy, x, r, r, s, s, pad, pad),
            lambda: lib_bwd([False, True, False]),
        ]
        ts = [[] for _ in arms]
        for _ in range(args.repeats):
            for i, fn in enumerate(arms):
                if args.fda_only and i % 2:
                    ts[i].append(float("inf"))
                else:
                    ts[i].append(event_us(fn, args.iters))
        med = [sorted(t)[len(t) // 2] for t in ts]
        for i in range(6):
            tot[i] += med[i] * cnt
        rows_d = n * -(-h // s) * -(-w // s)
        cf = (C_.conv_f32_config(n * P * Q, c, k, r, r, "fwd"),
              C_.conv_f32_config(rows_d, c, k, r, r, "dgrad"),
              C_.conv_f32_config(n * P * Q, c, k, r, r, "wgrad"))
        tf = 2.0 * n * P * Q * k * c * r * r / med[0] / 1e6
        name = f"{c}x{h}x{w} k{k} {r}x{r} s{s} x{cnt}"
        print(f"{name:32s} {med[0]:9.1f} {med[1]:9.1f} | {med[2]:9.1f} "
              f"{med[3]:9.1f} | {med[4]:9.1f} {med[5]:9.1f}  {tf:6.1f}  "
              f"{cf[0][0]}/{cf[1][0]}/{cf[2][0]} ({cf[2][2]})")
    print(f"{'TOTAL (weighted by layer count)':32s} {tot[0]:9.1f} {tot[1]:9.1f} "
          f"| {tot[2]:9.1f} {tot[3]:9.1f} | {tot[4]:9.1f} {tot[5]:9.1f}")


# grouped 3x3 convs of ResNeXt-50 32x4d: (C, H, W, groups, stride, count)
GROUPED_SHAPES = [
    (128, 56, 56, 32, 1, 3),
    (256, 56, 56, 32, 2, 1),
    (256, 28, 28, 32, 1, 3),
    (512, 28, 28, 32, 2, 1),
    (512, 14, 14, 32, 1, 5),
    (1024, 14, 14, 32, 2, 1),
    (1024, 7, 7, 32, 1, 2),
]
HBM_BYTES_PER_US = 8.0e6   # MI355X peak, 8 TB/s


def grouped_arms(args):
    """Grouped 3x3: the conv_grouped kernels against the library's grouped
    conv on the same tensors, per shape and per leg; figures as for --dtype
    fp32. floor: the time the leg's compulsory bytes (input + output once;
    wgrad: x + dy once) take at the peak HBM rate, and the fraction of it
    the native kernel reaches."""
    C_ = require_native("conv_grouped_fwd")
    torch.backends.cudnn.benchmark = True
    n = args.batch
    print(f"# batch={n} grouped bf16, us per call: median of {args.repeats} "
          f"blocks of {args.iters} calls; floor at 8 TB/s")
    print(f"{'shape':30s} {'fda_fwd':>8s} {'lib_fwd':>8s} | {'fda_dg':>8s} "
          f"{'lib_dg':>8s} | {'fda_wg':>8s} {'lib_wg':>8s} | {'floor':>6s}  "
          f"fwd/dg/wg of floor  wgrad (nch, px)")
    shapes = (GROUPED_SHAPES if args.only < 0
              else [GROUPED_SHAPES[args.only]])
    tot = [0.0] * 6
    cl = torch.channels_last
    for (c, h, w, g, s, cnt) in shapes:
        P, Q = (h - 1) // s + 1, (w - 1) // s + 1
        x = torch.randn(n, c, h, w, device="cuda").bfloat16() \
            .contiguous(memory_format=cl)
        wt = torch.randn(c, c // g, 3, 3, device="cuda").bfloat16() \
            .contiguous(memory_format=cl)
        gy = torch.randn(n, c, P, Q, device="cuda").bfloat16() \
            .contiguous(memory_format=cl)

        def lib_bwd(mask):
            return torch.ops.aten.convolution_backward(
                gy, x, wt, None, [s, s], [1, 1], [1, 1], False, [0, 0], g,
                mask)
        arms = [
            lambda: C_.conv_grouped_fwd(x, wt, s, s, 1, 1, g),
            lambda: torch.nn.functional.conv2d(x, wt, None, s, 1, 1, g),
            lambda: C_.conv_grouped_dgrad(gy, wt, h, w, s, s, 1, 1, g),
            lambda: lib_bwd([True, False, False]),
            lambda: C_.conv_grouped_wgrad(gy, x, s, s, 1, 1, g),
            lambda: lib_bwd([False, True, False]),
        ]
        ts = [[] for _ in arms]
        for _ in range(args.repeats):
            for i, fn in enumerate(arms):
                if args.fda_only and i % 2:
                    ts[i].append(float("inf"))
                else:
                    ts[i].append(event_us(fn, args.iters))
        med = [sorted(t)[len(t) // 2] for t in ts]
        for i in range(6):
            tot[i] += med[i] * cnt
        floor = 2.0 * (x.numel() + gy.numel()) / HBM_BYTES_PER_US
        cf = C_.conv_grouped_config(n, h, w, c, g, s, "wgrad")
        name = f"{c}x{h}x{w} g{g} s{s} x{cnt}"
        print(f"{name:30s} {med[0]:8.1f} {med[1]:8.1f} | {med[2]:8.1f} "
              f"{med[3]:8.1f} | {med[4]:8.1f} {med[5]:8.1f} | {floor:6.1f}  "
              f"{floor / med[0]:.2f}/{floor / med[2]:.2f}/{floor / med[4]:.2f}"
              f"  ({cf[2]}, {cf[3]})", flush=True)
    print(f"{'TOTAL (weighted by layer count)':30s} {tot[0]:8.1f} {tot[1]:8.1f} "
          f"| {tot[2]:8.1f} {tot[3]:8.1f} | {tot[4]:8.1f} {tot[5]:8.1f}")


# depthwise 3x3 convs of MobileNetV1: (C, input H = W, stride, count)
DW_SHAPES = [
    (32, 112, 1, 1),
    (64, 112, 2, 1),
    (128, 56, 1, 1),
    (128, 56, 2, 1),
    (256, 28, 1, 1),
    (256, 28, 2, 1),
    (512, 14, 1, 5),
    (512, 14, 2, 1),
    (1024, 7, 1, 1),
]


def depthwise_arms(args):
    """Depthwise 3x3: the conv_dw kernels against the library's depthwise
    conv on the same tensors, per shape and per leg; figures as for --groups.
    min MB: the leg's compulsory traffic (fwd and dgrad: the input once and
    the output once; wgrad: x and dy once; the same bytes for all three), and
    after it the rate each native leg reaches on those bytes, in TB/s."""
    C_ = require_native("conv_dw_fwd")
    torch.backends.cudnn.benchmark = True
    n = args.batch
    print(f"# batch={n} depthwise bf16, us per call: median of {args.repeats} "
          f"blocks of {args.iters} calls")
    print(f"{'shape':22s} {'fda_fwd':>8s} {'lib_fwd':>8s} | {'fda_dg':>8s} "
          f"{'lib_dg':>8s} | {'fda_wg':>8s} {'lib_wg':>8s} | {'min MB':>7s}  "
          f"fwd/dg/wg TB/s  wgrad (nch, rows)")
    shapes = DW_SHAPES if args.only < 0 else [DW_SHAPES[args.only]]
    tot = [0.0] * 6
    cl = torch.channels_last
    for (c, h, s, cnt) in shapes:
        P = (h - 1) // s + 1
        x = torch.randn(n, c, h, h, device="cuda").bfloat16() \
            .contiguous(memory_format=cl)
        wt = torch.randn(c, 1, 3, 3, device="cuda").bfloat16()
        gy = torch.randn(n, c, P, P, device="cuda").bfloat16() \
            .contiguous(memory_format=cl)

        def lib_bwd(mask):
            return torch.ops.aten.convolution_backward(
                gy, x, wt, None, [s, s], [1, 1], [1, 1], False, [0, 0], c,
                mask)
        arms = [
            lambda: C_.conv_dw_fwd(x, wt, s, s),
            lambda: torch.nn.functional.conv2d(x, wt, None, s, 1, 1, c),
            lambda: C_.conv_dw_dgrad(gy, wt, h, h, s, s),
            lambda: lib_bwd([True, False, False]),
            lambda: C_.conv_dw_wgrad(gy, x, s, s),
            lambda: lib_bwd([False, True, False]),
        ]
        ts = [[] for _ in arms]
        for _ in range(args.repeats):
            for i, fn in enumerate(arms):
                if args.fda_only and i % 2:
                    ts[i].append(float("inf"))
                else:
                    ts[i].append(event_us(fn, args.iters))
        med = [sorted(t)[len(t) // 2] for t in ts]
        for i in range(6):
            tot[i] += med[i] * cnt
        nbytes = 2.0 * (x.numel() + gy.numel())
        rate = [nbytes / med[i] / 1e6 for i in (0, 2, 4)]   # B/us -> TB/s
        cf = C_.conv_dw_config(n, h, h, c, s, "wgrad")
        name = f"{c}x{h}x{h} s{s} x{cnt}"
        print(f"{name:22s} {med[0]:8.1f} {med[1]:8.1f} | {med[2]:8.1f} "
              f"{med[3]:8.1f} | {med[4]:8.1f} {med[5]:8.1f} | "
              f"{nbytes / 1e6:7.1f}  "
              f"{rate[0]:.2f}/{rate[1]:.2f}/{rate[2]:.2f}"
              f"  ({cf[2]}, {cf[3]})", flush=True)
    print(f"{'TOTAL (weighted by count)':22s} {tot[0]:8.1f} {tot[1]:8.1f} "
          f"| {tot[2]:8.1f} {tot[3]:8.1f} | {tot[4]:8.1f} {tot[5]:8.1f}")


# pointwise convs of MobileNetV1 that conv_pw serves: (C, K, H = W, label)
PW_SHAPES = [
    (32, 64, 112, "w1.0"),
    (8, 16, 112, "w0.25"),
    (16, 32, 56, "w0.25"),
    (32, 32, 56, "w0.25"),
    (32, 64, 28, "w0.25"),
]


def pointwise_arms(args):
    """Narrow 1x1: the conv_pw kernels against the library's conv on the same
    tensors, per shape and per leg. us per call: the median of the blocks,
    and behind each library figure its spread over the blocks,
    (max - min) / median in percent. min MB: the leg's compulsory traffic (x
    and y, or dy and dx, or x and dy, once: the same bytes for all three),
    and after it the rate each native leg reaches on those bytes, in TB/s."""
    C_ = require_native("conv_pw_fwd")
    torch.backends.cudnn.benchmark = True
    n = args.batch
    print(f"# batch={n} pointwise bf16, us per call: median of {args.repeats} "
          f"blocks of {args.iters} calls; (..%): spread of the library arm")
    print(f"{'shape':22s} {'fda_fwd':>8s} {'lib_fwd':>14s} | {'fda_dg':>8s} "
          f"{'lib_dg':>14s} | {'fda_wg':>8s} {'lib_wg':>14s} | {'min MB':>7s}  "
          f"fwd/dg/wg TB/s  wgrad (nch, pixels)")
    shapes = PW_SHAPES if args.only < 0 else [PW_SHAPES[args.only]]
    cl = torch.channels_last
    for (c, k, h, label) in shapes:
        x = torch.randn(n, c, h, h, device="cuda").bfloat16() \
            .contiguous(memory_format=cl)
        wt = torch.randn(k, c, 1, 1, device="cuda").bfloat16()
        gy = torch.randn(n, k, h, h, device="cuda").bfloat16() \
            .contiguous(memory_format=cl)

        def lib_bwd(mask):
            return torch.ops.aten.convolution_backward(
                gy, x, wt, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                mask)
        arms = [
            lambda: C_.conv_pw_fwd(x, wt),
            lambda: torch.nn.functional.conv2d(x, wt),
            lambda: C_.conv_pw_dgrad(gy, wt),
            lambda: lib_bwd([True, False, False]),
            lambda: C_.conv_pw_wgrad(gy, x),
            lambda: lib_bwd([False, True, False]),
        ]
        ts = [[] for _ in arms]
        for _ in range(args.repeats):
            for i, fn in enumerate(arms):
                if args.fda_only and i % 2:
                    ts[i].append(float("nan"))
                else:
                    ts[i].append(event_us(fn, args.iters))
        med = [sorted(t)[len(t) // 2] for t in ts]
        lib = [f"{med[i]:7.1f} ({100 * (max(ts[i]) - min(ts[i])) / med[i]:2.0f}%)"
               for i in (1, 3, 5)]
        nbytes = 2.0 * (x.numel() + gy.numel())
        rate = [nbytes / med[i] / 1e6 for i in (0, 2, 4)]   # B/us -> TB/s
        cf = C_.conv_pw_config(n * h * h, c, k, "wgrad")
        name = f"{c}->{k} {h}x{h} {label}"
        print(f"{name:22s} {med[0]:8.1f} {lib[0]:>14s} | {med[2]:8.1f} "
              f"{lib[1]:>14s} | {med[4]:8.1f} {lib[2]:>14s} | "
              f"{nbytes / 1e6:7.1f}  "
              f"{rate[0]:.2f}/{rate[1]:.2f}/{rate[2]:.2f}"
              f"  ({cf[2]}, {cf[3]})", flush=True)


# narrow stems of MobileNetV1: (K, H = W, stride, label)
STEM_NARROW_SHAPES = [
    (8, 224, 2, "w0.25"),
    (16, 224, 2, "w0.5"),
    (24, 224, 2, "w0.75"),
    (32, 224, 2, "w1.0"),
    (32, 32, 1, "w1.0 small_input"),
]


def _blocks(arms, args):
    """event_us of every arm, args.repeats blocks, the arms alternating."""
    ts = [[] for _ in arms]
    for _ in range(args.repeats):
        for i, fn in enumerate(arms):
            if args.fda_only and i % 2:
                ts[i].append(float("nan"))
            else:
                ts[i].append(event_us(fn, args.iters))
    med = [sorted(t)[len(t) // 2] for t in ts]
    lib = [f"{med[i]:7.1f} ({100 * (max(ts[i]) - min(ts[i])) / med[i]:2.0f}%)"
           for i in range(1, len(arms), 2)]
    return med, lib


def stem_narrow_arms(args):
    """The conv_stem_narrow kernels against the library's conv on the same
    tensors (forward and weight-grad; there is no dgrad), then the narrow
    BatchNorm: the native bn_act_fwd / bn_act_bwd pair on 32 channels at
    112x112 against the fp32 library composition BNAct falls back to (its
    backward through autograd). us per call: the median of the blocks, the
    arms alternating; behind each library figure its spread over the blocks,
    (max - min) / median in percent. min MB and TB/s as for --pointwise."""
    C_ = require_native("conv_stem_narrow_fwd")
    F = torch.nn.functional
    torch.backends.cudnn.benchmark = True
    n = args.batch
    cl = torch.channels_last
    print(f"# batch={n} narrow stem bf16, us per call: median of "
          f"{args.repeats} blocks of {args.iters} calls; (..%): spread of the "
          f"library arm")
    print(f"{'shape':28s} {'fda_fwd':>8s} {'lib_fwd':>14s} | {'fda_wg':>8s} "
          f"{'lib_wg':>14s} | {'min MB':>7s}  fwd/wg TB/s  wgrad (nch, upc)")
    shapes = (STEM_NARROW_SHAPES if args.only < 0
              else [STEM_NARROW_SHAPES[args.only]])
    for (k, h, s, label) in shapes:
        x = torch.randn(n, 3, h, h, device="cuda").bfloat16() \
            .contiguous(memory_format=cl)
        wt = torch.randn(k, 3, 3, 3, device="cuda").bfloat16() \
            .contiguous(memory_format=cl)
        q = (h - 1) // s + 1
        gy = torch.randn(n, k, q, q, device="cuda").bfloat16() \
            .contiguous(memory_format=cl)
        arms = [
            lambda: C_.conv_stem_narrow_fwd(x, wt, s),
            lambda: F.conv2d(x, wt, None, s, 1),
            lambda: C_.conv_stem_narrow_wgrad(gy, x, s),
            lambda: torch.ops.aten.convolution_backward(
                gy, x, wt, None, [s, s], [1, 1], [1, 1], False, [0, 0], 1,
                [False, True, False]),
        ]
        med, lib = _blocks(arms, args)
        nbytes = 2.0 * (x.numel() + gy.numel())
        cf = C_.conv_stem_narrow_config(n, h, h, 3, k, s, "wgrad")
        name = f"3->{k} {h}x{h}/{s} {label}"
        print(f"{name:28s} {med[0]:8.1f} {lib[0]:>14s} | {med[2]:8.1f} "
              f"{lib[1]:>14s} | {nbytes / 1e6:7.1f}  "
              f"{nbytes / med[0] / 1e6:.2f}/{nbytes / med[2] / 1e6:.2f}"
              f"  ({cf[5]}, {cf[6]})", flush=True)

    c, h = 32, 112
    x = torch.randn(n, c, h, h, device="cuda").bfloat16() \
        .contiguous(memory_format=cl)
    gy = torch.randn_like(x)
    w = torch.rand(c, device="cuda") + 0.5
    b = torch.randn(c, device="cuda")
    rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    none = torch.empty(0, device="cuda", dtype=torch.bfloat16)
    out, mean, invstd = C_.bn_act_fwd(x, w, b, rm, rv, True, 0.1, 1e-5, True,
                                      none)

    def lib_fwd():
        o = F.batch_norm(x.float(), rm, rv, w, b, True, 0.1, 1e-5)
        return torch.relu(o).to(x.dtype)

    xr = x.detach().requires_grad_(True)
    wr, br = w.detach().requires_grad_(True), b.detach().requires_grad_(True)
    yr = torch.relu(F.batch_norm(xr.float(), rm, rv, wr, br, True, 0.1,
                                 1e-5)).to(x.dtype)
    arms = [
        lambda: C_.bn_act_fwd(x, w, b, rm, rv, True, 0.1, 1e-5, True, none),
        lib_fwd,
        lambda: C_.bn_act_bwd(gy, x, w, mean, invstd, out, True, True, None,
                              None, False, b),
        lambda: torch.autograd.grad(yr, (xr, wr, br), gy, retain_graph=True),
    ]
    med, lib = _blocks(arms, args)
    print(f"# BN+ReLU training, {c} channels, {n}x{h}x{h} bf16")
    print(f"{'':28s} {'fda_fwd':>8s} {'lib_fwd':>14s} | {'fda_bwd':>8s} "
          f"{'lib_bwd':>14s}")
    print(f"{'bn_act ' + str(c):28s} {med[0]:8.1f} {lib[0]:>14s} | "
          f"{med[2]:8.1f} {lib[1]:>14s}", flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=96)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--repeats", type=int, default=5,
                   help="timed blocks per arm (--mode dgrad, wgrad)")
    p.add_argument("--mode", choices=["fwd", "dgrad", "wgrad", "both"],
                   default="both",
                   help="dgrad: only the input-grad arms, plain and with "
                        "accum, with their run-to-run spread; wgrad: only "
                        "the weight-grad arms, likewise")
    p.add_argument("--only", type=int, default=-1,
                   help="run only SHAPES[i] (for PMC profiling runs)")
    p.add_argument("--fda-only", action="store_true",
                   help="skip the library arms (clean kernel-trace)")
    p.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16",
                   help="fp32: the conv_f32 kernels against aten's fp32 conv, "
                        "all three legs")
    p.add_argument("--groups", action="store_true",
                   help="the grouped 3x3 shapes of ResNeXt-50 32x4d: the "
                        "conv_grouped kernels against the library, all three "
                        "legs")
    p.add_argument("--depthwise", action="store_true",
                   help="the depthwise 3x3 shapes of MobileNetV1: the conv_dw "
                        "kernels against the library, all three legs, with "
                        "the rate reached on the compulsory bytes")
    p.add_argument("--pointwise", action="store_true",
                   help="the narrow 1x1 shapes of MobileNetV1 (width 1.0 and "
                        "0.25): the conv_pw kernels against the library, all "
                        "three legs, with the library's spread")
    p.add_argument("--stem-narrow", action="store_true",
                   help="the MobileNetV1 stems (K = 8 .. 32): the "
                        "conv_stem_narrow kernels against the library, forward "
                        "and weight-grad, then the 32-channel training BN "
                        "against the library composition")
    args = p.parse_args()
    assert torch.cuda.is_available()
    if args.stem_narrow:
        return stem_narrow_arms(args)
    if args.pointwise:
        return pointwise_arms(args)
    if args.depthwise:
        return depthwise_arms(args)
    if args.groups:
        return grouped_arms(args)
    if args.dtype == "fp32":
        return f32_arms(args)
    if args.mode == "dgrad":
        return dgrad_arms(args)
    if args.mode == "wgrad":
        return wgrad_arms(args)
    torch.backends.cudnn.benchmark = True
    C_ = require_native("conv_igemm_fwd")
    n = args.batch

    print(f"# batch={n}  times in us, eff TF = 2*M*N*K / t")
    print(f"{'shape':34s} {'fda_fwd':>9s} {'lib_fwd':>9s} {'fda_TF':>7s} {'lib_TF':>7s}"
          f" | {'fda_dg':>9s} {'lib_dg':>9s} | {'fda_wg':>9s} {'lib_wg':>9s}")
    tot_fda_f = tot_lib_f = tot_fda_d = tot_lib_d = 0.0
    tot_fda_w = tot_lib_w = 0.0
    shapes = SHAPES if args.only < 0 else [SHAPES[args.only]]
    for (c, h, w, k, r, s, cnt) in shapes:
        pad = r // 2
        P, Q = (h + 2 * pad - r) // s + 1, (w + 2 * pad - r) // s + 1
        x = torch.randn(n, c, h, w, device="cuda").bfloat16() \
            .contiguous(memory_format=torch.channels_last)
        wt = torch.randn(k, c, r, r, device="cuda").bfloat16() \
            .contiguous(memory_format=torch.channels_last)
        flops = 2.0 * n * P * Q * k * c * r * r

        t_ff = timeit(lambda: C_.conv_igemm_fwd(x, wt, s, s, pad, pad), args.iters)
        t_lf = (timeit(lambda: torch.nn.functional.conv2d(x, wt, None, s, pad),
                       args.iters) if not args.fda_only else float("inf"))
        gy = torch.randn(n, k, P, Q, device="cuda").bfloat16() \
            .contiguous(memory_format=torch.channels_last)
        wtt = wt.permute(2, 3, 1, 0).reshape(r * r * c, k).contiguous()
        t_fd = timeit(lambda: C_.conv_igemm_dgrad(gy, wtt, c, h, w, r, r,
                                                  s, s, pad, pad), args.iters)
        xg = x.requires_grad_(True)

        def lib_dgrad():
            return torch.ops.aten.convolution_backward(
                gy, xg, wt, None, [s, s], [pad, pad], [1, 1], False, [0, 0],
                1, [True, False, False])[0]
        t_ld = timeit(lib_dgrad, args.iters) if not args.fda_only else float("inf")
        t_fw = timeit(lambda: C_.conv_igemm_wgrad(gy, x, r, r, s, s, pad, pad),
                      args.iters)

        def lib_wgrad():
            return torch.ops.aten.convolution_backward(
                gy, xg, wt, None, [s, s], [pad, pad], [1, 1], False, [0, 0],
                1, [False, True, False])[1]
        t_lw = timeit(lib_wgrad, args.iters) if not args.fda_only else float("inf")

        name = f"{c}x{h}x{w} k{k} {r}x{r} s{s} x{cnt}"
        print(f"{name:34s} {t_ff*1e6:9.1f} {t_lf*1e6:9.1f} "
              f"{flops/t_ff/1e12:7.1f} {flops/t_lf/1e12:7.1f} | "
              f"{t_fd*1e6:9.1f} {t_ld*1e6:9.1f} | "
              f"{t_fw*1e6:9.1f} {t_lw*1e6:9.1f}")
        tot_fda_f += t_ff * cnt
        tot_lib_f += t_lf * cnt
        tot_fda_d += t_fd * cnt
        tot_lib_d += t_ld * cnt
        tot_fda_w += t_fw * cnt
        tot_lib_w += t_lw * cnt
    print(f"{'TOTAL (weighted by layer count)':34s} {tot_fda_f*1e6:9.1f} "
          f"{tot_lib_f*1e6:9.1f} {'':7s} {'':7s} | {tot_fda_d*1e6:9.1f} "
          f"{tot_lib_d*1e6:9.1f} | {tot_fda_w*1e6:9.1f} {tot_lib_w*1e6:9.1f}")


if __name__ == "__main__":
    main()
