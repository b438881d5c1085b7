#!/usr/bin/env python3
"""Inference microbenchmarks: the fused conv+BN(+residual)+ReLU epilogue
against the two-pass eval path. Run on a GPU box.

  python tools/bench_infer.py shapes --model resnet34 --batch 96
      every distinct conv+BN pair of the model (shapes traced from a CPU
      forward), unfused (conv_igemm_fwd / conv_stem_fwd, then eval
      bn_act_fwd) against fused (one launch, BN coefficients folded
      beforehand), us per pair

  python tools/bench_infer.py model --model resnet34 --batch 1 8 96
      whole-model eval forward, images/s: model.eval() under no_grad,
      InferenceModel, InferenceModel.capture()

Arms are interleaved within each repeat; the table shows the median over
--repeats and the min..max spread.
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fluxdistributed_amd.inference import compile_for_inference  # noqa: E402
from fluxdistributed_amd.models import build_model  # noqa: E402
from fluxdistributed_amd.ops.native import require_native  # noqa: E402
from fluxdistributed_amd.utils.precision import to_mixed_bf16  # noqa: E402

CL = torch.channels_last


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def interleaved(arms, iters, repeats, warmup=10):
    """arms: {name: fn}. Returns {name: [seconds per call] * repeats}."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            out[k].append(window(fn, iters))
    return out


def fmt(ts, scale=1e6):
    return (f"{statistics.median(ts) * scale:8.1f} "
            f"[{min(ts) * scale:7.1f}..{max(ts) * scale:7.1f}]")


def traced_pairs(name, image):
    """Distinct (C, H, W, K, R, stride, pad, relu, residual) -> count, from
    a batch-1 CPU forward of the model."""
    model = build_model(name, num_classes=1000).eval()
    im = compile_for_inference(model)
    tails = {id(b.pairs[-1].conv) for b in im.blocks}
    seen = {}
    hooks = []
    for p in im.pairs:
        def hook(mod, inp, out, p=p):
            x = inp[0]
            key = (x.shape[1], x.shape[2], x.shape[3], mod.out_channels,
                   mod.kernel_size[0], mod.stride[0], mod.padding[0],
                   p.bn.relu, id(mod) in tails)
            seen[key] = seen.get(key, 0) + 1
        hooks.append(p.conv.register_forward_hook(hook))
    with torch.no_grad():
        model(torch.zeros(1, 3, image, image))
    for h in hooks:
        h.remove()
    return seen


def bench_shapes(args):
    C_ = require_native("conv_igemm_fwd_fused")
    dev = "cuda"
    n = args.batch[0]
    empty = torch.empty(0, device=dev, dtype=torch.bfloat16)
    print(f"# {args.model} batch={n}: us per conv+BN pair, median "
          f"[min..max] of {args.repeats} interleaved repeats x {args.iters} "
          f"calls")
    print(f"{'pair':40s} {'n':>2s} {'unfused':>26s} {'fused':>26s} {'ratio':>6s}")
    tot = {"unfused": 0.0, "fused": 0.0}
    for key, cnt in traced_pairs(args.model, args.image).items():
        c, h, w, k, r, s, pad, relu, has_res = key
        P, Q = (h + 2 * pad - r) // s + 1, (w + 2 * pad - r) // s + 1
        x = torch.randn(n, c, h, w, device=dev).bfloat16() \
            .contiguous(memory_format=CL)
        wt = (torch.randn(k, c, r, r, device=dev) / (r * r * c) ** 0.5) \
            .bfloat16().contiguous(memory_format=CL)
        res = (torch.randn(n, k, P, Q, device=dev).bfloat16()
               .contiguous(memory_format=CL) if has_res else empty)
        bn = [torch.rand(k, device=dev) + 0.5, torch.randn(k, device=dev),
              torch.randn(k, device=dev), torch.rand(k, device=dev) + 0.5]
        arena = torch.empty(2 * k, device=dev)
        mk = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)  # noqa: E731
        C_.bn_fold_eval_batch(*(mk([t.data_ptr()], torch.long) for t in bn),
                              mk([k], torch.int32), mk([0], torch.long),
                              mk([1e-5], torch.float32), arena, k)
        scale, shift = arena[:k], arena[k:]
        if c % 64 == 0:
            def conv():
                return C_.conv_igemm_fwd(x, wt, s, s, pad, pad)

            def fused():
                return C_.conv_igemm_fwd_fused(x, wt, scale, shift, res, relu,
                                               s, s, pad, pad)
        else:   # stem: operands as ops/conv.py builds them
            x8 = torch.zeros(n, 8, h + 2 * pad, w + 2 * pad + 8, device=dev,
                             dtype=torch.bfloat16).contiguous(memory_format=CL)
            x8[:, :c, pad:pad + h, pad:pad + w] = x
            wpad = torch.zeros(k, r, 64, dtype=torch.bfloat16, device=dev)
            wpad.view(k, r, 8, 8)[:, :, :r, :c] = wt.permute(0, 2, 3, 1)

            def conv():
                return C_.conv_stem_fwd(x8, wpad, r, s, s, P, Q)

            def fused():
                return C_.conv_stem_fwd_fused(x8, wpad, scale, shift, relu, r,
                                              s, s, P, Q)

        def unfused():
            return C_.bn_act_fwd(conv(), *bn, False, 0.1, 1e-5, relu, res)

        ts = interleaved({"unfused": unfused, "fused": fused}, args.iters,
                         args.repeats)
        name = (f"{c}x{h}x{w} k{k} {r}x{r} s{s}"
                f"{' +res' if has_res else ''}{'' if relu else ' lin'}")
        mu, mf = (statistics.median(ts[a]) for a in ("unfused", "fused"))
        print(f"{name:40s} {cnt:2d} {fmt(ts['unfused'])} {fmt(ts['fused'])} "
              f"{mu / mf:6.2f}")
        tot["unfused"] += mu * cnt
        tot["fused"] += mf * cnt
    print(f"{'TOTAL (median x count)':40s}    {tot['unfused'] * 1e6:8.1f}"
          f"{'':18s} {tot['fused'] * 1e6:8.1f}{'':18s} "
          f"{tot['unfused'] / tot['fused']:6.2f}")


def bench_model(args):
    dev = torch.device("cuda:0")
    model = build_model(args.model, num_classes=1000).to(dev)
    model = to_mixed_bf16(model.to(memory_format=CL)).eval()
    im = compile_for_inference(model)
    print(f"# {args.model} eval forward, images/s: median [min..max] of "
          f"{args.repeats} interleaved repeats")
    print(f"{'batch':>5s} {'model.eval()':>28s} {'InferenceModel':>28s} "
          f"{'capture()':>28s}")
    for n in args.batch:
        x = torch.randn(n, 3, args.image, args.image, device=dev).bfloat16() \
            .contiguous(memory_format=CL)
        replay = im.capture(x)

        def eval_path():
            with torch.no_grad():
                return model(x)

        arms = {"eval": eval_path, "fused": lambda: im(x),
                "graph": lambda: replay(x)}
        iters = max(10, min(args.iters, 2000 // n))
        ts = interleaved(arms, iters, args.repeats, warmup=5)
        cols = []
        for a in ("eval", "fused", "graph"):
            r = [n / t for t in ts[a]]
            cols.append(f"{statistics.median(r):10.1f} "
                        f"[{min(r):8.1f}..{max(r):8.1f}]")
        print(f"{n:5d} " + " ".join(cols))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["shapes", "model"])
    p.add_argument("--model", default="resnet34")
    p.add_argument("--batch", type=int, nargs="+", default=[96])
    p.add_argument("--image", type=int, default=224)
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--repeats", type=int, default=5)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    (bench_shapes if args.mode == "shapes" else bench_model)(args)


if __name__ == "__main__":
    main()
