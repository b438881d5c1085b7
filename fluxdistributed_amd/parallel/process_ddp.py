"""Process-based DDP: one process per GPU, RCCL over xGMI.

MI355X-native replacement for the reference's disabled multi-process path
(/root/reference/src/sync.jl:36-232 + bin/driver.jl): there, every step
serialized the full CPU gradient tree over TCP RemoteChannels to a reducer
on proc 1 that folded, divided by a HARD-CODED 4.0, and serialized back.
Here: torch.distributed (backend "nccl" == RCCL on ROCm) with bucketed
all-reduce overlapped with backward; world size comes from the
communicator (fixing sync.jl:68); no D2H, no serializer in the data path.

Cooperative shutdown (the reference's all-`nothing` sentinel,
sync.jl:49-53) becomes an all-reduce of a stop flag: training stops only
when EVERY rank has voted to stop.
"""

import datetime
import os
from typing import Callable, Optional

import torch
import torch.distributed as dist

from .bucketing import GradBucketer
from ..ops.fused_optim import _FlatOptimizer
from ..utils.logging import get_logger
from ..utils.timers import StageTimers, Throughput

log = get_logger(__name__)


def init_process_group(backend: Optional[str] = None, timeout_s: int = 600):
    """Initialize from torchrun env vars; pins LOCAL_RANK's GPU.

    Backend: "nccl" (RCCL) when CUDA/HIP devices exist, else "gloo"
    (the CPU CI path — reference's fake-device trick).
    """
    if dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    if backend is None:
        backend = os.environ.get(
            "FLUXDIST_PG_BACKEND",
            "nccl" if torch.cuda.is_available() else "gloo",
        )
    if backend == "nccl":
        torch.cuda.set_device(local_rank)
    dist.init_process_group(
        backend=backend, rank=rank, world_size=world,
        timeout=datetime.timedelta(seconds=timeout_s),
    )
    return rank, world


class DDPModel(torch.nn.Module):
    """Data-parallel wrapper: broadcast params from rank 0 at init, bucketed
    all-reduce of the flat gradient buffer overlapped with backward.

    Requires a flat optimizer (FusedSGDMomentum / FusedAdam) constructed on
    the model FIRST — gradients then live in one flat buffer and buckets
    are zero-copy slices of it.
    """

    def __init__(self, model: torch.nn.Module, optimizer: _FlatOptimizer,
                 process_group=None, bucket_cap_mb: float = 25.0,
                 overlap: bool = True):
        super().__init__()
        self.module = model
        self.optimizer = optimizer
        self.overlap = overlap
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.bucketer = GradBucketer(optimizer, process_group, bucket_cap_mb)
        if self.world > 1:
            # one flat broadcast per group instead of ~110 leaf messages
            for g in optimizer.groups:
                dist.broadcast(g.P, src=0, group=process_group)
                if g.master is not None:
                    g.master.copy_(g.P.float())
            for name, buf in model.named_buffers():
                dist.broadcast(buf, src=0, group=process_group)
        if overlap:
            self.bucketer.attach()

    def forward(self, *args, **kw):
        return self.module(*args, **kw)

    def finalize_backward(self):
        """Call between loss.backward() and optimizer.step()."""
        if self.overlap:
            self.bucketer.finalize()
        else:
            self.bucketer.allreduce_now()


def log_grad_health(optimizer):
    """Log points only (both reads synchronize): the latest gradient norm
    and the skipped-step count of an optimizer that tracks them."""
    if hasattr(optimizer, "last_grad_norm"):
        log.info("grad_norm=%.4e skipped_steps=%d lr=%.4e",
                 float(optimizer.last_grad_norm()), optimizer.skipped_steps(),
                 optimizer.param_groups[0]["lr"])


def syncgrads_worker(
    model: torch.nn.Module,
    optimizer: _FlatOptimizer,
    loss_fn: Callable,
    batch_iter,
    steps: int,
    val: Optional[tuple] = None,
    val_every: int = 10,
    checkpoint_every: int = 0,
    checkpoint_dir: str = "weights",
    should_stop: Optional[Callable[[int], bool]] = None,
    bucket_cap_mb: float = 25.0,
    fused_eval: bool = False,
    sched: Optional[Callable[[int], None]] = None,
    log_every: int = 0,
):
    """Per-rank training loop — the `getgrads` worker + `syncgrads` reducer
    of the reference collapsed into symmetric all-reduce ranks
    (/root/reference/src/sync.jl:83-170 and :36-81).

    `sched(step)` is called once after every step with the number of steps
    done, as train() in task mode does. `log_every` > 0 logs the loss on
    rank 0 at that cadence, and the gradient norm and skipped-step count of
    an optimizer that has them (FusedLARS).

    Returns (model, optimizer, stats). Checkpoints (rank 0 only) follow the
    reference cadence knob (every `checkpoint_every` steps when > 0;
    sync.jl:156-161 used every-20-cycles).
    """
    rank = dist.get_rank() if dist.is_initialized() else 0
    ddp = DDPModel(model, optimizer, bucket_cap_mb=bucket_cap_mb)
    timers, thr = StageTimers(), Throughput()
    stop_flag = torch.zeros(1, dtype=torch.int64)
    if torch.cuda.is_available():
        stop_flag = stop_flag.cuda()

    for step, (x, y) in enumerate(batch_iter):
        if step >= steps:
            break
        with timers.stage("fwd"):
            out = ddp(x)
            loss = loss_fn(out, y)
        with timers.stage("bwd"):
            optimizer.zero_grad()
            loss.backward()
        with timers.stage("allreduce"):
            ddp.finalize_backward()
        with timers.stage("optimizer"):
            optimizer.step()
        thr.add(int(x.shape[0]) * ddp.world)
        if sched is not None:
            sched(step + 1)
        if log_every and (step + 1) % log_every == 0 and rank == 0:
            log.info("step %d loss=%.4f imgs/s=%.1f", step + 1, float(loss),
                     thr.rate())
            log_grad_health(optimizer)

        if val is not None and val_every and (step + 1) % val_every == 0 and rank == 0:
            from .task_ddp import log_loss_and_acc, Replica

            dev = x.device if x.is_cuda else "cpu"
            log_loss_and_acc(loss_fn, Replica(0, dev, model, optimizer), val,
                             fused=fused_eval)
        if checkpoint_every and (step + 1) % checkpoint_every == 0 and rank == 0:
            from ..utils.checkpoint import save_checkpoint

            save_checkpoint(
                os.path.join(checkpoint_dir, f"ckpt_step{step + 1}.pt"),
                model, optimizer, step=step + 1,
            )

        # cooperative sentinel: stop only when ALL ranks vote stop
        if should_stop is not None:
            stop_flag.fill_(1 if should_stop(step) else 0)
            if dist.is_initialized():
                dist.all_reduce(stop_flag, op=dist.ReduceOp.MIN)
            if int(stop_flag.item()) == 1:
                log.info("rank %d: cooperative stop at step %d", rank, step)
                break

    return model, optimizer, {"timers": timers.summary(), "images_per_sec": thr.rate()}
