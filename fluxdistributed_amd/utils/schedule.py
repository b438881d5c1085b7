"""LR schedules as `sched(cycle)` callbacks for train()/drivers.

The reference's only schedule is dead code (test.jl:50: lr/5 every 10
cycles); provided here as a working helper plus the standard step/cosine.
"""

import math
from typing import Callable

import torch


def _set_lr(opt: torch.optim.Optimizer, lr: float):
    for g in opt.param_groups:
        g["lr"] = lr


def step_decay(opt, base_lr: float, factor: float = 0.2, every: int = 10) -> Callable[[int], None]:
    """reference test.jl:50 semantics: lr *= factor every `every` cycles."""

    def sched(cycle: int):
        _set_lr(opt, base_lr * (factor ** (cycle // every)))

    return sched


def warmup_poly_lr(cycle: int, base_lr: float, warmup_cycles: int,
                   total_cycles: int, power: float = 2.0,
                   min_lr: float = 0.0) -> float:
    """Linear ramp 0 -> base_lr over `warmup_cycles`, then
    min_lr + (base_lr - min_lr) * (1 - t)^power with t running 0 -> 1 from
    the end of warm-up to `total_cycles` (the LARS large-batch schedule)."""
    if cycle < warmup_cycles:
        return base_lr * cycle / warmup_cycles
    span = max(1, total_cycles - warmup_cycles)
    t = min((cycle - warmup_cycles) / span, 1.0)
    return min_lr + (base_lr - min_lr) * (1.0 - t) ** power


def warmup_poly(opt, base_lr: float, warmup_cycles: int, total_cycles: int,
                power: float = 2.0, min_lr: float = 0.0) -> Callable[[int], float]:
    """`sched(cycle)` sets and returns warmup_poly_lr(cycle, ...). An
    optimizer with a device-side learning rate (`set_lr`, FusedLARS) gets it
    written there as well, so the next replay of a captured step uses it."""

    def sched(cycle: int):
        lr = warmup_poly_lr(cycle, base_lr, warmup_cycles, total_cycles,
                            power, min_lr)
        _set_lr(opt, lr)
        if hasattr(opt, "set_lr"):
            opt.set_lr(lr)
        return lr

    return sched


def cosine(opt, base_lr: float, total_cycles: int, min_lr: float = 0.0) -> Callable[[int], None]:
    def sched(cycle: int):
        t = min(cycle / max(1, total_cycles), 1.0)
        _set_lr(opt, min_lr + 0.5 * (base_lr - min_lr) * (1 + math.cos(math.pi * t)))

    return sched
