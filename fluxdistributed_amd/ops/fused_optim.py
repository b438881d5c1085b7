"""Fused flat-buffer optimizers (reference: the Optimisers.jl Momentum/ADAM
updates applied leaf-wise at /root/reference/src/ddp_tasks.jl:168 and
src/overloads.jl:1-12 — here re-designed MI355X-first).

Instead of ~110 per-leaf elementwise launches, all parameters live in ONE
contiguous flat buffer per (device, dtype) group:

  P (param dtype, what the model computes with)
  G (param dtype, gradients — autograd accumulates into views of it, so a
     data-parallel all-reduce is a single flat collective over G)
  M (fp32 master copy, only when P is low precision)
  V/S (fp32 optimizer state)

One kernel launch updates the whole model (~22M elems for ResNet-34): pure
HBM-bound streaming, vectorized 16B/lane (guide Appendix B elementwise).
"""

from typing import List

import torch

from .native import require_native
from .step_state import bump_step_epoch, register_flat_slice


class _FlatGroup:
    """All parameters of one (device, dtype) flattened into shared storage."""

    ALIGN = 64  # elements; keeps every param slice 128B-aligned for vector IO

    def __init__(self, params: List[torch.nn.Parameter]):
        self.params = params
        dev, dt = params[0].device, params[0].dtype
        self.device, self.dtype = dev, dt
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.offsets, self.numel = offs, total
        self.P = torch.zeros(total, device=dev, dtype=dt)
        self.G = torch.zeros(total, device=dev, dtype=dt)
        for p, off in zip(params, offs):
            # Rebind: the Parameter stays a leaf; its storage is now the flat
            # buffer. channels_last params keep their physical layout.
            v = self._view_like(self.P, off, p.data)
            v.copy_(p.data)
            p.data = v
            p.grad = self._view_like(self.G, off, p.data)
            register_flat_slice(p, self.G, off, p.numel())
        self.master = self.P.float() if dt != torch.float32 else None

    @staticmethod
    def _view_like(flat, off, like):
        v = flat[off : off + like.numel()]
        if like.is_contiguous(memory_format=torch.channels_last) and like.dim() == 4 \
                and not like.is_contiguous():
            return v.view(like.shape[0], like.shape[2], like.shape[3], like.shape[1]) \
                .permute(0, 3, 1, 2)
        return v.view(like.shape)

    def grad_views(self):
        return [p.grad for p in self.params]


def _flatten_param_groups(params) -> List[_FlatGroup]:
    params = [p for p in params if p.requires_grad]
    if not params:
        return []
    by_key = {}
    for p in params:
        by_key.setdefault((p.device, p.dtype), []).append(p)
    return [_FlatGroup(ps) for ps in by_key.values()]


class _FlatOptimizer(torch.optim.Optimizer):
    """Base: flattens params, exposes flat G for DDP, state_dict round-trips."""

    def __init__(self, params, defaults):
        params = list(params)
        super().__init__(params, defaults)
        flat_params = [p for g in self.param_groups for p in g["params"]]
        self.groups = _flatten_param_groups(flat_params)

    @torch.no_grad()
    def zero_grad(self, set_to_none: bool = False):
        # set_to_none must stay False: autograd accumulates into the flat views.
        for g in self.groups:
            g.G.zero_()

    def flat_grads(self) -> List[torch.Tensor]:
        return [g.G for g in self.groups]

    @torch.no_grad()
    def refresh_master(self):
        """Re-seed fp32 masters from current (possibly just-loaded) params."""
        for g in self.groups:
            if g.master is not None:
                g.master.copy_(g.P.float())

    def state_dict(self):
        d = super().state_dict()
        d["flat_state"] = [
            {
                "master": (g.master.clone() if g.master is not None else None),
                **{k: v.clone() for k, v in self._flat_buffers(g).items()},
            }
            for g in self.groups
        ]
        return d

    def load_state_dict(self, d):
        flat = d.pop("flat_state", None)
        super().load_state_dict(d)
        if flat is not None:
            for g, s in zip(self.groups, flat):
                if g.master is not None and s["master"] is not None:
                    g.master.copy_(s["master"])
                for k, v in self._flat_buffers(g).items():
                    v.copy_(s[k])

    def _flat_buffers(self, g):  # pragma: no cover - overridden
        return {}


class FusedSGDMomentum(_FlatOptimizer):
    """SGD with (heavy-ball) momentum — reference flagship optimizer
    Momentum(0.01, 0.9) (/root/reference/README.md:37-38)."""

    def __init__(self, params, lr=0.01, momentum=0.9, weight_decay=0.0, nesterov=False):
        super().__init__(params, dict(lr=lr, momentum=momentum,
                                      weight_decay=weight_decay, nesterov=nesterov))
        for g in self.groups:
            g.V = torch.zeros(g.numel, device=g.device, dtype=torch.float32)

    def _flat_buffers(self, g):
        return {"V": g.V}

    @torch.no_grad()
    def step(self, closure=None):
        hp = self.param_groups[0]
        lr, mom, wd = hp["lr"], hp["momentum"], hp["weight_decay"]
        nesterov = hp["nesterov"]
        for g in self.groups:
            if g.P.is_cuda:
                C = require_native("fused_sgd")
                C.sgd_step(g.P, g.G, g.master if g.master is not None else g.P,
                           g.V, lr, mom, wd, nesterov)
                bump_step_epoch()
            else:
                master = g.master if g.master is not None else g.P
                grad = g.G.float()
                if wd:
                    grad = grad.add(master, alpha=wd)
                g.V.mul_(mom).add_(grad)
                upd = grad.add(g.V, alpha=mom) if nesterov else g.V
                master.add_(upd, alpha=-lr)
                if g.master is not None:
                    g.P.copy_(master.to(g.dtype))
        return None


class FusedAdam(_FlatOptimizer):
    """Adam — reference process-DDP optimizer (/root/reference/bin/driver.jl:27)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        for g in self.groups:
            g.V = torch.zeros(g.numel, device=g.device, dtype=torch.float32)  # m1
            g.S = torch.zeros(g.numel, device=g.device, dtype=torch.float32)  # m2
        self._step = 0

    def _flat_buffers(self, g):
        return {"V": g.V, "S": g.S}

    @torch.no_grad()
    def step(self, closure=None):
        hp = self.param_groups[0]
        lr, (b1, b2), eps, wd = hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"]
        self._step += 1
        bc1 = 1.0 - b1 ** self._step
        bc2 = 1.0 - b2 ** self._step
        for g in self.groups:
            if g.P.is_cuda:
                C = require_native("fused_adam")
                C.adam_step(g.P, g.G, g.master if g.master is not None else g.P,
                            g.V, g.S, lr, b1, b2, eps, wd, bc1, bc2)
                bump_step_epoch()
            else:
                master = g.master if g.master is not None else g.P
                grad = g.G.float()
                if wd:
                    grad = grad.add(master, alpha=wd)
                g.V.mul_(b1).add_(grad, alpha=1 - b1)
                g.S.mul_(b2).addcmul_(grad, grad, value=1 - b2)
                denom = (g.S / bc2).sqrt_().add_(eps)
                master.addcdiv_(g.V / bc1, denom, value=-lr)
                if g.master is not None:
                    g.P.copy_(master.to(g.dtype))
        return None

    def state_dict(self):
        d = super().state_dict()
        d["step_count"] = self._step
        return d

    def load_state_dict(self, d):
        self._step = d.pop("step_count", 0)
        super().load_state_dict(d)


def _own_device(opt: _FlatOptimizer):
    devs = {g.device for g in opt.groups}
    if len(devs) != 1:
        raise ValueError(
            "the segment kernels fold all flat groups in one launch: every "
            f"parameter must live on one device, got {sorted(map(str, devs))}")
    return next(iter(devs))


class _SegmentPlan:
    """Device tables and scratch of the segmented-norm kernels (csrc/lars.hip)
    for one flat optimizer: one segment per parameter, numbered over the
    groups in group order, then parameter order. Built once, uploaded once."""

    def __init__(self, opt: _FlatOptimizer, flags: List[int]):
        C = require_native("lars")
        dev = _own_device(opt)
        self.S = sum(len(g.params) for g in opt.groups)
        assert len(flags) == self.S
        tables, seg_rows, base = [], [], 0
        for g in opt.groups:
            t = C.lars_plan(list(g.offsets), [p.numel() for p in g.params],
                            g.numel, len(seg_rows))
            for p in g.params:
                k = -(-p.numel() // C.LARS_CHUNK)
                seg_rows.append([base, base + k, flags[len(seg_rows)]])
                base += k
            tables.append(t)
        self.total_chunks = base
        self.chunk_bases, b = [], 0
        for t in tables:
            self.chunk_bases.append(b)
            b += t.shape[0]
        self.tables = [t.to(dev) for t in tables]
        self.seg_meta = torch.tensor(seg_rows, dtype=torch.int32) \
            .reshape(self.S, 3).to(dev)
        self.partials = torch.zeros(2 * base, device=dev, dtype=torch.float64)
        self.coef = torch.zeros(self.S, device=dev, dtype=torch.float32)
        self.stats = torch.zeros(2 + 2 * self.S, device=dev,
                                 dtype=torch.float32)

    def norms_and_fold(self, opt, lr_t, skipped, eta, wd, eps, max_grad_norm):
        C = require_native("lars")
        for g, t, cb in zip(opt.groups, self.tables, self.chunk_bases):
            C.lars_norms(g.P, g.G, g.master if g.master is not None else g.P,
                         t, self.partials, cb, self.total_chunks, self.S)
        C.lars_fold(self.partials, self.seg_meta, lr_t, self.coef, self.stats,
                    skipped, eta, wd, eps, max_grad_norm)


def _segments(opt: _FlatOptimizer):
    """(group, offset, numel, param) of every segment, in segment order."""
    return [(g, off, p.numel(), p) for g in opt.groups
            for p, off in zip(g.params, g.offsets)]


class FusedLARS(_FlatOptimizer):
    """Momentum SGD with layer-wise trust ratios (LARS), global-norm clipping
    and a skip rule for non-finite gradients, on the flat buffers. Segment s
    is one parameter; with w the fp32 master (else P), g the gradient as fp32
    and v the momentum:

      W_s = sum w^2, G_s = sum g^2;  gnorm = sqrt(sum_s G_s)
      clip = min(1, max_grad_norm / (gnorm + 1e-6)) if max_grad_norm > 0 else 1
      wn = sqrt(W_s), gn = clip sqrt(G_s), wd_s = weight_decay if decay_s else 0
      trust_s = eta wn / (gn + wd_s wn + eps) if adapt_s and wn > 0 and gn > 0
                else 1
      u = clip g + wd_s w;  v <- momentum v + lr trust_s u;  w <- w - v

    A non-finite gnorm leaves P, master and v untouched and bumps a device
    counter. adapt_s and decay_s are both false for parameters `exclude(p)`
    selects: by default those with ndim <= 1 (BN scales and biases, FC bias).

    On the GPU a step is 2 launches per flat group and one fold launch
    (csrc/lars.hip), none of which synchronizes. lr lives in a device scalar
    the fold kernel reads, so a captured step follows `set_lr` between
    replays; momentum, weight_decay, eta, eps and max_grad_norm are kernel
    arguments and baked into a capture.
    """

    def __init__(self, params, lr=0.1, momentum=0.9, weight_decay=5e-5,
                 eta=1e-3, eps=1e-9, max_grad_norm=0.0, exclude=None):
        super().__init__(params, dict(lr=lr, momentum=momentum,
                                      weight_decay=weight_decay, eta=eta,
                                      eps=eps, max_grad_norm=max_grad_norm))
        if exclude is None:
            exclude = lambda p: p.ndim <= 1  # noqa: E731
        for g in self.groups:
            g.V = torch.zeros(g.numel, device=g.device, dtype=torch.float32)
        # bit 0 = adapt, bit 1 = decay
        self.seg_flags = [0 if exclude(p) else 3
                          for _, _, _, p in _segments(self)]
        dev = _own_device(self) if self.groups else torch.device("cpu")
        self._lr_t = torch.full((1,), float(lr), device=dev,
                                dtype=torch.float32)
        self._lr_written = float(lr)
        self._skipped = torch.zeros(1, device=dev, dtype=torch.int32)
        self._gnorm = torch.zeros((), device=dev, dtype=torch.float32)
        self._plan = None
        if dev.type == "cuda":
            self._plan = _SegmentPlan(self, self.seg_flags)
            self._gnorm = self._plan.stats[0]

    def _flat_buffers(self, g):
        return {"V": g.V}

    @torch.no_grad()
    def set_lr(self, lr: float):
        """Set the learning rate, in param_groups and in the device scalar
        the kernels read. Call between graph replays, not inside a capture."""
        for pg in self.param_groups:
            pg["lr"] = lr
        self._lr_t.fill_(float(lr))
        self._lr_written = float(lr)

    def last_grad_norm(self) -> torch.Tensor:
        """gnorm of the latest step as a 0-d device tensor; no synchronize."""
        return self._gnorm

    def skipped_steps(self) -> int:
        """Steps skipped for a non-finite gradient norm. Synchronizes."""
        return int(self._skipped.item())

    @torch.no_grad()
    def step(self, closure=None):
        hp = self.param_groups[0]
        if not self.groups:
            return None
        on_gpu = self._plan is not None
        if float(hp["lr"]) != self._lr_written and not (
                on_gpu and torch.cuda.is_current_stream_capturing()):
            self.set_lr(hp["lr"])
        if not on_gpu:
            self._step_reference(hp)
            return None
        C = require_native("lars")
        plan = self._plan
        plan.norms_and_fold(self, self._lr_t, self._skipped, hp["eta"],
                            hp["weight_decay"], hp["eps"],
                            hp["max_grad_norm"])
        for g, t in zip(self.groups, plan.tables):
            C.lars_step(g.P, g.G, g.master if g.master is not None else g.P,
                        g.V, t, plan.seg_meta, plan.coef, plan.stats,
                        hp["momentum"], hp["weight_decay"])
        bump_step_epoch()
        return None

    def _step_reference(self, hp):
        """The definition in plain torch (CPU): sums and trust ratios in
        fp64, the per-element update in fp32 as the kernel does it."""
        segs = _segments(self)
        w_of = lambda g: g.master if g.master is not None else g.P  # noqa: E731
        W = torch.stack([w_of(g)[o:o + n].double().square().sum()
                         for g, o, n, _ in segs])
        G = torch.stack([g.G[o:o + n].double().square().sum()
                         for g, o, n, _ in segs])
        gnorm = G.sum().sqrt().float()
        self._gnorm.copy_(gnorm)
        if not torch.isfinite(gnorm):
            self._skipped += 1
            return
        mgn = hp["max_grad_norm"]
        clip = torch.ones((), dtype=torch.float32)
        if mgn > 0:
            clip = torch.clamp(mgn / (gnorm.double() + 1e-6), max=1.0).float()
        lr = self._lr_t.double()[0]
        for s, (g, o, n, _) in enumerate(segs):
            adapt, decay = self.seg_flags[s] & 1, self.seg_flags[s] & 2
            wds = hp["weight_decay"] if decay else 0.0
            wn, gn = W[s].sqrt(), clip.double() * G[s].sqrt()
            trust = torch.ones((), dtype=torch.float64)
            if adapt and wn > 0 and gn > 0:
                trust = hp["eta"] * wn / (gn + wds * wn + hp["eps"])
            coef = (lr * trust).float()
            w, v = w_of(g)[o:o + n], g.V[o:o + n]
            u = clip * g.G[o:o + n].float()
            if wds:
                u = u.add(w, alpha=wds)
            v.mul_(hp["momentum"]).add_(coef * u)
            w.sub_(v)
            if g.master is not None:
                g.P[o:o + n].copy_(w.to(g.dtype))

    def state_dict(self):
        d = super().state_dict()
        d["skipped_steps"] = self.skipped_steps()
        return d

    def load_state_dict(self, d):
        self._skipped.fill_(int(d.pop("skipped_steps", 0)))
        super().load_state_dict(d)
        self._lr_written = None     # param_groups may carry another lr


@torch.no_grad()
def flat_grad_norm(optimizer: _FlatOptimizer):
    """Global gradient norm (0-d tensor) and per-parameter gradient norms
    (1-D, in segment order: groups, then parameters) of any flat optimizer,
    on its device and without a host synchronize. On the GPU this is the
    LARS norms pass and fold over G (csrc/lars.hip); the plan is built on
    first use and cached on the optimizer, whose buffers are only read."""
    segs = _segments(optimizer)
    if not segs:
        return torch.zeros(()), torch.zeros(0)
    if not optimizer.groups[0].P.is_cuda:
        G = torch.stack([g.G[o:o + n].double().square().sum()
                         for g, o, n, _ in segs])
        return G.sum().sqrt().float(), G.sqrt().float()
    cache = getattr(optimizer, "_grad_norm_plan", None)
    if cache is None:
        plan = _SegmentPlan(optimizer, [0] * len(segs))
        dev = plan.stats.device
        cache = (plan, torch.zeros(1, device=dev, dtype=torch.float32),
                 torch.zeros(1, device=dev, dtype=torch.int32))
        optimizer._grad_norm_plan = cache
    plan, lr_t, scratch_count = cache
    plan.norms_and_fold(optimizer, lr_t, scratch_count, 0.0, 0.0, 0.0, 0.0)
    return plan.stats[0].clone(), plan.stats[2 + plan.S:].sqrt()
