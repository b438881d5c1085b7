"""Cross-op state of one training step: every handshake between ops that
autograd cannot see, in one place. Sits below every other ops module and
below parallel/; imports nothing from the package. Who writes and reads
each piece, and its scope: docs/kernels.md, "Step state"."""

import threading

import torch
from torch.utils.weak import WeakIdKeyDictionary


_EPOCH = 0


def step_epoch() -> int:
    """Process-global counter of raw-kernel parameter updates. The fused
    optimizers write parameters through kernels that autograd version
    counters never see, and bump this after each such update. Three
    consumers (ops/arenas.py) compare it with the value they last saw:
      - the dgrad transposed-weight arena: are the transposes still fresh;
      - the wgrad workspace arena: has this backward epoch been zeroed yet;
      - the padded FC weights: do the pads need a refresh."""
    return _EPOCH


def bump_step_epoch() -> None:
    global _EPOCH
    _EPOCH += 1


# param -> its contiguous slice of a fused optimizer's flat G. Lets backward
# ops write gradients straight into the flat buffer (no AccumulateGrad
# kernel). Keyed weakly by identity: an entry goes when its parameter dies,
# so a new parameter at a recycled address can never alias a dead one's
# slice.
_FLAT = WeakIdKeyDictionary()


def register_flat_slice(param: torch.Tensor, G: torch.Tensor, offset: int,
                        numel: int) -> None:
    # the view is made once here, not per backward op
    _FLAT[param] = G[offset : offset + numel]


def flat_grad_slice(param):
    """Contiguous flat-G slice backing param.grad, or None."""
    return _FLAT.get(param)


# Backward ops that write gradients straight into the flat G bypass
# AccumulateGrad, so post-accumulate hooks never fire for them; they call
# notify_grad_written(param) instead. An attached GradBucketer subscribes.
_SUBSCRIBERS = []


def subscribe_grad_written(cb) -> None:
    _SUBSCRIBERS.append(cb)


def unsubscribe_grad_written(cb) -> None:
    if cb in _SUBSCRIBERS:
        _SUBSCRIBERS.remove(cb)


def has_grad_subscribers() -> bool:
    return bool(_SUBSCRIBERS)


def notify_grad_written(param) -> None:
    for cb in _SUBSCRIBERS:
        cb(param)


# Replica threads flag their backwards as non-deferrable (ops/gradflush.py).
# Autograd device workers inherit nothing from the launching thread, so the
# flag is a process-global count of open no_defer() blocks, not a
# thread-local.
_GATE_LOCK = threading.Lock()
_gate_depth = 0


class no_defer:
    """Context manager: direct-grad flushes stay per-layer immediate while
    any thread is inside one."""

    def __enter__(self):
        global _gate_depth
        with _GATE_LOCK:
            _gate_depth += 1

    def __exit__(self, *exc):
        global _gate_depth
        with _GATE_LOCK:
            _gate_depth -= 1


def deferral_ok() -> bool:
    return _gate_depth == 0


# Per-thread single-slot handshake: the conv fwd epilogue accumulates
# per-channel sum/sumsq of its (rounded) output; the immediately following
# BatchNorm on the SAME thread consumes them and skips its own stats read
# pass. Thread-local so task-DDP replica threads can't cross-feed; cleared
# at every conv forward so an unconsumed stash can't later match a
# recycled allocator pointer of the same shape.
_TLS = threading.local()


def stash_conv_stats(y, part):
    _TLS.conv_stats = (y.data_ptr(), tuple(y.shape), part)


def clear_conv_stats():
    _TLS.conv_stats = None


def take_conv_stats(x):
    ent = getattr(_TLS, "conv_stats", None)
    _TLS.conv_stats = None
    if ent is not None and ent[0] == x.data_ptr() and ent[1] == tuple(x.shape):
        return ent[2]
    return None


# Residual-junction grad stash: at an identity-shortcut junction the grad
# wrt x is dgrad(conv1) + gres(BN residual). When the block knows conv1's
# dgrad will run on the native kernel (models/resnet.py), the BN backward
# DEFERS gres here (returning None to autograd) and the conv dgrad folds
# it in via the kernel's += epilogue — autograd's separate
# CUDAFunctor_add pass over the full activation disappears.
# Thread-local (task-DDP replica threads), keyed by (data_ptr, shape) of
# the junction tensor; entries MUST be consumed by the very next dgrad of
# that tensor (backward visits bn2 ... conv1 strictly in order on the
# identity path), and an unconsumed entry is a loud error, never a silent
# gradient drop.


def stash_junction_gres(key, gres):
    d = getattr(_TLS, "junction", None)
    if d is None:
        d = _TLS.junction = {}
    if key in d:
        raise RuntimeError(
            "residual-junction gres stash collision: previous deferred "
            "gradient was never consumed by a conv dgrad (fusion contract "
            "broken — check models/resnet.py _junction_fusible gating)")
    d[key] = gres


def take_junction_gres(x):
    d = getattr(_TLS, "junction", None)
    if not d:
        return None
    return d.pop((x.data_ptr(), tuple(x.shape)), None)


def junction_stash_empty() -> bool:
    return not getattr(_TLS, "junction", None)
