"""Flat gradient sync on the GPU: the grad_mean_multi kernel, the reducer on
real gradients (direct and staged), and flat-mode training end to end.

The oracle everywhere is the definition itself in plain torch — a sequential
fp32 sum in replica order, one division, one cast — and the kernel must match
it bit for bit: the definition is order-fixed and atomic-free, so there is no
tolerance."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("GPU-only suite", allow_module_level=True)

from fluxdistributed_amd.models import build_model
from fluxdistributed_amd.ops import FusedSGDMomentum, logit_cross_entropy
from fluxdistributed_amd.ops.native import require_native
from fluxdistributed_amd.parallel import FlatGradReducer
from fluxdistributed_amd.parallel.task_ddp import prepare_training, train
from fluxdistributed_amd.utils.precision import to_mixed_bf16

DEV = "cuda:0"
SCALES = (1.0, 1e-3, 1e3)


def _oracle(g, dtype):
    """The definition, evaluated by torch on the CPU. Not on the GPU: ATen's
    device kernel for `tensor / python_scalar` multiplies by the reciprocal,
    which differs from the IEEE quotient in the last bit for R = 3 (seen on
    the first run of this file), whereas its CPU kernel divides."""
    acc = g[0].float().cpu().clone()
    for t in g[1:]:
        acc += t.float().cpu()
    return (acc / len(g)).to(dtype).to(g[0].device)


def _inputs(R, n, dtype, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(seed + 17 * R + n % 1000)
    return [(torch.randn(n, device=DEV, generator=gen)
             * SCALES[r % len(SCALES)]).to(dtype) for r in range(R)]


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    """Raw-value equality (torch.equal on floats would call NaN != NaN)."""
    return torch.equal(_bits(a), _bits(b))


# 8*256*3 + 64: three blocks of bf16 lanes plus a partial one; the last size
# is above one full sweep of the capped 4096 x 256 grid at 8 elements per
# lane, so the grid-stride loop runs its second, partial sweep.
SIZES = [64, 320, 8 * 256 * 3 + 64]
BIG = 4096 * 256 * 8 + 192


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("R,n", [(R, n) for R in (1, 2, 3, 16) for n in SIZES]
                         + [(2, BIG)])
def test_kernel_matches_definition(dtype, R, n):
    C = require_native("grad_mean_multi")
    g = _inputs(R, n, dtype)
    snap = [t.clone() for t in g]
    expect = _oracle(snap, dtype)
    C.grad_mean_multi(g)
    torch.cuda.synchronize()
    for r in range(R):
        assert _same(g[r], expect), f"replica {r} differs from the oracle"
    if R == 1:
        assert _same(g[0], snap[0]), "R=1 must be the identity"
    if R == 3 and dtype == torch.bfloat16 and n >= 320:
        # the scales make per-add bf16 rounding visible: the fold the tree
        # protocol does is a different number
        fold = ((snap[0] + snap[1]) + snap[2]) / 3
        assert not torch.equal(fold, expect)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
def test_nonfinite_flag(dtype):
    C = require_native("grad_mean_multi")
    n = 8 * 256 * 3 + 64
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)

    g = _inputs(3, n, dtype, seed=5)
    C.grad_mean_multi(g, flag)
    assert int(flag.item()) == 0, "flag raised on finite data"

    for pos, bad in ((n - 1, float("inf")), (0, float("nan"))):
        flag.zero_()
        g = _inputs(3, n, dtype, seed=6)
        g[1][pos] = bad
        expect = _oracle([t.clone() for t in g], dtype)
        C.grad_mean_multi(g, flag)
        assert int(flag.item()) == 1, f"{bad} at {pos} not flagged"
        keep = torch.ones(n, dtype=torch.bool, device=DEV)
        keep[pos] = False
        for r in range(3):
            assert not bool(torch.isfinite(g[r][pos]))
            assert torch.equal(g[r][keep], expect[keep]), r


# ---- reducer on real gradients: the recipe of test_task_ddp_gpu.py --------

def _model():
    torch.manual_seed(31)
    m = build_model("resnet18", num_classes=16, small_input=True)
    return to_mixed_bf16(m.to(memory_format=torch.channels_last)).train()


def _shards(step, n=2, devices=None):
    out = []
    for r in range(n):
        dev = devices[r] if devices else DEV
        g = torch.Generator().manual_seed(1000 + step * 10 + r)
        x = torch.randn(4, 3, 32, 32, generator=g).bfloat16().to(dev) \
            .contiguous(memory_format=torch.channels_last)
        y = torch.randint(0, 16, (4,), generator=g).to(dev)
        out.append((x, y))
    return out


def _sgd(m):
    return FusedSGDMomentum(m.parameters(), lr=0.05, momentum=0.9)


def _check_reducer_on_real_gradients(devices):
    """fwd+bwd on every replica once, snapshot each G; then for the direct
    and the staged reducer: restore the snapshots, reduce(), and compare
    every replica's G with the oracle of the snapshots, bit for bit."""
    st = prepare_training(_model(), None, devices, _sgd, grad_sync="flat")
    assert st.buffer == {}
    for r, (x, y) in zip(st.replicas, _shards(0, len(devices), devices)):
        with torch.cuda.device(r.device):
            r.optimizer.zero_grad()
            logit_cross_entropy(r.model(x), y).backward()
            torch.cuda.synchronize(r.device)
    groups = [r.optimizer.groups for r in st.replicas]
    host = groups[0][0].G.device
    snaps = [[g.G.clone() for g in gs] for gs in groups]
    expect = []
    for k in range(len(groups[0])):
        on_host = [s[k].to(host) for s in snaps]
        assert float(on_host[0].float().abs().max()) > 0, "no gradient"
        expect.append(_oracle(on_host, on_host[0].dtype))
    assert not _same(snaps[0][0], snaps[1][0]), "shards gave equal gradients"

    for force_stage in (False, True):
        red = FlatGradReducer(st.replicas, force_stage=force_stage)
        for gs, ss in zip(groups, snaps):
            for g, s in zip(gs, ss):
                g.G.copy_(s)
        for r in st.replicas:
            torch.cuda.synchronize(r.device)
        red.reduce()
        for r in st.replicas:
            torch.cuda.synchronize(r.device)
        for i, gs in enumerate(groups):
            for k, g in enumerate(gs):
                assert _same(g.G.to(host), expect[k]), \
                    f"force_stage={force_stage} replica {i} group {k}"
        assert red.pop_nonfinite() is False


@pytest.mark.parametrize("nrep", [2, 3])
def test_reducer_on_real_gradients(nrep):
    _check_reducer_on_real_gradients([DEV] * nrep)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs 2 GPUs")
def test_reducer_across_two_gpus():
    _check_reducer_on_real_gradients(["cuda:0", "cuda:1"])


def test_flat_training_end_to_end():
    st = prepare_training(_model(), None, [DEV, DEV], _sgd, grad_sync="flat")
    assert st.buffer == {}
    losses = []

    def loss_fn(out, y):
        loss = logit_cross_entropy(out, y)
        losses.append(loss.detach())
        return loss

    train(loss_fn, st, steps=3, batches=_shards, log_every=1, val_every=0)
    assert len(losses) == 6
    assert all(bool(torch.isfinite(l)) for l in losses), losses
    assert st.nonfinite_steps == 0
    assert st.cycles == 3 and st.num_missed == 0

    p0 = dict(st.replicas[0].model.named_parameters())
    p1 = dict(st.replicas[1].model.named_parameters())
    for k in p0:
        assert torch.equal(p0[k].float(), p1[k].float()), f"divergence in {k}"
        assert bool(torch.isfinite(p0[k].float()).all()), k

    # Sequential shard-average oracle of test_task_ddp_gpu.py: per-shard
    # grads on one model, averaged in fp32, one step. The 0.12 bound is that
    # test's: the two arms sample the wgrad/BN kernels' atomic fp32
    # accumulation order independently; it does not come from this kernel.
    solo = _model().to(DEV)
    opt = _sgd(solo)
    for step in range(3):
        shard_grads = []
        for (x, y) in _shards(step):
            opt.zero_grad()
            logit_cross_entropy(solo(x), y).backward()
            torch.cuda.synchronize()
            shard_grads.append([g.G.float().clone() for g in opt.groups])
        with torch.no_grad():
            for g, g0, g1 in zip(opt.groups, *shard_grads):
                g.G.copy_(((g0 + g1) / 2).to(g.G.dtype))
        opt.step()
    torch.cuda.synchronize()
    ps = dict(solo.named_parameters())
    for k in p0:
        a, b = p0[k].detach().float(), ps[k].detach().float()
        scale = float(b.abs().max())
        err = float((a - b).abs().max())
        assert err < 0.12 * max(scale, 1e-2), f"{k}: drift {err} scale {scale}"
