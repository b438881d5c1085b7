"""FusedLARS on the GPU: the three kernels of csrc/lars.hip against the fp64
definition (docs/training.md, "Large-batch training"), reproducibility, the
skip rule, the untrusted-table guard, the optimizer against its CPU
fallback, graph replay under a schedule, and flat_grad_norm.

Shapes are the smallest at which each mechanism can break: a mask inside the
only vector (10), one aligned unit (64), a mask in the second vector (77),
one full chunk, a second chunk of one element, several chunks with a ragged
tail, the CIFAR stem weight, and more segments than the fold block has
threads (300 more of 64 elements)."""

import copy
import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("GPU-only suite", allow_module_level=True)

from fluxdistributed_amd.models import build_model
from fluxdistributed_amd.ops import (
    FusedLARS, FusedSGDMomentum, flat_grad_norm, logit_cross_entropy,
)
from fluxdistributed_amd.ops.native import require_native
from fluxdistributed_amd.utils.precision import to_mixed_bf16

DEV = torch.device("cuda:0")
F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
CH = require_native("lars").LARS_CHUNK
NUMELS = [10, 64, 77, CH, CH + 1, 3 * CH + 520, 1728] + [64] * 300
S = len(NUMELS)
HP = dict(lr=0.25, momentum=0.9, weight_decay=1e-2, eta=0.02, eps=1e-9)
# A lane adds at most CHUNK/256 fp32 squares before everything is double:
# a relative error of about CHUNK/256 * 2^-24 (1e-6 at CHUNK = 4096).
assert CH // 256 * 2.0 ** -24 < 1e-5
RTOL = 1e-5


def excluded(i):
    return i % 3 == 1      # neither adapted nor decayed


def make_opt(dtype, cls=FusedLARS, **kw):
    gen = torch.Generator().manual_seed(3)
    params = [nn.Parameter((torch.randn(n, generator=gen) * 0.1)
                           .to(dtype).to(DEV)) for n in NUMELS]
    if cls is FusedLARS:
        skip = {id(p) for i, p in enumerate(params) if excluded(i)}
        kw = dict(HP, exclude=lambda p: id(p) in skip, **kw)
    opt = cls(params, **kw)
    g = opt.groups[0]
    # gradients scaled per segment by 1e-3, 1, 1e3; momentum not zero
    for i, p in enumerate(params):
        p.grad.copy_(torch.randn(p.numel(), generator=gen)
                     * 10.0 ** (3 * (i % 3 - 1)))
        g.V[g.offsets[i]:g.offsets[i] + p.numel()] = \
            (torch.randn(p.numel(), generator=gen) * 1e-3).to(DEV)
    return opt


def buffers(opt):
    g = opt.groups[0]
    return {"P": g.P, "V": g.V, **({"M": g.master} if g.master is not None
                                   else {})}


def snapshot(opt):
    return {k: v.clone() for k, v in buffers(opt).items()}


def restore(opt, snap):
    for k, v in buffers(opt).items():
        v.copy_(snap[k])


def assert_bits_equal(opt, snap):
    for k, v in buffers(opt).items():
        a, b = v.view(torch.uint8), snap[k].view(torch.uint8)
        assert torch.equal(a, b), f"{k} changed"


def outputs(opt):
    torch.cuda.synchronize()
    out = snapshot(opt)
    out.update(stats=opt._plan.stats.clone(), coef=opt._plan.coef.clone(),
               partials=opt._plan.partials.clone(),
               skipped=opt._skipped.clone())
    return out


def own_mask(opt):
    g = opt.groups[0]
    own = torch.zeros(g.numel, dtype=torch.bool, device=DEV)
    for p, off in zip(g.params, g.offsets):
        own[off:off + p.numel()] = True
    return own


def per_element(opt, values):
    """values[s] spread over segment s's padded slot in the flat buffer."""
    g = opt.groups[0]
    ends = list(g.offsets[1:]) + [g.numel]
    lens = torch.tensor([e - o for o, e in zip(g.offsets, ends)], device=DEV)
    return torch.repeat_interleave(values.to(DEV), lens)


@pytest.fixture(scope="module", params=[BF, F32], ids=["bf16_master", "fp32"])
def stepped(request):
    """One step on the hand-made layout, with clipping active; inputs and
    outputs are kept for the tests below and never modified."""
    opt = make_opt(request.param)
    g = opt.groups[0]
    w0 = (g.master if g.master is not None else g.P).clone()
    before = snapshot(opt)
    gnorm = float(g.G.double().square().sum().sqrt())
    opt.param_groups[0]["max_grad_norm"] = 0.3 * gnorm
    opt.step()
    return dict(opt=opt, w0=w0, g0=g.G.clone(), before=before,
                out=outputs(opt), max_grad_norm=0.3 * gnorm)


def test_sums_and_global_norm_match_fp64(stepped):
    opt, out = stepped["opt"], stepped["out"]
    g = opt.groups[0]
    w, gr = stepped["w0"].double(), stepped["g0"].double()
    W = torch.stack([w[o:o + n].square().sum()
                     for o, n in zip(g.offsets, NUMELS)])
    G = torch.stack([gr[o:o + n].square().sum()
                     for o, n in zip(g.offsets, NUMELS)])
    stats = out["stats"].double()
    print("max rel err W", float(((stats[2:2 + S] - W) / W).abs().max()),
          "G", float(((stats[2 + S:] - G) / G).abs().max()),
          "gnorm", float((stats[0] - G.sum().sqrt()).abs() / G.sum().sqrt()))
    assert torch.allclose(stats[2:2 + S], W, rtol=RTOL, atol=0)
    assert torch.allclose(stats[2 + S:], G, rtol=RTOL, atol=0)
    assert torch.allclose(stats[0], G.sum().sqrt(), rtol=RTOL, atol=0)


def test_coef_matches_fp64_definition(stepped):
    opt, out = stepped["opt"], stepped["out"]
    g = opt.groups[0]
    w, gr = stepped["w0"].double(), stepped["g0"].double()
    gnorm = math.sqrt(float(gr.square().sum()))
    clip = min(1.0, stepped["max_grad_norm"] / (gnorm + 1e-6))
    assert clip < 0.31
    want = []
    for i, (o, n) in enumerate(zip(g.offsets, NUMELS)):
        wn = math.sqrt(float(w[o:o + n].square().sum()))
        gn = clip * math.sqrt(float(gr[o:o + n].square().sum()))
        wds = 0.0 if excluded(i) else HP["weight_decay"]
        trust = 1.0 if excluded(i) else \
            HP["eta"] * wn / (gn + wds * wn + HP["eps"])
        want.append(HP["lr"] * trust)
    want = torch.tensor(want, dtype=F64, device=DEV)
    assert want.max() / want.min() > 1e4     # trust ratios orders apart
    assert torch.allclose(out["stats"][1].double(),
                          torch.tensor(clip, dtype=F64, device=DEV),
                          rtol=RTOL, atol=0)
    assert torch.allclose(out["coef"].double(), want, rtol=RTOL, atol=0)


def test_update_matches_rule_4(stepped):
    opt, out, before = stepped["opt"], stepped["out"], stepped["before"]
    clip, coef = out["stats"][1], out["coef"]
    decay = torch.tensor([0.0 if excluded(i) else HP["weight_decay"]
                          for i in range(S)])
    cf, wd = per_element(opt, coef), per_element(opt, decay)
    w0 = stepped["w0"].float()
    u = clip * stepped["g0"].float() + wd * w0
    v = HP["momentum"] * before["V"] + cf * u
    w = w0 - v
    assert torch.allclose(out["V"], v, rtol=1e-5, atol=1e-6)
    got_w = out["M"] if "M" in out else out["P"]
    assert torch.allclose(got_w, w, rtol=1e-5, atol=1e-6)
    assert not torch.equal(got_w, stepped["w0"])
    if "M" in out:
        assert torch.equal(out["P"].view(torch.int16),
                           out["M"].to(BF).view(torch.int16))


def test_padding_still_zero(stepped):
    opt, out = stepped["opt"], stepped["out"]
    pad = ~own_mask(opt)
    assert int(pad.sum()) > 0
    for k in buffers(opt):
        assert (out[k][pad] == 0).all(), k


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16_master", "fp32"])
def test_two_runs_are_bit_identical(dtype):
    runs = []
    for _ in range(2):
        opt = make_opt(dtype, max_grad_norm=1.0)
        opt.step()
        runs.append(outputs(opt))
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(torch.uint8),
                           runs[1][k].view(torch.uint8)), k


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16_master", "fp32"])
def test_non_finite_gradient_skips_the_step(dtype):
    opt = make_opt(dtype)
    g = opt.groups[0]
    before = snapshot(opt)
    g.G[g.offsets[5] + NUMELS[5] // 2] = float("inf")
    opt.step()
    torch.cuda.synchronize()
    assert_bits_equal(opt, before)
    assert opt.skipped_steps() == 1
    assert math.isinf(float(opt.last_grad_norm()))
    g.G[g.offsets[5] + NUMELS[5] // 2] = 1.0
    g.G[g.offsets[0] + 9] = float("nan")
    opt.step()
    torch.cuda.synchronize()
    assert_bits_equal(opt, before)
    assert opt.skipped_steps() == 2
    # and a finite gradient steps again
    g.G[g.offsets[0] + 9] = 1.0
    opt.step()
    assert opt.skipped_steps() == 2
    assert not torch.equal(g.P, before["P"])


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16_master", "fp32"])
def test_untrusted_table_row_becomes_a_skipped_step(dtype):
    """A row naming segment S: the norms block writes NaN partials and the
    step block returns, neither reads anything through the row."""
    opt = make_opt(dtype)
    before = snapshot(opt)
    table = opt._plan.tables[0].clone()
    row = 8                       # inside the several-chunk segment
    assert int(table[row, 0]) == 5
    table[row, 0] = S
    opt._plan.tables[0] = table
    opt.step()
    torch.cuda.synchronize()
    assert_bits_equal(opt, before)
    assert opt.skipped_steps() == 1
    assert math.isnan(float(opt.last_grad_norm()))
    assert torch.isnan(opt._plan.partials[2 * row:2 * row + 2]).all()
    assert torch.isfinite(opt._plan.partials[:2 * row]).all()


def test_optimizer_matches_cpu_fallback():
    """ResNet-18 mixed bf16, 3 steps; the CPU optimizer gets the GPU run's
    gradients, so only the optimizers are compared."""
    torch.manual_seed(11)
    base = build_model("resnet18", num_classes=8, small_input=True) \
        .to(memory_format=torch.channels_last)
    mg = to_mixed_bf16(copy.deepcopy(base).to(DEV)).train()
    mc = to_mixed_bf16(copy.deepcopy(base)).train()
    hp = dict(lr=0.2, momentum=0.9, weight_decay=1e-3, eta=0.02,
              max_grad_norm=5.0)
    og, oc = FusedLARS(mg.parameters(), **hp), FusedLARS(mc.parameters(), **hp)
    assert [g.dtype for g in og.groups] == [g.dtype for g in oc.groups]
    assert len(og.groups) == 2
    gen = torch.Generator().manual_seed(5)
    for _ in range(3):
        x = torch.randn(4, 3, 32, 32, generator=gen).bfloat16().to(DEV) \
            .contiguous(memory_format=torch.channels_last)
        y = torch.randint(0, 8, (4,), generator=gen).to(DEV)
        og.zero_grad()
        logit_cross_entropy(mg(x), y).backward()
        for a, b in zip(og.groups, oc.groups):
            b.G.copy_(a.G)
        og.step()
        oc.step()
    assert og.skipped_steps() == 0 and oc.skipped_steps() == 0
    assert float(og.last_grad_norm()) == pytest.approx(
        float(oc.last_grad_norm()), rel=1e-5)
    for a, b in zip(og.groups, oc.groups):
        wa = a.master if a.master is not None else a.P
        wb = b.master if b.master is not None else b.P
        assert torch.allclose(wa.cpu(), wb, rtol=1e-5, atol=1e-6)
        assert torch.allclose(a.V.cpu(), b.V, rtol=1e-5, atol=1e-6)


def test_graph_replay_follows_set_lr():
    lr_a, lr_b = 0.25, 0.0625
    opt = make_opt(BF, max_grad_norm=1.0)
    assert opt.param_groups[0]["lr"] == lr_a
    # warm-up on a side stream, then a single-stream capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            opt.step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    start = snapshot(opt)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()

    restore(opt, start)
    opt.set_lr(lr_b)
    graph.replay()
    torch.cuda.synchronize()
    replayed = snapshot(opt)

    eager = {}
    for lr in (lr_b, lr_a):
        restore(opt, start)
        opt.set_lr(lr)
        opt.step()
        torch.cuda.synchronize()
        eager[lr] = snapshot(opt)
    for k in replayed:
        assert torch.equal(replayed[k].view(torch.uint8),
                           eager[lr_b][k].view(torch.uint8)), k
    assert not torch.equal(replayed["V"], eager[lr_a]["V"])
    assert not torch.equal(replayed["P"], eager[lr_a]["P"])


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16_master", "fp32"])
def test_flat_grad_norm(dtype):
    opt = make_opt(dtype, cls=FusedSGDMomentum, lr=0.1, momentum=0.9)
    g = opt.groups[0]
    before = snapshot(opt)
    g0 = g.G.clone()
    total, per = flat_grad_norm(opt)
    total2, _ = flat_grad_norm(opt)          # the cached plan
    gd = g.G.double()
    want = torch.stack([gd[o:o + n].square().sum().sqrt()
                        for o, n in zip(g.offsets, NUMELS)])
    assert total.dim() == 0 and per.shape == (S,) and total.is_cuda
    assert torch.allclose(total.double(), gd.square().sum().sqrt(),
                          rtol=RTOL, atol=0)
    assert torch.allclose(per.double(), want, rtol=RTOL, atol=0)
    assert torch.equal(total, total2)
    assert_bits_equal(opt, before)
    assert torch.equal(g.G, g0)
