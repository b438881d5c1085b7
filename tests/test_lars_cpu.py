"""FusedLARS without a GPU: the plain-torch fallback against an fp64
evaluation of the definition (docs/training.md, "Large-batch training"), the
special cases, the host chunk plan, the bindings' refusals, flat_grad_norm,
checkpoints and the warm-up schedule."""

import math

import pytest
import torch
import torch.nn as nn

from fluxdistributed_amd.ops import (
    FusedLARS, FusedSGDMomentum, flat_grad_norm,
)
from fluxdistributed_amd.ops.native import load_native
from fluxdistributed_amd.utils.checkpoint import load_checkpoint, save_checkpoint
from fluxdistributed_amd.utils.schedule import warmup_poly

F32, BF, I32, F64 = torch.float32, torch.bfloat16, torch.int32, torch.float64

# numels 10, 64, 77, 1728, 4096, 4097, 12808: 1-D, 2-D and 4-D, so the
# default rule (ndim <= 1 is neither adapted nor decayed) splits them
SHAPES = [(10,), (64,), (77,), (64, 3, 3, 3), (64, 64), (4097,), (8, 1601)]
HP = dict(lr=0.5, momentum=0.9, weight_decay=1e-2, eta=0.02, eps=1e-9,
          max_grad_norm=0.0)


def make_params(seed=0, dtype=F32, zero=()):
    gen = torch.Generator().manual_seed(seed)
    ps = []
    for i, s in enumerate(SHAPES):
        w = torch.randn(*s, generator=gen) * (0.1 if len(s) > 1 else 1.0)
        if i in zero:
            w.zero_()
        ps.append(nn.Parameter(w.to(dtype)))
    return ps


def make_grads(seed, scale=1.0, zero=()):
    gen = torch.Generator().manual_seed(1000 + seed)
    gs = [torch.randn(*s, generator=gen) * scale * 10.0 ** (i % 3 - 1)
          for i, s in enumerate(SHAPES)]
    for i in zero:
        gs[i].zero_()
    return gs


def set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad.copy_(g)


def definition_fp64(w, v, g, hp, adapt, decay):
    """One step of the definition on lists of fp64 tensors, in place.
    Returns (gnorm, clip, trust per segment); a non-finite gnorm changes
    nothing."""
    G = [float((x * x).sum()) for x in g]
    gnorm = math.sqrt(sum(G))
    if not math.isfinite(gnorm):
        return gnorm, None, None
    clip = 1.0
    if hp["max_grad_norm"] > 0:
        clip = min(1.0, hp["max_grad_norm"] / (gnorm + 1e-6))
    trusts = []
    for s in range(len(w)):
        wds = hp["weight_decay"] if decay[s] else 0.0
        wn = math.sqrt(float((w[s] * w[s]).sum()))
        gn = clip * math.sqrt(G[s])
        trust = 1.0
        if adapt[s] and wn > 0 and gn > 0:
            trust = hp["eta"] * wn / (gn + wds * wn + hp["eps"])
        trusts.append(trust)
        u = clip * g[s] + wds * w[s]
        v[s].mul_(hp["momentum"]).add_(hp["lr"] * trust * u)
        w[s].sub_(v[s])
    return gnorm, clip, trusts


def default_flags():
    f = [len(s) > 1 for s in SHAPES]
    return f, f


def run_both(hp, steps=3, zero_w=(), zero_g=(), exclude=None, flags=None):
    params = make_params(zero=zero_w)
    opt = FusedLARS(params, exclude=exclude, **hp)
    w = [p.detach().double().clone() for p in params]
    v = [torch.zeros_like(x) for x in w]
    adapt, decay = flags or default_flags()
    trusts = None
    for k in range(steps):
        grads = make_grads(k, zero=zero_g)
        set_grads(params, grads)
        opt.step()
        _, _, trusts = definition_fp64(w, v, [g.double() for g in grads], hp,
                                       adapt, decay)
    return params, opt, w, v, trusts


def assert_matches(params, opt, w, v):
    g = opt.groups[0]
    for p, off, wr, vr in zip(params, g.offsets, w, v):
        assert torch.allclose(p.detach().double(), wr, rtol=1e-5, atol=1e-6)
        got_v = g.V[off:off + p.numel()].view(p.shape).double()
        assert torch.allclose(got_v, vr, rtol=1e-5, atol=1e-6)


def test_fallback_matches_fp64_definition():
    params, opt, w, v, trusts = run_both(HP)
    assert_matches(params, opt, w, v)
    # the default rule left both kinds of segment
    assert opt.seg_flags == [0, 0, 0, 3, 3, 0, 3]
    assert all(t == 1.0 for t, s in zip(trusts, SHAPES) if len(s) == 1)
    assert all(t != 1.0 for t, s in zip(trusts, SHAPES) if len(s) > 1)


def test_padding_stays_zero():
    params, opt, _, _, _ = run_both(HP, steps=2)
    g = opt.groups[0]
    own = torch.zeros(g.numel, dtype=torch.bool)
    for p, off in zip(g.params, g.offsets):
        own[off:off + p.numel()] = True
    assert not own.all()
    for buf in (g.P, g.V):
        assert (buf[~own] == 0).all()


def test_zero_gradient_segment_has_trust_one():
    # segment 4 (2-D, adapted): gn == 0 -> trust 1, the update is pure decay
    params, opt, w, v, trusts = run_both(HP, zero_g=(4,))
    assert trusts[4] == 1.0 and trusts[3] != 1.0
    assert_matches(params, opt, w, v)


def test_zero_weight_segment_has_trust_one():
    # wn == 0 on the first step only; compare that step
    params, opt, w, v, trusts = run_both(HP, steps=1, zero_w=(3,))
    assert trusts[3] == 1.0 and trusts[4] != 1.0
    assert_matches(params, opt, w, v)
    assert params[3].detach().abs().sum() > 0


@pytest.mark.parametrize("factor", [0.25, 4.0])
def test_clipping_below_and_above_the_norm(factor):
    gnorm0 = math.sqrt(sum(float(g.double().square().sum())
                           for g in make_grads(0)))
    hp = dict(HP, max_grad_norm=factor * gnorm0)
    params, opt, w, v, _ = run_both(hp, steps=1)
    assert_matches(params, opt, w, v)
    assert float(opt.last_grad_norm()) == pytest.approx(gnorm0, rel=1e-6)
    # clipping changed the result exactly when the bound was below the norm
    params1, _, _, _, _ = run_both(HP, steps=1)
    same = all(torch.equal(a, b) for a, b in zip(params, params1))
    assert same == (factor > 1)


def test_exclude_override():
    # adapt and decay everything but the 4-D weight
    exclude = lambda p: p.ndim == 4  # noqa: E731
    flags = [len(s) != 4 for s in SHAPES]
    params, opt, w, v, trusts = run_both(HP, exclude=exclude,
                                         flags=(flags, flags))
    assert opt.seg_flags == [3, 3, 3, 0, 3, 3, 3]
    assert trusts[3] == 1.0 and trusts[0] != 1.0
    assert_matches(params, opt, w, v)


@pytest.mark.parametrize("dtype", [F32, BF])
def test_inf_gradient_skips_the_step(dtype):
    params = make_params(dtype=dtype)
    opt = FusedLARS(params, **HP)
    set_grads(params, make_grads(0))
    opt.step()
    g = opt.groups[0]
    bufs = [g.P, g.V] + ([g.master] if g.master is not None else [])
    before = [b.clone() for b in bufs]
    grads = make_grads(1)
    grads[4].view(-1)[100] = float("inf")
    set_grads(params, grads)
    opt.step()
    assert opt.skipped_steps() == 1
    assert not math.isfinite(float(opt.last_grad_norm()))
    for b, b0 in zip(bufs, before):
        assert torch.equal(b.view(I32 if b.dtype == F32 else torch.int16),
                           b0.view(I32 if b0.dtype == F32 else torch.int16))
    # the next finite step proceeds
    set_grads(params, make_grads(2))
    opt.step()
    assert opt.skipped_steps() == 1
    assert not torch.equal(g.P, before[0])
    assert math.isfinite(float(opt.last_grad_norm()))


def test_bf16_params_follow_their_master():
    params = make_params(dtype=BF)
    opt = FusedLARS(params, **HP)
    for k in range(2):
        set_grads(params, make_grads(k))
        opt.step()
    g = opt.groups[0]
    assert g.master is not None
    assert torch.equal(g.P, g.master.to(BF))


def test_step_follows_param_group_lr_and_set_lr():
    a, b = make_params(), make_params()
    oa, ob = FusedLARS(a, **HP), FusedLARS(b, **dict(HP, lr=0.125))
    oa.param_groups[0]["lr"] = 0.125      # what _set_lr of a schedule does
    for ps, o in ((a, oa), (b, ob)):
        set_grads(ps, make_grads(0))
        o.step()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    oa.set_lr(0.25)
    assert oa.param_groups[0]["lr"] == 0.25 and float(oa._lr_t) == 0.25


def test_flat_grad_norm_reads_only():
    torch.manual_seed(0)
    m = nn.Sequential(nn.Linear(8, 16), nn.ReLU(), nn.Linear(16, 4))
    opt = FusedSGDMomentum(m.parameters(), lr=0.1, momentum=0.9)
    m(torch.randn(5, 8)).pow(2).sum().backward()
    g = opt.groups[0]
    before = [g.P.clone(), g.G.clone(), g.V.clone()]
    total, per = flat_grad_norm(opt)
    cat = torch.cat([p.grad.reshape(-1) for p in m.parameters()])
    assert total.dim() == 0 and per.shape == (4,)
    assert torch.allclose(total, torch.linalg.vector_norm(cat), rtol=1e-6)
    for n, p in zip(per, m.parameters()):
        assert torch.allclose(n, torch.linalg.vector_norm(p.grad), rtol=1e-6)
    for x, x0 in zip((g.P, g.G, g.V), before):
        assert torch.equal(x, x0)


def test_checkpoint_roundtrip_resumes_bit_identically(tmp_path):
    class Net(nn.Module):
        def __init__(self, seed):
            super().__init__()
            self.ps = nn.ParameterList(make_params(seed))

    def steps(net, opt, ks):
        for k in ks:
            grads = make_grads(k)
            if k == 1:
                grads[0][3] = float("nan")      # one skipped step on the way
            set_grads(list(net.ps), grads)
            opt.step()

    n1 = Net(0)
    o1 = FusedLARS(n1.parameters(), **HP)
    steps(n1, o1, [0, 1, 2])
    path = save_checkpoint(str(tmp_path / "lars.pt"), n1, o1, step=3)

    n2 = Net(5)
    o2 = FusedLARS(n2.parameters(), **dict(HP, lr=0.03))
    load_checkpoint(path, n2, o2)
    assert o2.skipped_steps() == o1.skipped_steps() == 1
    assert o2.param_groups[0]["lr"] == HP["lr"]
    steps(n1, o1, [3, 4])
    steps(n2, o2, [3, 4])
    for a, b in zip(n1.ps, n2.ps):
        assert torch.equal(a, b)
    assert torch.equal(o1.groups[0].V, o2.groups[0].V)


def test_warmup_poly():
    params = make_params()
    opt = FusedLARS(params, **HP)
    sched = warmup_poly(opt, base_lr=0.8, warmup_cycles=5, total_cycles=25,
                        power=2.0, min_lr=0.01)
    lrs = [sched(c) for c in range(26)]
    assert lrs[0] == 0.0
    assert lrs[5] == 0.8
    assert lrs[25] == pytest.approx(0.01)
    assert all(a < b for a, b in zip(lrs[:5], lrs[1:6]))
    assert all(a > b for a, b in zip(lrs[5:25], lrs[6:26]))
    # past the end it stays at min_lr, and the optimizer follows
    assert sched(40) == pytest.approx(0.01)
    assert opt.param_groups[0]["lr"] == pytest.approx(0.01)
    assert float(opt._lr_t) == pytest.approx(0.01)
    # an optimizer without set_lr only gets its param_groups written
    sgd = FusedSGDMomentum(make_params(), lr=0.1)
    warmup_poly(sgd, 0.8, 5, 25)(5)
    assert sgd.param_groups[0]["lr"] == 0.8


# ---- the native host plan and the bindings' refusals -----------------------

C = load_native()
needs_native = pytest.mark.skipif(C is None, reason="native extension not built")


def _layout(numels):
    offs, total = [], 0
    for n in numels:
        offs.append(total)
        total += (n + 63) // 64 * 64
    return offs, total


@needs_native
def test_lars_plan_tiles_every_segment():
    CH = C.LARS_CHUNK
    numels = [10, 64, 77, CH, CH + 1, 3 * CH + 520, 1728, 64]
    offs, n = _layout(numels)
    t = C.lars_plan(offs, numels, n, 7)
    assert t.dtype == I32 and t.device.type == "cpu" and t.shape[1] == 3
    assert t.is_contiguous()
    rows = t.tolist()
    # segments appear in order, ids start at seg_base
    assert [r[0] for r in rows] == sorted(r[0] for r in rows)
    for i, (off, numel) in enumerate(zip(offs, numels)):
        mine = [r for r in rows if r[0] == 7 + i]
        assert len(mine) == -(-numel // CH)
        at = off
        for _, start, count in mine:       # exact tiling, in order
            assert start == at and 1 <= count <= CH
            assert (start - off) % 64 == 0 and start % 64 == 0
            at += count
        assert at == off + numel
        assert sum(r[2] for r in mine) == numel


@needs_native
def test_lars_plan_refusals():
    ok_offs, ok_n = _layout([100, 64])
    C.lars_plan(ok_offs, [100, 64], ok_n, 0)
    cases = {
        "unsorted": (([128, 0], [64, 100], 192, 0), "unsorted or overlaps"),
        "overlapping": (([0, 64], [100, 64], 192, 0), "unsorted or overlaps"),
        "misaligned": (([0, 100], [100, 64], 192, 0), "multiple of 64"),
        "past_the_end": (([0, 128], [100, 65], 192, 0), "reaches past"),
        "n_2_31": (([0], [64], 2 ** 31, 0), "fewer than 2\\^31"),
        "lengths": (([0, 128], [100], 192, 0), "differ in length"),
    }
    for name, (args, msg) in cases.items():
        with pytest.raises(RuntimeError, match=msg):
            C.lars_plan(*args)


on_cpu_only = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="CPU-only: a refusal test must never reach a launch")


def _operands(dtype=F32, n=128, S=2, chunks=2):
    P = torch.zeros(n, dtype=dtype)
    M = torch.zeros(n) if dtype == BF else P
    return dict(
        P=P, G=torch.zeros(n, dtype=dtype), M=M, V=torch.zeros(n),
        table=torch.tensor([[0, 0, 64], [1, 64, 64]], dtype=I32),
        partials=torch.zeros(2 * chunks, dtype=F64),
        seg_meta=torch.tensor([[0, 1, 3], [1, 2, 0]], dtype=I32),
        coef=torch.zeros(S), stats=torch.zeros(2 + 2 * S),
        lr=torch.zeros(1), skipped=torch.zeros(1, dtype=I32))


def _norms(o, chunk_base=0, total=2, S=2):
    C.lars_norms(o["P"], o["G"], o["M"], o["table"], o["partials"],
                 chunk_base, total, S)


def _fold(o):
    C.lars_fold(o["partials"], o["seg_meta"], o["lr"], o["coef"], o["stats"],
                o["skipped"], 1e-3, 5e-5, 1e-9, 0.0)


def _step(o):
    C.lars_step(o["P"], o["G"], o["M"], o["V"], o["table"], o["seg_meta"],
                o["coef"], o["stats"], 0.9, 5e-5)


@needs_native
@on_cpu_only
@pytest.mark.parametrize("call", [_norms, _fold, _step])
@pytest.mark.parametrize("dtype", [F32, BF])
def test_host_tensors_refused_by_the_device_check_alone(call, dtype):
    with pytest.raises(RuntimeError, match="device tensors required"):
        call(_operands(dtype))


def _with(**kw):
    o = _operands()
    o.update(kw)
    return o


REFUSALS = {
    "norms_G_dtype": (lambda: _norms(_with(G=torch.zeros(128, dtype=BF))),
                      "G must be contiguous"),
    "norms_short_G": (lambda: _norms(_with(G=torch.zeros(64))),
                      "G must be contiguous"),
    "norms_bf16_without_master": (
        lambda: _norms(_with(P=torch.zeros(128, dtype=BF),
                             G=torch.zeros(128, dtype=BF),
                             M=torch.zeros(128, dtype=BF))),
        "M must be contiguous"),
    "norms_unpadded": (lambda: _norms(_with(P=torch.zeros(72),
                                            G=torch.zeros(72),
                                            M=torch.zeros(72))),
                       "padded to 64"),
    "norms_table_dtype": (
        lambda: _norms(_with(table=torch.zeros(2, 3, dtype=torch.int64))),
        "table must be contiguous int32"),
    "norms_table_shape": (
        lambda: _norms(_with(table=torch.zeros(2, 4, dtype=I32))),
        "table must be contiguous int32"),
    "norms_table_strided": (
        lambda: _norms(_with(table=torch.zeros(2, 6, dtype=I32)[:, ::2])),
        "table must be contiguous int32"),
    "norms_partials_dtype": (
        lambda: _norms(_with(partials=torch.zeros(4))),
        "partials must be contiguous"),
    "norms_partials_short": (
        lambda: _norms(_with(partials=torch.zeros(2, dtype=F64))),
        "partials must be contiguous"),
    "norms_chunks_past_partials": (lambda: _norms(_operands(), chunk_base=1),
                                   "leave the 2 rows of partials"),
    "fold_partials_dtype": (lambda: _fold(_with(partials=torch.zeros(4))),
                            "partials must be contiguous double"),
    "fold_partials_odd": (
        lambda: _fold(_with(partials=torch.zeros(3, dtype=F64))),
        "partials must be contiguous double"),
    "fold_seg_meta_dtype": (
        lambda: _fold(_with(seg_meta=torch.zeros(2, 3))),
        "seg_meta must be contiguous int32"),
    "fold_coef_length": (lambda: _fold(_with(coef=torch.zeros(3))),
                         "coef must be contiguous"),
    "fold_stats_length": (lambda: _fold(_with(stats=torch.zeros(4))),
                          "stats must be contiguous"),
    "fold_lr_dtype": (lambda: _fold(_with(lr=torch.zeros(1, dtype=F64))),
                      "lr must be contiguous"),
    "fold_lr_length": (lambda: _fold(_with(lr=torch.zeros(2))),
                       "lr must be contiguous"),
    "fold_counter_dtype": (lambda: _fold(_with(skipped=torch.zeros(1))),
                           "skipped must be contiguous"),
    "fold_counter_length": (
        lambda: _fold(_with(skipped=torch.zeros(2, dtype=I32))),
        "skipped must be contiguous"),
    "step_V_dtype": (lambda: _step(_with(V=torch.zeros(128, dtype=BF))),
                     "state must be contiguous"),
    "step_short_V": (lambda: _step(_with(V=torch.zeros(64))),
                     "state must be contiguous"),
    "step_table_dtype": (
        lambda: _step(_with(table=torch.zeros(2, 3))),
        "table must be contiguous int32"),
    "step_coef_dtype": (lambda: _step(_with(coef=torch.zeros(2, dtype=F64))),
                        "coef must be contiguous"),
    "step_stats_short": (lambda: _step(_with(stats=torch.zeros(5))),
                         "stats must be contiguous"),
}


@needs_native
@on_cpu_only
@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refused_before_the_device_check(case):
    call, message = REFUSALS[case]
    with pytest.raises(RuntimeError, match=message) as info:
        call()
    assert "device tensors required" not in str(info.value)
