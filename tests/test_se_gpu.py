"""Squeeze-and-excitation kernels (se.hip) against the formula in float64 on
the CPU, autograd for the backward, from the bf16-rounded operands.

Bounds, with U = 2^-24, B = 2^-8 (one bf16 round), HW pixels, and S the same
linear computation on |operands| (a value rounded once to bf16 from an fp32
value of error E may differ by E + B*(|ref| + E)):
  z    |err| <= 2*HW*U*Sz,  Sz = mean|u|: HW-1 adds, the 1/HW round, one mul.
  a1   |err| <= 2*(HW+C+8)*U*S1,  S1 = |W1| Sz + |b1|: z's error through
       |W1|, a C-long fp32 dot, the bias add. Every reference |a1| exceeds
       100x this (asserted), so the hidden ReLU's mask is not in question;
       h inherits the bound (ReLU is 1-Lipschitz).
  s    |err| <= 2*(HW+C+Cr+8)*U*S2/4 + 8U,  S2 = |W2| S1 + |b2|: sigmoid is
       1/4-Lipschitz; 8U for exp, the add and the division.
  out  against relu(u*s + identity) in float64 with the KERNEL's s: one fp32
       round (the fma) and one bf16 round of that value, E = U*|v|.
se_bwd fed the reference's out (bf16) and s, h, z (rounded to fp32), with
Sds = sum_hw |mg*u|, Sdh = |W2|^T Sds, Sdz = |W1|^T Sdh / HW, which drop the
factor s(1-s) <= 1/4 (|d s(1-s)| <= |ds| absorbs the fp32 round of s):
  du   E = 2*(HW+C+Cr+264)*U*(Sdz + |mg|*s), then one bf16 round: the ds sum,
       the C-long dot in C/rg + rg <= C + 256 adds, the Cr-long dot, the fma.
  gidentity  bit for bit out > 0 ? g : +0.
  dW2, db2   E = 2*(N+HW+4)*U*S, S = sum_n Sds*|h| (db2: sum_n Sds)
  dW1, db1   E = 2*(N+HW+C+264)*U*S, S = sum_n Sdh*|z| (db1: sum_n Sdh)
       then one bf16 round; two calls give equal bits.
Whole op (kernel's own gate in the backward): the gate's errors bs, ba1, bz
enter linearly, du: + bs*(|mg| + Sdz); dW2: + bs*S + ba1*sum_n Sds; dW1:
+ bs*S + bz*sum_n Sdh; db*: + bs*S. Elements whose reference pre-ReLU value
lies within 2^-7*(|u*s| + |identity|) of zero are left out of du/gidentity
(at most 2 %, asserted from the reference alone).
Worst measured |err|/bound on the MI355X over the table and all tests: z 0.06,
h 0.01, s 0.01, out 1.00, du 0.98, dW1 0.45, db1 0.20, dW2 0.99, db2 0.97 (the
values near 1 are the bf16 round itself).
"""

import functools
import types

import pytest
import torch

from fluxdistributed_amd.models import build_model
from fluxdistributed_amd.ops import logit_cross_entropy, se as se_mod
from fluxdistributed_amd.ops.native import load_native
from fluxdistributed_amd.utils.precision import to_mixed_bf16

pytestmark = pytest.mark.gpu

# (N, C, H, W, Cr)
SHAPES = [
    (2, 64, 7, 7, 4),        # smallest C and Cr, odd HW
    (3, 128, 5, 3, 8),       # HW < one block pass, odd N: short last ipb group
    (2, 2048, 2, 2, 128),    # largest C and Cr
    (5, 512, 9, 9, 32),      # parameter-grad sum over 5 images
    (2, 64, 10, 20, 4),      # nsplit 3, chunks of 67 rows, the last of 66
    (33, 64, 2, 2, 4),       # a long image loop
    (2, 192, 3, 3, 12),      # 256 % (C/8) != 0: idle lanes; Cr % 8 != 0
    (513, 64, 1, 1, 4),      # ipb 4, last group of one image
]
U, B = 2.0 ** -24, 2.0 ** -8


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last).cuda()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded bf16 operands (CPU), the float64 reference and its bounds."""
    N, C, H, W, Cr = shape
    HW = H * W
    gen = torch.Generator().manual_seed(sum(shape))
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    # a per-channel offset keeps z, and so a1, O(1); |b1| ~ 6 gives a1 its
    # margin and a mask with both signs
    ops = [r(N, C, H, W) + r(1, C, 1, 1), r(N, C, H, W), r(Cr, C) / C ** 0.5,
           (6 + torch.rand(Cr, generator=gen)) * torch.sign(r(Cr)),
           0.25 * r(C, Cr) / Cr ** 0.5, r(C)]
    ops = [t.bfloat16() for t in ops]
    g = r(N, C, H, W).bfloat16()
    u, idn, w1, b1, w2, b2 = leaves = [t.double().requires_grad_(True)
                                       for t in ops]
    z = u.mean((2, 3))
    a1 = z @ w1.T + b1
    h = a1.relu()
    s = (h @ w2.T + b2).sigmoid()
    pre = u * s[:, :, None, None] + idn
    out = pre.relu()
    grads = torch.autograd.grad(out, leaves, g.double())
    with torch.no_grad():
        Sz = u.abs().mean((2, 3))
        S1 = Sz @ w1.abs().T + b1.abs()
        S2 = S1 @ w2.abs().T + b2.abs()
        bz, ba1 = 2 * HW * U * Sz, 2 * (HW + C + 8) * U * S1
        bs = 2 * (HW + C + Cr + 8) * U * S2 / 4 + 8 * U
        assert bool((a1.abs() > 100 * ba1).all())
        mg = torch.where(out > 0, g.double(), 0.0)
        Sds = (mg * u).abs().sum((2, 3))
        Sdh = Sds @ w2.abs()
        Sdz = (Sdh @ w1.abs()) / HW
        near = pre.abs() < 2.0 ** -7 * ((u * s[:, :, None, None]).abs()
                                        + idn.abs())
        assert near.double().mean().item() <= 0.02
        k1, k2 = 2 * (N + HW + C + 264) * U, 2 * (N + HW + 4) * U
        # (E, extra of the whole-op test) for du, dw1, db1, dw2, db2
        Eg = {
            "du": (2 * (HW + C + Cr + 264) * U
                   * (Sdz[:, :, None, None] + mg.abs() * s[:, :, None, None]),
                   bs.max() * (mg.abs() + Sdz[:, :, None, None])),
            "dw1": (k1 * (Sdh.T @ z.abs()),
                    bs.max() * (Sdh.T @ z.abs()) + bz.max() * Sdh.sum(0)[:, None]),
            "db1": (k1 * Sdh.sum(0), bs.max() * Sdh.sum(0)),
            "dw2": (k2 * (Sds.T @ h.abs()),
                    bs.max() * (Sds.T @ h.abs()) + ba1.max() * Sds.sum(0)[:, None]),
            "db2": (k2 * Sds.sum(0), bs.max() * Sds.sum(0)),
        }
    det = lambda t: t.detach()  # noqa: E731
    return types.SimpleNamespace(
        ops=ops, g=g, z=det(z), h=det(h), s=det(s), out=det(out), near=near,
        grads=dict(zip(("du", "gid", "dw1", "db1", "dw2", "db2"), grads)),
        bz=bz, ba1=ba1, bs=bs, Eg=Eg)


def _check(what, got, ref, E, rounded):
    err = (got.double().cpu() - ref).abs()
    bound = E + B * (ref.abs() + E) if rounded else E + 0 * ref
    print(f"{what}: worst |err|/bound = "
          f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert got.shape == ref.shape
    assert bool((err <= bound).all())


def _gid_ref(out, g):
    return torch.where(out > 0, g, torch.zeros_like(g))


@pytest.mark.parametrize("shape", SHAPES)
def test_fwd(shape):
    c = _case(shape)
    u, idn = c.ops[0], c.ops[1]
    out, s, h, z = load_native().se_fwd(_cl(u), _cl(idn),
                                        *(t.cuda() for t in c.ops[2:]))
    assert out.dtype == torch.bfloat16 and s.dtype == torch.float32
    _check("z", z, c.z, c.bz, False)
    _check("h", h, c.h, c.ba1, False)
    _check("s", s, c.s, c.bs, False)
    v = (u.double() * s.double().cpu()[:, :, None, None] + idn.double()).relu()
    _check("out", out, v, U * v, True)


@pytest.mark.parametrize("shape", SHAPES)
def test_bwd(shape):
    c = _case(shape)
    out = c.out.bfloat16()
    run = lambda: load_native().se_bwd(  # noqa: E731
        _cl(c.g), _cl(out), _cl(c.ops[0]), c.s.float().cuda(),
        c.h.float().cuda(), c.z.float().cuda(), c.ops[2].cuda(),
        c.ops[4].cuda())
    got = dict(zip(("du", "gid", "dw1", "db1", "dw2", "db2"), run()))
    again = run()
    assert torch.equal(got["gid"].cpu().view(torch.int16),
                       _gid_ref(out, c.g).view(torch.int16))
    for i, k in enumerate(("du", "dw1", "db1", "dw2", "db2")):
        _check(k, got[k], c.grads[k], c.Eg[k][0], True)
        assert torch.equal(got[k], again[i + (i > 0)])  # same bits every run


def test_plan_splits_rows_and_groups_images():
    cfg = load_native().se_config
    nsplit, rpc, _ = cfg(2, 200, 64, 4)
    assert (nsplit, rpc) == (3, 67) and 200 % rpc != 0
    assert cfg(3, 15, 128, 8)[2] == 2 and cfg(513, 1, 64, 4)[2] == 4


@pytest.mark.parametrize("shape", SHAPES[:5])
def test_whole_op_autograd(shape, monkeypatch):
    monkeypatch.setenv("FLUXDIST_SE", "1")
    c = _case(shape)
    leaves = [_cl(t).requires_grad_(True) for t in c.ops[:2]]
    leaves += [t.cuda().requires_grad_(True) for t in c.ops[2:]]
    out = se_mod.se_scale_add_relu(*leaves)
    out.backward(_cl(c.g))
    au = c.ops[0].double().abs()
    E = c.bs[:, :, None, None] * au
    _check("out", out.detach(), c.out, E + U * c.out, True)
    keep = ~c.near
    gid = leaves[1].grad.cpu()
    assert torch.equal(gid[keep].view(torch.int16),
                       _gid_ref(c.out, c.g)[keep].view(torch.int16))
    E, extra = c.Eg["du"]
    z0 = torch.zeros(())
    _check("du", torch.where(keep, leaves[0].grad.cpu().double(), z0),
           torch.where(keep, c.grads["du"], z0.double()), E + extra, True)
    for k, t in zip(("dw1", "db1", "dw2", "db2"), leaves[2:]):
        _check(k, t.grad, c.grads[k], sum(c.Eg[k]), True)


@pytest.mark.parametrize("knob", ["1", "0"])
def test_dispatch(knob, monkeypatch):
    c = _case(SHAPES[0])
    native, calls = load_native(), []

    def se_fwd(*a):
        calls.append("se_fwd")
        return native.se_fwd(*a)

    monkeypatch.setenv("FLUXDIST_SE", knob)
    monkeypatch.setattr(se_mod, "require_native", lambda op: (
        types.SimpleNamespace(se_fwd=se_fwd, se_bwd=native.se_bwd)))
    out = se_mod.se_scale_add_relu(_cl(c.ops[0]), _cl(c.ops[1]),
                                   *(t.cuda() for t in c.ops[2:]))
    assert calls == (["se_fwd"] if knob == "1" else [])
    # either path is the op: the composition rounds u*s, s and the sum to
    # bf16, 3 * 2^-8 relative to |u*s| + |identity| at the most
    assert torch.allclose(out.double().cpu(), c.out, rtol=2 ** -6, atol=2 ** -6)


def test_se_resnet18_step(monkeypatch):
    torch.manual_seed(0)
    model = build_model("se_resnet18", num_classes=16, small_input=True).cuda()
    model = to_mixed_bf16(model.to(memory_format=torch.channels_last)).train()
    x = _cl(torch.randn(2, 3, 32, 32)).bfloat16()
    y = torch.tensor([3, 11]).cuda()
    losses = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("FLUXDIST_SE", knob)
        model.zero_grad()
        loss = logit_cross_entropy(model(x), y)
        loss.backward()
        losses[knob] = float(loss.detach())
        assert bool(torch.isfinite(loss))
        se = [(n, p) for n, p in model.named_parameters() if ".se." in n]
        assert len(se) == 8 * 4
        for n, p in se:
            assert p.dtype == torch.bfloat16
            assert bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), n
    assert abs(losses["1"] - losses["0"]) < 1e-2
