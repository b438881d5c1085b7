"""Grouped 3x3 conv kernels (conv_grouped.hip) against float64 F.conv2d and
its autograd on the CPU, from the bf16-rounded operands.

Products of bf16 values are exact in fp32, so the bounds are derived. With S
the same computation on |operands| and U = 2^-24:
  wgrad (fp32 out):         |err| <= 2*(M + nch)*U*S, M pixels, nch slabs;
  fwd, dgrad (one bf16 round), n = 9*cpg, E = 2*n*U*S:
                            |err| <= E + 2^-8*(|ref| + E)
on every element. Worst measured |err|/bound on the MI355X over the table:
fwd 0.99, dgrad 0.99 (the bf16 round itself), wgrad 0.03.
"""

import functools
import types

import pytest
import torch
import torch.nn.functional as F

from fluxdistributed_amd.models import build_model
from fluxdistributed_amd.ops import conv as conv_mod
from fluxdistributed_amd.ops.native import load_native
from fluxdistributed_amd.utils.precision import to_mixed_bf16

pytestmark = pytest.mark.gpu

# (N, C, H, W, groups, stride)
SHAPES = [
    (2, 64, 9, 11, 16, 1),     # cpg 4, odd extents, borders, partial tile
    (1, 64, 13, 13, 8, 2),     # cpg 8, stride 2, unequal parity classes
    (2, 128, 7, 7, 8, 1),      # cpg 16, two 64-channel slabs
    (1, 128, 10, 9, 4, 2),     # cpg 32, stride 2, even x odd extent
    (1, 256, 6, 6, 64, 1),     # cpg 4, group index beyond one slab
    (3, 64, 20, 23, 2, 1),     # cpg 32, several spatial tiles
    (7, 64, 20, 23, 2, 1),     # wgrad: 11 chunks of 4 units, the last of 2
]
U = 2.0 ** -24


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded bf16 operands (CPU) and the float64 reference with its S."""
    N, C, H, W, g, s = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, C, H, W, generator=gen).bfloat16()
    w = torch.randn(C, C // g, 3, 3, generator=gen).bfloat16()
    dy = torch.randn(N, C, (H - 1) // s + 1, (W - 1) // s + 1,
                     generator=gen).bfloat16()

    def run(x_, w_, dy_):
        x_ = x_.double().requires_grad_(True)
        w_ = w_.double().requires_grad_(True)
        y = F.conv2d(x_, w_, None, s, 1, 1, g)
        y.backward(dy_.double())
        return y.detach(), x_.grad, w_.grad

    return types.SimpleNamespace(x=x, w=w, dy=dy, ref=run(x, w, dy),
                                 S=run(x.abs(), w.abs(), dy.abs()),
                                 M=dy.numel() // C, cpg=C // g,
                                 args=(s, s, 1, 1, g))


def _check(what, got, ref, S, n, rounded):
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 * n * U * S
    if rounded:
        bound = bound + 2.0 ** -8 * (ref.abs() + bound)
    print(f"{what}: worst |err|/bound = "
          f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert got.shape == ref.shape
    assert bool((err <= bound).all())


def _nch(shape):
    N, C, H, W, g, s = shape
    return load_native().conv_grouped_config(N, H, W, C, g, s, "wgrad")[2]


@pytest.mark.parametrize("shape", SHAPES)
def test_fwd(shape):
    c = _case(shape)
    y = load_native().conv_grouped_fwd(_cl(c.x).cuda(), _cl(c.w).cuda(),
                                       *c.args)
    assert y.dtype == torch.bfloat16
    _check("fwd", y, c.ref[0], c.S[0], 9 * c.cpg, True)


@pytest.mark.parametrize("shape", SHAPES)
def test_dgrad(shape):
    c = _case(shape)
    dx = load_native().conv_grouped_dgrad(_cl(c.dy).cuda(), _cl(c.w).cuda(),
                                          shape[2], shape[3], *c.args)
    _check("dgrad", dx, c.ref[1], c.S[1], 9 * c.cpg, True)


@pytest.mark.parametrize("shape", SHAPES)
def test_wgrad(shape):
    c = _case(shape)
    run = lambda: load_native().conv_grouped_wgrad(  # noqa: E731
        _cl(c.dy).cuda(), _cl(c.x).cuda(), *c.args)
    ws = run()
    assert ws.dtype == torch.float32 and ws.shape == (shape[1], 9 * c.cpg)
    dw = ws.view(shape[1], 3, 3, c.cpg).permute(0, 3, 1, 2)
    _check("wgrad", dw, c.ref[2], c.S[2], c.M + _nch(shape), False)
    assert torch.equal(ws, run())   # same bits on every run


def test_wgrad_chunks_with_short_last():
    # 7 images x 6 tiles of 7x12 = 42 units, 4 per chunk: 10 x 4 + 2
    cfg = load_native().conv_grouped_config
    assert cfg(7, 20, 23, 64, 2, 1, "wgrad") == (7, 12, 11, 4 * 84)
    assert cfg(1, 10, 9, 128, 4, 2, "wgrad")[2] == 1   # written directly


@pytest.mark.parametrize("knob", ["1", "0"])
def test_fda_conv2d_dispatches_grouped(knob, monkeypatch):
    shape = SHAPES[1]
    N, C, H, W, g, s = shape
    c = _case(shape)

    def library(*a, **k):
        raise AssertionError("library conv reached")

    monkeypatch.setenv("FLUXDIST_CONV_GROUPED", knob)
    monkeypatch.delenv("FLUXDIST_CONV", raising=False)
    monkeypatch.setattr(conv_mod, "F", types.SimpleNamespace(conv2d=library))
    x = _cl(c.x).cuda().requires_grad_(True)
    w = _cl(c.w).cuda().requires_grad_(True)
    if knob == "0":
        with pytest.raises(AssertionError, match="library conv reached"):
            conv_mod.fda_conv2d(x, w, s, 1, 1, g)
        return
    y = conv_mod.fda_conv2d(x, w, s, 1, 1, g)
    y.backward(_cl(c.dy).cuda())
    _check("fwd", y.detach(), c.ref[0], c.S[0], 9 * c.cpg, True)
    _check("dgrad", x.grad, c.ref[1], c.S[1], 9 * c.cpg, True)
    # dw is the bf16 cast of the fp32 result: one more round
    _check("wgrad", w.grad, c.ref[2], c.S[2], c.M + _nch(shape), True)


def test_resnext50_step_without_library_conv(monkeypatch):
    def library(*a, **k):
        raise AssertionError("library conv reached")

    monkeypatch.setenv("FLUXDIST_CONV_GROUPED", "1")
    monkeypatch.delenv("FLUXDIST_CONV", raising=False)
    monkeypatch.setattr(conv_mod, "F", types.SimpleNamespace(conv2d=library))
    torch.manual_seed(0)
    model = build_model("resnext50_32x4d").cuda()
    model = to_mixed_bf16(model.to(memory_format=torch.channels_last)).train()
    x = _cl(torch.randn(2, 3, 64, 64)).cuda().bfloat16()
    out = model(x)
    out.float().square().mean().backward()
    assert bool(torch.isfinite(out).all())
    convs = [m for m in model.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 53
    assert all(m.weight.grad is not None for m in convs)
