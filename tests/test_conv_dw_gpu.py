"""Depthwise 3x3 conv kernels (conv_dw.hip) against float64 F.conv2d with
groups == C and its autograd on the CPU, from the bf16-rounded operands.

Products of bf16 values are exact in fp32, so the bounds are derived. With S
the same computation on |operands| and U = 2^-24:
  wgrad (fp32 out):         |err| <= 2*(M + nch)*U*S, M pixels, nch slabs;
  fwd, dgrad (one bf16 round), E = 2*9*U*S:
                            |err| <= E + 2^-8*(|ref| + E)
on every element. Worst measured |err|/bound on the MI355X over the table:
fwd 0.99, dgrad 0.99 (the bf16 round itself), wgrad 0.08; through fda_conv2d
(dw rounded to bf16) 0.91.
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

# (N, C, H, W, stride)
SHAPES = [
    (2, 8, 5, 7, 1),       # one lane per pixel, odd extents, short rows
    (1, 24, 9, 11, 2),     # 3 lanes per pixel: idle lanes; unequal classes
    (2, 32, 12, 10, 2),    # even extents at stride 2
    (2, 16, 1, 1, 2),      # a single pixel: only the centre tap is inside
    (1, 512, 3, 3, 1),     # many channels, image smaller than a strip
    (1, 1032, 4, 5, 1),    # five channel slabs, the last one short
    (3, 64, 20, 23, 1),    # several strips per row and a remainder strip
    (3, 64, 24, 6, 1),     # wgrad: 72 rows in chunks of 32, 32 and 8
]
U = 2.0 ** -24


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded bf16 operands (CPU) and the float64 reference with its S."""
    N, C, H, W, s = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, C, H, W, generator=gen).bfloat16()
    w = torch.randn(C, 1, 3, 3, generator=gen).bfloat16()
    dy = torch.randn(N, C, (H - 1) // s + 1, (W - 1) // s + 1,
                     generator=gen).bfloat16()

    def run(x_, w_, dy_):
        x_ = x_.double().requires_grad_(True)
        w_ = w_.double().requires_grad_(True)
        y = F.conv2d(x_, w_, None, s, 1, 1, C)
        y.backward(dy_.double())
        return y.detach(), x_.grad, w_.grad

    return types.SimpleNamespace(x=x, w=w, dy=dy, ref=run(x, w, dy),
                                 S=run(x.abs(), w.abs(), dy.abs()),
                                 M=dy.numel() // C)


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
    N, C, H, W, s = shape
    return load_native().conv_dw_config(N, H, W, C, s, "wgrad")[2]


@pytest.mark.parametrize("shape", SHAPES)
def test_fwd(shape):
    c = _case(shape)
    y = load_native().conv_dw_fwd(_cl(c.x).cuda(), c.w.cuda(), shape[4],
                                  shape[4])
    assert y.dtype == torch.bfloat16
    _check("fwd", y, c.ref[0], c.S[0], 9, True)


@pytest.mark.parametrize("shape", SHAPES)
def test_dgrad(shape):
    c = _case(shape)
    dx = load_native().conv_dw_dgrad(_cl(c.dy).cuda(), c.w.cuda(), shape[2],
                                     shape[3], shape[4], shape[4])
    _check("dgrad", dx, c.ref[1], c.S[1], 9, True)


@pytest.mark.parametrize("shape", SHAPES)
def test_wgrad(shape):
    c = _case(shape)
    run = lambda: load_native().conv_dw_wgrad(  # noqa: E731
        _cl(c.dy).cuda(), _cl(c.x).cuda(), shape[4], shape[4])
    ws = run()
    assert ws.dtype == torch.float32 and ws.shape == (shape[1], 9)
    _check("wgrad", ws.view(shape[1], 1, 3, 3), c.ref[2], c.S[2],
           c.M + _nch(shape), False)
    assert torch.equal(ws, run())   # same bits on every run


def test_wgrad_chunks_with_short_last():
    # 3 images x 24 rows = 72 units, 32 per chunk (one per pixel group of
    # the 8-lane slab): 32 + 32 + 8
    cfg = load_native().conv_dw_config
    assert cfg(3, 24, 6, 64, 1, "wgrad") == (1, 6, 3, 32)
    assert cfg(2, 5, 7, 8, 1, "wgrad")[2] == 1   # written directly


@pytest.mark.parametrize("knob", ["1", "0"])
def test_fda_conv2d_dispatches_depthwise(knob, monkeypatch):
    shape = SHAPES[1]
    N, C, H, W, s = shape
    c = _case(shape)

    def library(*a, **k):
        raise AssertionError("library conv reached")

    monkeypatch.setenv("FLUXDIST_CONV_DW", knob)
    monkeypatch.delenv("FLUXDIST_CONV", raising=False)
    monkeypatch.setattr(conv_mod, "F", types.SimpleNamespace(conv2d=library))
    x = _cl(c.x).cuda().requires_grad_(True)
    w = c.w.cuda().requires_grad_(True)
    if knob == "0":
        with pytest.raises(AssertionError, match="library conv reached"):
            conv_mod.fda_conv2d(x, w, s, 1, 1, C)
        return
    y = conv_mod.fda_conv2d(x, w, s, 1, 1, C)
    y.backward(_cl(c.dy).cuda())
    _check("fwd", y.detach(), c.ref[0], c.S[0], 9, True)
    _check("dgrad", x.grad, c.ref[1], c.S[1], 9, True)
    # dw is the bf16 cast of the fp32 result: one more round
    _check("wgrad", w.grad, c.ref[2], c.S[2], c.M + _nch(shape), True)


def test_mobilenet_step_without_library_depthwise(monkeypatch):
    real = F.conv2d

    def library(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        if groups != 1:
            raise AssertionError("library depthwise conv reached")
        return real(x, w, b, stride, padding, dilation, groups)

    monkeypatch.setenv("FLUXDIST_CONV_DW", "1")
    monkeypatch.delenv("FLUXDIST_CONV", raising=False)
    monkeypatch.setattr(conv_mod, "F", types.SimpleNamespace(conv2d=library))
    torch.manual_seed(0)
    model = build_model("mobilenet_v1", small_input=True).cuda()
    model = to_mixed_bf16(model.to(memory_format=torch.channels_last)).train()
    x = _cl(torch.randn(2, 3, 64, 64)).cuda().bfloat16()
    out = model(x)
    out.float().square().mean().backward()
    assert bool(torch.isfinite(out).all())
    convs = [m for m in model.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 27
    assert all(m.weight.grad is not None for m in convs)
