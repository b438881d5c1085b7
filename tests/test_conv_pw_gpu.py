"""Narrow pointwise conv kernels (conv_pw.hip) against float64 F.conv2d and
its autograd on the CPU, from the bf16-rounded operands.

Products of bf16 values are exact in fp32, so the bounds are derived. With S
the same computation on |operands| and U = 2^-24:
  wgrad (fp32 out):         |err| <= 2*(M + nch)*U*S, M pixels, nch slabs;
  fwd (n = C), dgrad (n = K), one bf16 round, E = 2*n*U*S:
                            |err| <= E + 2^-8*(|ref| + E)
on every element. Worst measured |err|/bound on the MI355X over the table:
fwd 0.996, dgrad 0.996 (the bf16 round itself), wgrad 0.036; through
fda_conv2d (dw rounded to bf16) 0.961; with an Inf pixel fwd 0.965, dgrad
0.948.
"""

import functools
import types

import pytest
import torch
import torch.nn.functional as F

from fluxdistributed_amd.models import MobileNetV1
from fluxdistributed_amd.ops import conv as conv_mod
from fluxdistributed_amd.ops.native import load_native
from fluxdistributed_amd.utils.precision import to_mixed_bf16

pytestmark = pytest.mark.gpu

# (N, C, K, H, W)
SHAPES = [
    (1, 8, 8, 3, 5),        # one granule, far below an MFMA tile, M = 15 < 16
    (2, 24, 40, 5, 7),      # neither a multiple of 16; 3 of 4 granules; M = 70
    (1, 32, 64, 9, 9),      # the MobileNetV1 shape: exactly one reduction step
    (1, 72, 136, 4, 5),     # tail in the third step; three slabs, last short
    (1, 256, 256, 2, 9),    # the register-budget corner, four slabs each way
    (1, 200, 16, 6, 6),     # wide in, narrow out
    (1, 16, 200, 6, 6),     # and the reverse (the roles swap in dgrad)
    (1, 16, 24, 15, 20),    # wgrad: 300 pixels in chunks of 128, 128 and 44
    (1, 8, 200, 129, 255),  # fwd: two tiles per wave; wgrad: two rounds a chunk
    (1, 200, 8, 129, 255),  # dgrad: two tiles per wave
]
U = 2.0 ** -24
INF_CASE = SHAPES[1]


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded bf16 operands (CPU) and the float64 reference with its S."""
    N, C, K, H, W = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, C, H, W, generator=gen).bfloat16()
    w = torch.randn(K, C, 1, 1, generator=gen).bfloat16()
    dy = torch.randn(N, K, H, W, generator=gen).bfloat16()

    def run(x_, w_, dy_):
        x_ = x_.double().requires_grad_(True)
        w_ = w_.double().requires_grad_(True)
        y = F.conv2d(x_, w_)
        y.backward(dy_.double())
        return y.detach(), x_.grad, w_.grad

    return types.SimpleNamespace(x=x, w=w, dy=dy, ref=run(x, w, dy),
                                 S=run(x.abs(), w.abs(), dy.abs()),
                                 M=N * H * W)


def _check(what, got, ref, S, n, rounded, keep=None):
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 * n * U * S
    if rounded:
        bound = bound + 2.0 ** -8 * (ref.abs() + bound)
    if keep is not None:   # [N,1,H,W] mask of the pixels that are compared
        assert bool(torch.isfinite(got.cpu()[keep.expand_as(got)]).all())
        err = torch.where(keep, err, torch.zeros_like(err))
    print(f"{what}: worst |err|/bound = "
          f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert got.shape == ref.shape
    assert bool((err <= bound).all())


def _cfg(shape, mode):
    N, C, K, H, W = shape
    return load_native().conv_pw_config(N * H * W, C, K, mode)


@pytest.mark.parametrize("shape", SHAPES)
def test_fwd(shape):
    c = _case(shape)
    y = load_native().conv_pw_fwd(_cl(c.x).cuda(), c.w.cuda())
    assert y.dtype == torch.bfloat16
    _check("fwd", y, c.ref[0], c.S[0], shape[1], True)


@pytest.mark.parametrize("shape", SHAPES)
def test_dgrad(shape):
    c = _case(shape)
    dx = load_native().conv_pw_dgrad(_cl(c.dy).cuda(), c.w.cuda())
    _check("dgrad", dx, c.ref[1], c.S[1], shape[2], True)


@pytest.mark.parametrize("shape", SHAPES)
def test_wgrad(shape):
    c = _case(shape)
    run = lambda: load_native().conv_pw_wgrad(  # noqa: E731
        _cl(c.dy).cuda(), _cl(c.x).cuda())
    ws = run()
    assert ws.dtype == torch.float32 and ws.shape == (shape[2], shape[1])
    _check("wgrad", ws.view_as(c.w), c.ref[2], c.S[2],
           c.M + _cfg(shape, "wgrad")[2], False)
    assert torch.equal(ws, run())   # same bits on every run


def test_plans_reach_every_loop():
    # 300 pixels in whole 128-pixel rounds: 128 + 128 + 44
    assert _cfg(SHAPES[7], "wgrad")[2:] == (3, 128)
    assert _cfg(SHAPES[0], "wgrad")[2] == 1   # written directly
    # a chunk of two staging rounds, a short last chunk
    nch, mch = _cfg(SHAPES[8], "wgrad")[2:]
    assert mch == 256 and nch >= 3 and 129 * 255 % mch != 0
    # a wave walks more than one tile and prefetches the next
    assert _cfg(SHAPES[8], "fwd")[3] >= 2
    assert _cfg(SHAPES[9], "dgrad")[3] >= 2


@pytest.mark.parametrize("leg", ["fwd", "dgrad"])
def test_inf_pixel_reaches_no_other(leg):
    # C = 24 and K = 40 both leave a granule tail in the last MFMA step: an
    # Inf pixel's bytes lie right behind its neighbour's
    c = _case(INF_CASE)
    src = (c.x if leg == "fwd" else c.dy).clone()
    src[1, :, 2, 3] = float("inf")
    keep = torch.ones(2, 1, 5, 7, dtype=torch.bool)
    keep[1, :, 2, 3] = False
    C = load_native()
    if leg == "fwd":
        got = C.conv_pw_fwd(_cl(src).cuda(), c.w.cuda())
        _check(leg, got, c.ref[0], c.S[0], INF_CASE[1], True, keep)
    else:
        got = C.conv_pw_dgrad(_cl(src).cuda(), c.w.cuda())
        _check(leg, got, c.ref[1], c.S[1], INF_CASE[2], True, keep)


def _library(*a, **k):
    raise AssertionError("library conv reached")


@pytest.mark.parametrize("knob", ["1", "0"])
def test_fda_conv2d_dispatches_pointwise(knob, monkeypatch):
    shape = SHAPES[2]
    c = _case(shape)
    monkeypatch.setenv("FLUXDIST_CONV_PW", knob)
    monkeypatch.delenv("FLUXDIST_CONV", raising=False)
    monkeypatch.setattr(conv_mod, "F", types.SimpleNamespace(conv2d=_library))
    x = _cl(c.x).cuda().requires_grad_(True)
    w = c.w.cuda().requires_grad_(True)
    if knob == "0":
        with pytest.raises(AssertionError, match="library conv reached"):
            conv_mod.fda_conv2d(x, w)
        return
    y = conv_mod.fda_conv2d(x, w)
    y.backward(_cl(c.dy).cuda())
    _check("fwd", y.detach(), c.ref[0], c.S[0], shape[1], True)
    _check("dgrad", x.grad, c.ref[1], c.S[1], shape[2], True)
    # dw is the bf16 cast of the fp32 result: one more round
    _check("wgrad", w.grad, c.ref[2], c.S[2],
           c.M + _cfg(shape, "wgrad")[2], True)


def test_multiples_of_64_stay_on_conv_igemm(monkeypatch):
    monkeypatch.setenv("FLUXDIST_CONV_PW", "1")
    monkeypatch.delenv("FLUXDIST_CONV", raising=False)
    monkeypatch.setattr(conv_mod, "F", types.SimpleNamespace(conv2d=_library))
    monkeypatch.setattr(conv_mod, "_FdaConv2dPointwise",
                        types.SimpleNamespace(apply=_library))
    c = _case((1, 64, 128, 4, 5))
    with torch.no_grad():
        y = conv_mod.fda_conv2d(_cl(c.x).cuda(), c.w.cuda())
    _check("igemm fwd", y, c.ref[0], c.S[0], 64, True)


def test_mobilenet_quarter_width_step_without_library_pointwise(monkeypatch):
    real = F.conv2d

    def library(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        if groups == 1 and tuple(w.shape[2:]) == (1, 1):
            raise AssertionError("library pointwise conv reached")
        return real(x, w, b, stride, padding, dilation, groups)

    monkeypatch.setenv("FLUXDIST_CONV_PW", "1")
    monkeypatch.delenv("FLUXDIST_CONV", raising=False)
    monkeypatch.setattr(conv_mod, "F", types.SimpleNamespace(conv2d=library))
    torch.manual_seed(0)
    model = MobileNetV1(small_input=True, width_mult=0.25).cuda()
    model = to_mixed_bf16(model.to(memory_format=torch.channels_last)).train()
    x = _cl(torch.randn(2, 3, 64, 64)).cuda().bfloat16()
    out = model(x)
    out.float().square().mean().backward()
    assert bool(torch.isfinite(out).all())
    convs = [m for m in model.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 27
    assert all(m.weight.grad is not None for m in convs)
