"""Narrow stem conv kernels (conv_stem_narrow.hip) against float64 F.conv2d
and its autograd on the CPU, from the bf16-rounded operands.

Products of bf16 values are exact in fp32, so the bounds are derived. With S
the same computation on |operands| and U = 2^-24:
  fwd (one bf16 round), E = 2*(9*Cin)*U*S:   |err| <= E + 2^-8*(|ref| + E)
  wgrad (fp32 out), M = N*P*Q pixels, nch slabs:  |err| <= 2*(M + nch)*U*S
  through fda_conv2d (dw rounded to bf16): the wgrad bound plus the 2^-8 term
on every element. Worst measured |err|/bound on the MI355X over the table:
fwd 0.994 (the bf16 round itself), wgrad 0.063; through fda_conv2d fwd 0.958
and the bf16 dw 0.924; with an Inf pixel fwd 0.958.
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

# (N, Cin, K, H, W, stride)
SHAPES = [
    (1, 3, 8, 3, 5, 1),      # K half a 16-block; 15 pixels, all on the border
    (2, 3, 32, 9, 11, 2),    # the MobileNet stem in small; odd H, W
    (1, 3, 24, 8, 8, 2),     # K % 16 == 8 with two blocks; even extents
    (1, 1, 16, 7, 6, 1),     # Cin = 1: 23 of the 32 reduction slots are padding
    (1, 2, 40, 5, 4, 2),     # Cin = 2; the last block is half a 16-block
    # tiles are up to 128 columns wide: these two rows are wider than 37 and
    # 130 columns so that they still cross a tile edge
    (2, 3, 56, 33, 133, 1),  # 2 x 33 tiles; wgrad: 72 slabs, a two-level fold
    (1, 3, 64, 4, 262, 2),   # a row wider than a tile (Q = 131), widest K
    (64, 3, 8, 125, 20, 2),  # enough blocks for 4-row forward tiles, P % 4 != 0
]
U = 2.0 ** -24
INF_CASE = SHAPES[1]


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded bf16 operands (CPU) and the float64 reference with its S."""
    N, Cin, K, H, W, s = shape
    P, Q = (H - 1) // s + 1, (W - 1) // s + 1
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, Cin, H, W, generator=gen).bfloat16()
    w = torch.randn(K, Cin, 3, 3, generator=gen).bfloat16()
    dy = torch.randn(N, K, P, Q, generator=gen).bfloat16()

    def run(x_, w_, dy_):
        w_ = w_.double().requires_grad_(True)
        y = F.conv2d(x_.double(), w_, None, s, 1)
        y.backward(dy_.double())
        return y.detach(), w_.grad

    return types.SimpleNamespace(x=x, w=w, dy=dy, ref=run(x, w, dy),
                                 S=run(x.abs(), w.abs(), dy.abs()),
                                 M=N * P * Q)


def _check(what, got, ref, S, n, rounded, keep=None):
    got = got.double().cpu()
    err = (got - ref).abs()
    bound = 2.0 * n * U * S
    if rounded:
        bound = bound + 2.0 ** -8 * (ref.abs() + bound)
    if keep is not None:   # [N,1,P,Q] mask of the pixels that are compared
        assert bool(torch.isfinite(got[keep.expand_as(got)]).all())
        assert not bool(torch.isfinite(got[~keep.expand_as(got)]).any())
        err = torch.where(keep, err, torch.zeros_like(err))
    print(f"{what}: worst |err|/bound = "
          f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert got.shape == ref.shape
    assert bool((err <= bound).all())


def _nch(shape):
    N, Cin, K, H, W, s = shape
    return load_native().conv_stem_narrow_config(N, H, W, Cin, K, s,
                                                 "wgrad")[5]


@pytest.mark.parametrize("shape", SHAPES)
def test_fwd(shape):
    c = _case(shape)
    y = load_native().conv_stem_narrow_fwd(_cl(c.x).cuda(), _cl(c.w).cuda(),
                                           shape[5])
    assert y.dtype == torch.bfloat16
    _check("fwd", y, c.ref[0], c.S[0], 9 * shape[1], True)


@pytest.mark.parametrize("shape", SHAPES)
def test_wgrad(shape):
    c = _case(shape)
    N, Cin, K = shape[:3]
    run = lambda: load_native().conv_stem_narrow_wgrad(  # noqa: E731
        _cl(c.dy).cuda(), _cl(c.x).cuda(), shape[5])
    ws = run()
    assert ws.dtype == torch.float32 and ws.shape == (K, 9 * Cin)
    _check("wgrad", ws.view(K, 3, 3, Cin).permute(0, 3, 1, 2), c.ref[1],
           c.S[1], c.M + _nch(shape), False)
    assert torch.equal(ws, run())   # same bits on every run


def test_inf_pixel_reaches_its_windows_only():
    # a padded slot that is zero on one side only would spread NaN
    N, Cin, K, H, W, s = INF_CASE
    c = _case(INF_CASE)
    x = c.x.clone()
    x[1, :, 4, 5] = float("inf")
    hit = torch.zeros(N, 1, H, W, dtype=torch.float64)
    hit[1, 0, 4, 5] = 1.0
    keep = F.conv2d(hit, torch.ones(1, 1, 3, 3, dtype=torch.float64), None,
                    s, 1) == 0
    assert int((~keep).sum()) == 2
    y = load_native().conv_stem_narrow_fwd(_cl(x).cuda(), _cl(c.w).cuda(), s)
    _check("fwd, Inf pixel", y, c.ref[0], c.S[0], 9 * Cin, True, keep)


def _library(*a, **k):
    raise AssertionError("library conv reached")


@pytest.mark.parametrize("knob", ["1", "0"])
def test_fda_conv2d_dispatches_narrow_stem(knob, monkeypatch):
    shape = SHAPES[1]
    c = _case(shape)
    monkeypatch.setenv("FLUXDIST_CONV_STEM_NARROW", knob)
    monkeypatch.delenv("FLUXDIST_CONV", raising=False)
    monkeypatch.setattr(conv_mod, "F", types.SimpleNamespace(conv2d=_library))
    x = _cl(c.x).cuda()
    w = c.w.cuda().requires_grad_(True)
    if knob == "0":
        with pytest.raises(AssertionError, match="library conv reached"):
            conv_mod.fda_conv2d(x, w, 2, 1)
        return
    y = conv_mod.fda_conv2d(x, w, 2, 1)
    y.backward(_cl(c.dy).cuda(), retain_graph=True)
    _check("fwd", y.detach(), c.ref[0], c.S[0], 9 * shape[1], True)
    # dw is the bf16 cast of the fp32 result: one more round
    assert w.grad.shape == c.w.shape
    _check("wgrad", w.grad, c.ref[1], c.S[1], c.M + _nch(shape), True)
    # x itself is saved, not a pooled buffer: a second backward works
    first = w.grad.clone()
    w.grad = None
    y.backward(_cl(c.dy).cuda())
    assert torch.equal(w.grad, first)


@pytest.mark.parametrize("width", [0.25, 0.5, 0.75, 1.0])
def test_mobilenet_step_reaches_no_library_conv_or_bn(width, monkeypatch):
    from fluxdistributed_amd.models import mobilenet as mobilenet_mod
    for knob in ("FLUXDIST_CONV_STEM_NARROW", "FLUXDIST_BN_NARROW",
                 "FLUXDIST_CONV_PW"):
        monkeypatch.setenv(knob, "1")
    monkeypatch.delenv("FLUXDIST_CONV", raising=False)
    monkeypatch.setattr(conv_mod, "F", types.SimpleNamespace(conv2d=_library))
    monkeypatch.setattr(mobilenet_mod, "F",
                        types.SimpleNamespace(batch_norm=_library))
    torch.manual_seed(0)
    model = MobileNetV1(num_classes=10, width_mult=width).cuda()
    model = to_mixed_bf16(model.to(memory_format=torch.channels_last)).train()
    out = model(_cl(torch.randn(2, 3, 64, 64)).cuda().bfloat16())
    out.float().square().mean().backward()
    assert bool(torch.isfinite(out).all())


def test_fda_mode_runs_mobilenet(monkeypatch):
    monkeypatch.setenv("FLUXDIST_CONV", "fda")
    torch.manual_seed(0)
    model = MobileNetV1(num_classes=10, small_input=True, width_mult=0.5).cuda()
    model = to_mixed_bf16(model.to(memory_format=torch.channels_last)).train()
    x = _cl(torch.randn(2, 3, 16, 16)).cuda().bfloat16()
    out = model(x)
    out.float().square().mean().backward()
    g = model.conv1.weight.grad
    assert g is not None and g.shape == model.conv1.weight.shape
    assert bool(torch.isfinite(g).all())
