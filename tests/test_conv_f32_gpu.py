"""fp32 conv kernels (conv_f32.hip) against float64 F.conv2d and its autograd.

Bound, elementwise and on every element: |got - ref| <= 2*(n + nch)*2^-24 * S
with S the same convolution / gradient in float64 on |operands|, n the
reduction length and nch the number of folded wgrad slabs. Reduction lengths
stay under 2048, so one lost or doubled product (about S/n) breaks the bound;
the wgrad test therefore takes the table's shapes with N*P*Q < 2048.
"""

import functools
import types

import pytest
import torch
import torch.nn.functional as F

from fluxdistributed_amd.ops import conv as conv_mod
from fluxdistributed_amd.ops.native import load_native

pytestmark = pytest.mark.gpu

# (N, C, H, W, K, R, stride), padding R // 2
SHAPES = [
    (2, 64, 9, 11, 64, 3, 1),       # odd extent, M=198, partial tile, borders
    (1, 64, 13, 13, 128, 3, 2),     # parity classes of unequal size
    (2, 128, 7, 7, 64, 1, 2),       # a class with no tap
    (1, 192, 8, 8, 64, 3, 1),       # several K-steps per tap, C not 2^k
    (3, 64, 20, 20, 192, 1, 1),     # several M tiles, K=192; wgrad: 10 chunks
                                    # of 128 pixels, the last one 48 (n=1200)
    (2, 128, 129, 127, 128, 1, 1),  # 128x128 fwd and dgrad tile, partial last
    (1, 1024, 6, 6, 1024, 1, 1),    # 128x128 wgrad tile, written directly
]


def _pixels(shape):
    N, _, H, W, _, _, s = shape
    return N * ((H - 1) // s + 1) * ((W - 1) // s + 1)


WGRAD_SHAPES = [s for s in SHAPES if _pixels(s) < 2048]
U = 2.0 ** -24


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded operands (fp32, CPU) and the float64 reference with its S."""
    N, C, H, W, K, R, s = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, R, generator=g)
    P = (H + 2 * (R // 2) - R) // s + 1
    Q = (W + 2 * (R // 2) - R) // s + 1
    dy = torch.randn(N, K, P, Q, generator=g)

    def run(x_, w_, dy_):
        x_ = x_.double().requires_grad_(True)
        w_ = w_.double().requires_grad_(shape in WGRAD_SHAPES)
        y = F.conv2d(x_, w_, None, s, R // 2)
        y.backward(dy_.double())
        return y.detach(), x_.grad, w_.grad

    return types.SimpleNamespace(x=x, w=w, dy=dy, ref=run(x, w, dy),
                                 S=run(x.abs(), w.abs(), dy.abs()),
                                 args=(s, s, R // 2, R // 2))


def _check(what, got, ref, S, n):
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 * n * U * S
    print(f"{what}: worst |err|/bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert got.shape == ref.shape
    assert bool((err <= bound).all())


def _wgrad(c, shape):
    N, C, H, W, K, R, s = shape
    ws = load_native().conv_f32_wgrad(_cl(c.dy).cuda(), _cl(c.x).cuda(), R, R,
                                      *c.args)
    return ws, ws.view(K, R, R, C).permute(0, 3, 1, 2)


@pytest.mark.parametrize("shape", SHAPES)
def test_fwd(shape):
    c = _case(shape)
    y = load_native().conv_f32_fwd(_cl(c.x).cuda(), _cl(c.w).cuda(), *c.args)
    assert y.dtype == torch.float32
    _check("fwd", y, c.ref[0], c.S[0], shape[5] ** 2 * shape[1])


@pytest.mark.parametrize("shape", SHAPES)
def test_dgrad(shape):
    c = _case(shape)
    dx = load_native().conv_f32_dgrad(_cl(c.dy).cuda(), _cl(c.w).cuda(),
                                      shape[2], shape[3], *c.args)
    _check("dgrad", dx, c.ref[1], c.S[1], shape[5] ** 2 * shape[4])


@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_wgrad(shape):
    c = _case(shape)
    M = _pixels(shape)
    nch = load_native().conv_f32_config(M, shape[1], shape[4], shape[5],
                                        shape[5], "wgrad")[2]
    ws, dw = _wgrad(c, shape)
    _check("wgrad", dw, c.ref[2], c.S[2], M + nch)
    assert torch.equal(ws, _wgrad(c, shape)[0])   # same bits on every run


def test_table_reaches_every_config():
    cfg = load_native().conv_f32_config
    tiles = {m: set() for m in ("fwd", "dgrad", "wgrad")}
    for (N, C, H, W, K, R, s) in SHAPES:
        M = _pixels((N, C, H, W, K, R, s))
        tiles["fwd"].add(cfg(M, C, K, R, R, "fwd")[:2])
        tiles["dgrad"].add(cfg(N * -(-H // s) * -(-W // s), C, K, R, R,
                               "dgrad")[:2])
        if (N, C, H, W, K, R, s) in WGRAD_SHAPES:
            tiles["wgrad"].add(cfg(M, C, K, R, R, "wgrad")[:2])
    assert all(t == {(64, 64), (128, 128)} for t in tiles.values()), tiles
    # three or more chunks with a short last one: 9 * 128 + 48 pixels
    assert cfg(1200, 64, 192, 1, 1, "wgrad") == (64, 64, 10, 128)


@pytest.mark.parametrize("knob", ["1", "0"])
def test_fda_conv2d_dispatches_fp32(knob, monkeypatch):
    shape = SHAPES[1]
    c = _case(shape)

    def library(*a, **k):
        raise AssertionError("library conv reached")

    monkeypatch.setenv("FLUXDIST_CONV_F32", knob)
    monkeypatch.delenv("FLUXDIST_CONV", raising=False)
    monkeypatch.setattr(conv_mod, "F", types.SimpleNamespace(conv2d=library))
    x = _cl(c.x).cuda().requires_grad_(True)
    w = _cl(c.w).cuda().requires_grad_(True)
    if knob == "0":
        with pytest.raises(AssertionError, match="library conv reached"):
            conv_mod.fda_conv2d(x, w, shape[6], shape[5] // 2)
        return
    y = conv_mod.fda_conv2d(x, w, shape[6], shape[5] // 2)
    y.backward(_cl(c.dy).cuda())
    N, C, H, W, K, R, s = shape
    _check("fwd", y.detach(), c.ref[0], c.S[0], R * R * C)
    _check("dgrad", x.grad, c.ref[1], c.S[1], R * R * K)
    _check("wgrad", w.grad, c.ref[2], c.S[2], _pixels(shape) + 1)
