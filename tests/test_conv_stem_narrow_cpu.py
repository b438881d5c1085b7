"""Refusals of the conv_stem_narrow bindings, before any launch (host tensors:
the device check, made last, refuses whatever passes the others), and the
coverage of the plans conv_stem_narrow_config reports."""

import pytest
import torch

from fluxdistributed_amd.ops.native import load_native

BF16 = torch.bfloat16


def _cl(*shape, dtype=BF16):
    t = torch.zeros(*shape, dtype=dtype)
    return t.contiguous(memory_format=torch.channels_last)


# smallest valid problem: N=1, Cin=3, K=8, 4x4, stride 1
def _call(entry, x=None, w=None, dy=None, stride=1):
    C = load_native()
    x = _cl(1, 3, 4, 4) if x is None else x
    w = _cl(8, 3, 3, 3) if w is None else w
    dy = _cl(1, 8, 4, 4) if dy is None else dy
    if entry == "fwd":
        return C.conv_stem_narrow_fwd(x, w, stride)
    return C.conv_stem_narrow_wgrad(dy, x, stride)


REFUSALS = [
    ("fwd", dict(x=_cl(1, 3, 4, 4, dtype=torch.float32)),
     "x must be 4-D channels_last bf16"),
    ("wgrad", dict(dy=torch.zeros(1, 8, 4, 4, dtype=BF16)),
     "dy must be 4-D channels_last bf16"),
    ("fwd", dict(x=_cl(1, 4, 4, 4), w=_cl(8, 4, 3, 3)),
     "Cin must be 1, 2 or 3, got 4"),
    ("fwd", dict(w=_cl(12, 3, 3, 3)), r"multiple of 8 in \[8, 64\], got 12"),
    ("wgrad", dict(dy=_cl(1, 72, 4, 4)), r"multiple of 8 in \[8, 64\], got 72"),
    ("fwd", dict(stride=3), "stride must be 1 or 2, got 3"),
    ("wgrad", dict(dy=_cl(1, 8, 4, 3)),
     r"dy is \[1, .., 4, 3\] but x \[1, .., 4, 4\] at stride 1 gives "
     r"\[1, .., 4, 4\]"),
    ("fwd", dict(), "device tensors required"),
    ("wgrad", dict(), "device tensors required"),
]


@pytest.mark.skipif(torch.cuda.is_available(),
                    reason="the last refusal is that of host tensors")
@pytest.mark.parametrize("entry,operands,message", REFUSALS)
def test_conv_stem_narrow_refuses(entry, operands, message):
    with pytest.raises(RuntimeError, match=message):
        _call(entry, **operands)


# (N, Cin, K, H, W, stride): the GPU test's table and the real stems
PLANNED = [
    (1, 3, 8, 3, 5, 1), (2, 3, 32, 9, 11, 2), (1, 3, 24, 8, 8, 2),
    (1, 1, 16, 7, 6, 1), (1, 2, 40, 5, 4, 2), (2, 3, 56, 33, 37, 1),
    (1, 3, 64, 4, 130, 2), (2, 3, 56, 33, 133, 1), (1, 3, 64, 4, 262, 2),
    (64, 3, 8, 125, 20, 2),
] + [(96, 3, K, 224, 224, 2) for K in (8, 16, 24, 32)]


@pytest.mark.parametrize("mode", ["fwd", "wgrad"])
@pytest.mark.parametrize("shape", PLANNED)
def test_config_covers_every_pixel_once(shape, mode):
    N, Cin, K, H, W, s = shape
    P, Q = (H - 1) // s + 1, (W - 1) // s + 1
    th, tw, tiles_h, tiles_w, upw, nch, upc, fold_g = \
        load_native().conv_stem_narrow_config(N, H, W, Cin, K, s, mode)
    width = 16 if mode == "fwd" else 32     # pixels of one MFMA tile / step
    assert tw % width == 0 and 1 <= th <= 4 and tw <= 128
    # tiles start at multiples of (th, tw): no pixel in two, no empty tile
    assert (tiles_h - 1) * th < P <= tiles_h * th
    assert (tiles_w - 1) * tw < Q <= tiles_w * tw
    # every MFMA tile of a block tile belongs to one of the four waves
    assert upw * 4 >= th * (tw // width) > (upw - 1) * 4
    if mode == "fwd":
        assert (nch, upc, fold_g) == (1, 1, 1)
        return
    units = N * tiles_h * tiles_w
    assert th * tw <= 256
    # every unit in one chunk; only a two-level fold's padding chunks are empty
    assert nch * upc >= units and nch % fold_g == 0
    live = -(-units // upc)
    assert live <= nch < live + fold_g
    assert (fold_g == 1) == (live <= 32)
