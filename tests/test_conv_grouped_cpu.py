"""Refusals of the conv_grouped bindings, before any launch (host tensors:
the device check, made last, refuses whatever passes the others), and the
ResNeXt models: parameter counts and a CPU forward."""

import pytest
import torch

from fluxdistributed_amd.models import build_model
from fluxdistributed_amd.ops.native import load_native

BF16 = torch.bfloat16


def _cl(*shape, dtype=BF16):
    t = torch.zeros(*shape, dtype=dtype)
    return t.contiguous(memory_format=torch.channels_last)


# smallest valid problem: N=1, C=K=64, 4x4, 16 groups of 4, stride 1
def _call(entry, x=None, w=None, dy=None, stride=(1, 1), groups=16):
    C = load_native()
    x = _cl(1, 64, 4, 4) if x is None else x
    w = _cl(64, 4, 3, 3) if w is None else w
    dy = _cl(1, 64, 4, 4) if dy is None else dy
    if entry == "fwd":
        return C.conv_grouped_fwd(x, w, *stride, 1, 1, groups)
    if entry == "dgrad":
        return C.conv_grouped_dgrad(dy, w, 4, 4, *stride, 1, 1, groups)
    return C.conv_grouped_wgrad(dy, x, *stride, 1, 1, groups)


REFUSALS = [
    ("fwd", dict(), "device tensors required"),
    ("dgrad", dict(), "device tensors required"),
    ("wgrad", dict(), "device tensors required"),
    ("fwd", dict(x=_cl(1, 64, 4, 4, dtype=torch.float32)),
     "x must be 4-D channels_last bf16"),
    ("wgrad", dict(dy=torch.zeros(1, 64, 4, 4, dtype=BF16)),
     "dy must be 4-D channels_last bf16"),
    ("fwd", dict(w=_cl(64, 2, 3, 3), groups=32), "must be 4, 8, 16 or 32, got 2"),
    ("dgrad", dict(w=_cl(64, 64, 3, 3), groups=1), "must be 4, 8, 16 or 32, got 64"),
    ("fwd", dict(w=_cl(128, 4, 3, 3)), "needs C/g == K/g, got C/g=4 K/g=8"),
    ("wgrad", dict(x=_cl(1, 32, 4, 4), dy=_cl(1, 32, 4, 4), groups=8),
     "multiples of 64, got C=32"),
    ("fwd", dict(stride=(1, 2)), r"stride must be \(1,1\) or \(2,2\), got 1x2"),
    ("fwd", dict(w=_cl(64, 4, 1, 1)), "3x3 filter with padding 1, got 1x1"),
    ("dgrad", dict(dy=_cl(1, 64, 2, 2)), "dy is 2x2 but .* output of 4x4"),
    ("wgrad", dict(dy=_cl(1, 64, 4, 3)), "dy is 4x3 but .* output of 4x4"),
]


@pytest.mark.parametrize("entry,operands,message", REFUSALS)
def test_conv_grouped_refuses(entry, operands, message):
    with pytest.raises(RuntimeError, match=message):
        _call(entry, **operands)


@pytest.mark.parametrize("name,params", [
    ("resnext50_32x4d", 25_028_904),
    ("resnext101_32x4d", 44_177_704),
    ("resnext101_64x4d", 83_455_272),
])
def test_resnext_builds(name, params):
    assert sum(p.numel() for p in build_model(name).parameters()) == params
    model = build_model(name, num_classes=10, small_input=True).eval()
    with torch.no_grad():
        out = model(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 10) and bool(torch.isfinite(out).all())
