"""Refusals of the conv_dw bindings, before any launch (host tensors: the
device check, made last, refuses whatever passes the others), and the
MobileNetV1 model: parameter count and a CPU forward."""

import pytest
import torch

from fluxdistributed_amd.models import build_model
from fluxdistributed_amd.ops.native import load_native

BF16 = torch.bfloat16


def _cl(*shape, dtype=BF16):
    t = torch.zeros(*shape, dtype=dtype)
    return t.contiguous(memory_format=torch.channels_last)


# smallest valid problem: N=1, C=8, 4x4, stride 1
def _call(entry, x=None, w=None, dy=None, stride=(1, 1)):
    C = load_native()
    x = _cl(1, 8, 4, 4) if x is None else x
    w = torch.zeros(8, 1, 3, 3, dtype=BF16) if w is None else w
    dy = _cl(1, 8, 4, 4) if dy is None else dy
    if entry == "fwd":
        return C.conv_dw_fwd(x, w, *stride)
    if entry == "dgrad":
        return C.conv_dw_dgrad(dy, w, 4, 4, *stride)
    return C.conv_dw_wgrad(dy, x, *stride)


REFUSALS = [
    ("fwd", dict(), "device tensors required"),
    ("dgrad", dict(), "device tensors required"),
    ("wgrad", dict(), "device tensors required"),
    ("fwd", dict(x=_cl(1, 8, 4, 4, dtype=torch.float32)),
     "x must be 4-D channels_last bf16"),
    ("wgrad", dict(dy=torch.zeros(1, 8, 4, 4, dtype=BF16)),
     "dy must be 4-D channels_last bf16"),
    ("fwd", dict(w=torch.zeros(8, 1, 3, 3)), "w must be 4-D dense bf16"),
    ("fwd", dict(w=torch.zeros(8, 2, 3, 3, dtype=BF16)),
     r"w is \[8, 2, 3, 3\] but .* needs \[8, 1, 3, 3\]"),
    ("dgrad", dict(w=torch.zeros(16, 1, 3, 3, dtype=BF16)),
     r"w is \[16, 1, 3, 3\] but .* needs \[8, 1, 3, 3\]"),
    ("fwd", dict(w=torch.zeros(8, 1, 1, 1, dtype=BF16)),
     r"w is \[8, 1, 1, 1\]"),
    ("fwd", dict(x=_cl(1, 12, 4, 4)), "multiple of 8, got C=12"),
    ("wgrad", dict(x=_cl(1, 4, 4, 4), dy=_cl(1, 4, 4, 4)),
     "multiple of 8, got C=4"),
    ("fwd", dict(stride=(1, 2)), r"stride must be \(1,1\) or \(2,2\), got 1x2"),
    ("dgrad", dict(dy=_cl(1, 8, 2, 2)), "dy is 2x2 but .* output of 4x4"),
    ("wgrad", dict(dy=_cl(1, 8, 4, 3)), "dy is 4x3 but .* output of 4x4"),
    ("wgrad", dict(dy=_cl(2, 8, 4, 4)), r"dy is \[2, 8, ..\] but x is \[1, 8"),
]


@pytest.mark.parametrize("entry,operands,message", REFUSALS)
def test_conv_dw_refuses(entry, operands, message):
    with pytest.raises(RuntimeError, match=message):
        _call(entry, **operands)


def test_mobilenet_v1_builds():
    model = build_model("mobilenet_v1")
    assert sum(p.numel() for p in model.parameters()) == 4_231_976
    model = build_model("mobilenet_v1", num_classes=10, small_input=True).eval()
    with torch.no_grad():
        out = model(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 10) and bool(torch.isfinite(out).all())
