"""Refusals of the conv_pw bindings, before any launch (host tensors: the
device check, made last, refuses whatever passes the others), and the error
text of FLUXDIST_CONV=fda."""

import types

import pytest
import torch

from fluxdistributed_amd.ops import conv as conv_mod
from fluxdistributed_amd.ops.native import load_native

BF16 = torch.bfloat16


def _cl(*shape, dtype=BF16):
    t = torch.zeros(*shape, dtype=dtype)
    return t.contiguous(memory_format=torch.channels_last)


# smallest valid problem: N=1, C=8, K=16, 4x4
def _call(entry, x=None, w=None, dy=None):
    C = load_native()
    x = _cl(1, 8, 4, 4) if x is None else x
    w = torch.zeros(16, 8, 1, 1, dtype=BF16) if w is None else w
    dy = _cl(1, 16, 4, 4) if dy is None else dy
    if entry == "fwd":
        return C.conv_pw_fwd(x, w)
    if entry == "dgrad":
        return C.conv_pw_dgrad(dy, w)
    return C.conv_pw_wgrad(dy, x)


REFUSALS = [
    ("fwd", dict(x=_cl(1, 8, 4, 4, dtype=torch.float32)),
     "x must be 4-D channels_last bf16"),
    ("wgrad", dict(dy=torch.zeros(1, 16, 4, 4, dtype=BF16)),
     "dy must be 4-D channels_last bf16"),
    ("fwd", dict(w=torch.zeros(16, 8, 1, 1)), "w must be 4-D dense bf16"),
    ("fwd", dict(w=torch.zeros(16, 8, 3, 3, dtype=BF16)),
     r"w is \[16, 8, 3, 3\] but a pointwise conv needs \[K, C, 1, 1\]"),
    ("dgrad", dict(w=torch.zeros(16, 12, 1, 1, dtype=BF16)),
     r"multiples of 8 in \[8, 256\], got C=12 K=16"),
    ("fwd", dict(w=torch.zeros(264, 8, 1, 1, dtype=BF16)),
     r"multiples of 8 in \[8, 256\], got C=8 K=264"),
    ("wgrad", dict(x=_cl(1, 4, 4, 4)), "got C=4 K=16"),
    ("fwd", dict(x=_cl(1, 16, 4, 4)),
     r"x has 16 channels but w is \[16, 8, 1, 1\]"),
    ("dgrad", dict(dy=_cl(1, 8, 4, 4)),
     r"dy has 8 channels but w is \[16, 8, 1, 1\]"),
    ("wgrad", dict(dy=_cl(1, 16, 4, 3)),
     r"dy is \[1, .., 4, 3\] but x is \[1, .., 4, 4\]"),
    ("wgrad", dict(dy=_cl(2, 16, 4, 4)), r"dy is \[2, .., 4, 4\] but x is \[1"),
    ("fwd", dict(), "device tensors required"),
    ("dgrad", dict(), "device tensors required"),
    ("wgrad", dict(), "device tensors required"),
]


@pytest.mark.parametrize("entry,operands,message", REFUSALS)
def test_conv_pw_refuses(entry, operands, message):
    with pytest.raises(RuntimeError, match=message):
        _call(entry, **operands)


def test_config_refuses_and_plans():
    cfg = load_native().conv_pw_config
    with pytest.raises(RuntimeError, match="mode must be fwd, dgrad or wgrad"):
        cfg(64, 8, 16, "bwd")
    with pytest.raises(RuntimeError, match="got C=8 K=20"):
        cfg(64, 8, 20, "fwd")
    # the pixel count a host tensor cannot reach
    with pytest.raises(RuntimeError, match="M must be in"):
        cfg(2 ** 31, 8, 16, "wgrad")
    # 300 pixels: three chunks of whole 128-pixel rounds, the last one short
    assert cfg(300, 16, 24, "wgrad") == (1, 1, 3, 128)
    # 136 outputs are three slabs, one wave each; 40 are one slab, four pixel
    # groups per block
    assert cfg(70, 72, 136, "fwd")[:2] == (3, 1)
    assert cfg(70, 24, 40, "fwd")[:2] == (1, 4)


def test_fda_error_names_conv_pw(monkeypatch):
    # fp16 operands: no native path takes them, so =fda has to raise
    monkeypatch.setenv("FLUXDIST_CONV", "fda")
    x = types.SimpleNamespace(is_cuda=True, dtype=torch.float16,
                              shape=(1, 8, 4, 4), requires_grad=False)
    w = torch.zeros(16, 8, 1, 1, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="conv_dw and conv_pw kernels"):
        conv_mod.fda_conv2d(x, w)
