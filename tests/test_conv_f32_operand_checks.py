"""Every refusal of the conv_f32 bindings, before any launch.

CPU-only by construction: skipped wherever a GPU is visible, so a regression
in a check can never hand a host pointer or a short buffer to a kernel.
"""

import pytest
import torch

from fluxdistributed_amd.ops.native import load_native

if torch.cuda.is_available():  # pragma: no cover
    pytest.skip("CPU-only: must never reach a launch", allow_module_level=True)

C = load_native()
if C is None:  # pragma: no cover
    pytest.skip("native extension not built", allow_module_level=True)


def _cl(*shape, dtype=torch.float32):
    t = torch.zeros(*shape, dtype=dtype)
    return t.contiguous(memory_format=torch.channels_last)


# smallest valid problem: N=1, C=K=64, 4x4, 3x3 filter, stride 1, padding 1
X, W, DY = _cl(1, 64, 4, 4), _cl(64, 64, 3, 3), _cl(1, 64, 4, 4)
CALLS = {
    "fwd": lambda x=X, w=W, dy=DY: C.conv_f32_fwd(x, w, 1, 1, 1, 1),
    "dgrad": lambda x=X, w=W, dy=DY: C.conv_f32_dgrad(dy, w, 4, 4, 1, 1, 1, 1),
    "wgrad": lambda x=X, w=W, dy=DY: C.conv_f32_wgrad(dy, x, 3, 3, 1, 1, 1, 1),
}
BF16 = torch.bfloat16
REFUSALS = [
    ("fwd", dict(), "device tensors required"),
    ("dgrad", dict(), "device tensors required"),
    ("wgrad", dict(), "device tensors required"),
    ("fwd", dict(x=_cl(1, 64, 4, 4, dtype=BF16)), "x must be 4-D channels_last fp32"),
    ("fwd", dict(w=_cl(64, 64, 3, 3, dtype=BF16)), "w must be 4-D channels_last fp32"),
    ("dgrad", dict(dy=_cl(1, 64, 4, 4, dtype=BF16)), "dy must be 4-D channels_last fp32"),
    ("wgrad", dict(x=_cl(1, 64, 4, 4, dtype=BF16)), "x must be 4-D channels_last fp32"),
    ("fwd", dict(x=torch.zeros(1, 64, 4, 4)), "x must be 4-D channels_last fp32"),
    ("dgrad", dict(w=torch.zeros(64, 64, 3, 3)), "w must be 4-D channels_last fp32"),
    ("wgrad", dict(dy=torch.zeros(1, 64, 4, 4)), "dy must be 4-D channels_last fp32"),
    ("fwd", dict(x=_cl(1, 32, 4, 4), w=_cl(64, 32, 3, 3)), "multiples of 64, got C=32"),
    ("dgrad", dict(dy=_cl(1, 96, 4, 4), w=_cl(96, 64, 3, 3)), "multiples of 64, got C=64 K=96"),
    ("wgrad", dict(x=_cl(1, 96, 4, 4)), "multiples of 64, got C=96"),
    ("fwd", dict(w=_cl(64, 128, 3, 3)), "channel mismatch: x has 64, w has 128"),
    ("dgrad", dict(dy=_cl(1, 128, 4, 4)), "channel mismatch: dy has 128, w has 64"),
    ("dgrad", dict(dy=_cl(1, 64, 2, 2)), "dy is 2x2 but .* output of 4x4"),
    ("wgrad", dict(dy=_cl(1, 64, 2, 2)), "dy is 2x2 but .* output of 4x4"),
    ("wgrad", dict(x=_cl(2, 64, 4, 4)), "batch size mismatch: dy has 1, x has 2"),
]


@pytest.mark.parametrize("entry,operands,message", REFUSALS)
def test_conv_f32_refuses(entry, operands, message):
    with pytest.raises(RuntimeError, match=message):
        CALLS[entry](**operands)


def test_conv_f32_config_refuses_bad_geometry():
    with pytest.raises(RuntimeError, match="bad geometry"):
        C.conv_f32_config(64, 32, 64, 1, 1, "fwd")
    with pytest.raises(RuntimeError, match="mode must be"):
        C.conv_f32_config(64, 64, 64, 1, 1, "stem")
