"""The conv_igemm entry points refuse host tensors before any launch.

CPU-only by construction: the module is skipped wherever a GPU is visible,
so a regression in the check can never hand a host pointer to a kernel.
"""

import pytest
import torch

from fluxdistributed_amd.ops.native import load_native

if torch.cuda.is_available():  # pragma: no cover
    pytest.skip("CPU-only: must never reach a launch", allow_module_level=True)

C = load_native()
if C is None:  # pragma: no cover
    pytest.skip("native extension not built", allow_module_level=True)


def _cl(*shape):
    t = torch.zeros(*shape, dtype=torch.bfloat16)
    return t.contiguous(memory_format=torch.channels_last)


# smallest valid shape: N=1, C=K=64, 4x4, 1x1 filter, stride 1, no padding
X = _cl(1, 64, 4, 4)
W = _cl(64, 64, 1, 1)
DY = _cl(1, 64, 4, 4)
WT = torch.zeros(64, 64, dtype=torch.bfloat16)          # [R*S*C][K]
WS = torch.zeros(64, 64, dtype=torch.float32)           # [K][R*S*C]

CALLS = {
    "fwd": lambda: C.conv_igemm_fwd(X, W, 1, 1, 0, 0),
    "fwd_stats": lambda: C.conv_igemm_fwd_stats(X, W, 1, 1, 0, 0),
    "dgrad": lambda: C.conv_igemm_dgrad(DY, WT, 64, 4, 4, 1, 1, 1, 1, 0, 0),
    "wgrad": lambda: C.conv_igemm_wgrad(DY, X, 1, 1, 1, 1, 0, 0),
    "wgrad_into": lambda: C.conv_igemm_wgrad_into(DY, X, WS, 1, 1, 1, 1, 0, 0),
}


@pytest.mark.parametrize("entry", sorted(CALLS))
def test_conv_entry_point_refuses_cpu_tensors(entry):
    # match the operand check's own message: without a GPU a later runtime
    # call would raise too, which is not the check under test
    with pytest.raises(RuntimeError, match="device tensors required"):
        CALLS[entry]()


def test_conv_fwd_stats_refuses_c32():
    with pytest.raises(RuntimeError):
        C.conv_igemm_fwd_stats(_cl(1, 32, 4, 4), _cl(64, 32, 1, 1), 1, 1, 0, 0)
