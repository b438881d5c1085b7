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


# Geometry refusals: every operand but the one under test is the smallest
# valid one, and each refusal is matched on its own message (all of them
# come before the device check, so they are reachable here).
FWD = {"fwd": C.conv_igemm_fwd, "fwd_stats": C.conv_igemm_fwd_stats}


@pytest.mark.parametrize("entry", sorted(FWD))
def test_conv_fwd_refuses_stride_0(entry):
    with pytest.raises(RuntimeError, match="bad stride/padding"):
        FWD[entry](X, W, 0, 1, 0, 0)
    with pytest.raises(RuntimeError, match="bad stride/padding"):
        FWD[entry](X, W, 1, 0, 0, 0)


@pytest.mark.parametrize("entry", sorted(FWD))
def test_conv_fwd_refuses_filter_larger_than_input(entry):
    with pytest.raises(RuntimeError, match="filter 5x5 larger than the padded input 4x4"):
        FWD[entry](X, _cl(64, 64, 5, 5), 1, 1, 0, 0)


@pytest.mark.parametrize("entry", sorted(FWD))
def test_conv_fwd_refuses_split_k_wider_than_the_combine(entry):
    # 3x3 on C=384 is 54 K-steps deep and 1x32 tiles underfill the chip, so
    # the plan splits K; the combine kernel covers at most 2048 channels
    assert C.conv_igemm_fwd_config(16, 384, 4096, 3, 3)[2] == 4
    with pytest.raises(RuntimeError, match="split-K shapes need at most 2048"):
        FWD[entry](_cl(1, 384, 4, 4), _cl(4096, 384, 3, 3), 1, 1, 1, 1)


def test_conv_dgrad_refuses_dy_of_another_geometry():
    # a 3x3 filter without padding maps 4x4 to 2x2, not to dy's 4x4
    wt = torch.zeros(9 * 64, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="dy is 4x4 but .* output of 2x2"):
        C.conv_igemm_dgrad(DY, wt, 64, 4, 4, 3, 3, 1, 1, 0, 0)


def test_conv_dgrad_refuses_accum_of_wrong_sizes():
    # the right numel, another shape: dx is [1,64,4,4]
    with pytest.raises(RuntimeError, match="accum must be channels_last bf16 of dx's shape"):
        C.conv_igemm_dgrad(DY, WT, 64, 4, 4, 1, 1, 1, 1, 0, 0, _cl(1, 64, 2, 8))
    # a valid accum gets as far as the device check
    with pytest.raises(RuntimeError, match="device tensors required"):
        C.conv_igemm_dgrad(DY, WT, 64, 4, 4, 1, 1, 1, 1, 0, 0, _cl(1, 64, 4, 4))


def test_conv_dgrad_refuses_misaligned_accum():
    # the staged epilogue reads accum as 16-B vectors
    off = torch.zeros(64 * 16 + 1, dtype=torch.bfloat16)[1:]
    acc = off.view(1, 4, 4, 64).permute(0, 3, 1, 2)
    with pytest.raises(RuntimeError, match="accum must be 16-byte aligned"):
        C.conv_igemm_dgrad(DY, WT, 64, 4, 4, 1, 1, 1, 1, 0, 0, acc)


WGRAD = {
    "wgrad": lambda dy, x, ws: C.conv_igemm_wgrad(dy, x, 1, 1, 1, 1, 0, 0),
    "wgrad_into": lambda dy, x, ws: C.conv_igemm_wgrad_into(
        dy, x, ws, 1, 1, 1, 1, 0, 0),
}


@pytest.mark.parametrize("entry", sorted(WGRAD))
def test_conv_wgrad_refuses_short_dy(entry):
    # N comes from x: a dy of batch 1 would be read out of bounds
    with pytest.raises(RuntimeError, match="batch size mismatch: dy has 1, x has 2"):
        WGRAD[entry](DY, _cl(2, 64, 4, 4), WS)


@pytest.mark.parametrize("entry", sorted(WGRAD))
def test_conv_wgrad_refuses_dy_of_another_geometry(entry):
    with pytest.raises(RuntimeError, match="dy is 2x2 but .* output of 4x4"):
        WGRAD[entry](_cl(1, 64, 2, 2), X, WS)


def test_conv_wgrad_into_refuses_wrong_size_ws():
    with pytest.raises(RuntimeError, match="ws must be contiguous Float with 4096"):
        C.conv_igemm_wgrad_into(DY, X, torch.zeros(64, 32), 1, 1, 1, 1, 0, 0)
    with pytest.raises(RuntimeError, match="ws must be contiguous Float with 4096"):
        C.conv_igemm_wgrad_into(DY, X, WS.to(torch.float64), 1, 1, 1, 1, 0, 0)
