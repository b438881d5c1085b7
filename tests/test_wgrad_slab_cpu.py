"""Operand refusals of the slab wgrad bindings, and the slab/atomic rule.

Every shape, dtype and layout check runs before the device check, so each
refusal is reachable with host tensors; a call that passes them all must end
at "device tensors required". conv_igemm_wgrad_mode is host arithmetic: it
never sends one or two chunks to slabs (those sums are order-independent
already), and its choice for the ten ResNet-34 batch-96 shapes is pinned to
what was measured (profiles/wgrad_slab.md).
"""

import pytest
import torch

from fluxdistributed_amd.ops.native import load_native

C = load_native()
if C is None:  # pragma: no cover
    pytest.skip("native extension not built", allow_module_level=True)

from test_wgrad_raster_cpu import BODY, PINNED  # noqa: E402


def _cl(*shape):
    t = torch.zeros(*shape, dtype=torch.bfloat16)
    return t.contiguous(memory_format=torch.channels_last)


# N=2, C=K=64, 48x48, 1x1 filter: M = 4608 pixels, 11 chunks of 448
X = _cl(2, 64, 48, 48)
DY = _cl(2, 64, 48, 48)
NCH = 11
N_OUT = 64 * 64
ARGS = (1, 1, 1, 1, 0, 0)


def test_the_shape_under_test_has_the_chunks_it_claims():
    assert C.conv_igemm_wgrad_config(2 * 48 * 48, 64, 64, 1, 1)[2] == NCH


def test_valid_calls_reach_the_device_check():
    with pytest.raises(RuntimeError, match="device tensors required"):
        C.conv_igemm_wgrad_slabs_into(DY, X, torch.zeros(NCH * N_OUT), *ARGS)
    with pytest.raises(RuntimeError, match="device tensors required"):
        C.wgrad_slab_fold(torch.zeros(NCH * N_OUT), NCH, torch.zeros(N_OUT))
    with pytest.raises(RuntimeError, match="device tensors required"):
        C.wgrad_slab_fold(torch.zeros(NCH * N_OUT), NCH,
                          torch.zeros(N_OUT, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="device tensors required"):
        C.conv_igemm_wgrad_flush(
            DY, X, torch.zeros(N_OUT, dtype=torch.bfloat16), *ARGS)


def test_slabs_into_refuses_a_slab_that_does_not_match_the_plan():
    # one chunk short, one chunk long, the atomic workspace's size
    for numel in ((NCH - 1) * N_OUT, (NCH + 1) * N_OUT, N_OUT):
        with pytest.raises(RuntimeError, match=f"with {NCH * N_OUT} elements"):
            C.conv_igemm_wgrad_slabs_into(DY, X, torch.zeros(numel), *ARGS)


def test_slabs_into_refuses_wrong_dtype_and_layout():
    with pytest.raises(RuntimeError, match="slab .* must be contiguous Float"):
        C.conv_igemm_wgrad_slabs_into(
            DY, X, torch.zeros(NCH * N_OUT, dtype=torch.float64), *ARGS)
    with pytest.raises(RuntimeError, match="slab .* must be contiguous Float"):
        C.conv_igemm_wgrad_slabs_into(
            DY, X, torch.zeros(NCH * N_OUT, 2)[:, 0], *ARGS)
    with pytest.raises(RuntimeError, match="slab must be 1-D"):
        C.conv_igemm_wgrad_slabs_into(
            DY, X, torch.zeros(NCH, N_OUT), *ARGS)
    with pytest.raises(RuntimeError, match="slab must be 16-byte aligned"):
        C.conv_igemm_wgrad_slabs_into(
            DY, X, torch.zeros(NCH * N_OUT + 1)[1:], *ARGS)


def test_slab_entry_points_check_the_conv_geometry():
    slab = torch.zeros(NCH * N_OUT)
    g = torch.zeros(N_OUT, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="batch size mismatch"):
        C.conv_igemm_wgrad_slabs_into(_cl(1, 64, 48, 48), X, slab, *ARGS)
    with pytest.raises(RuntimeError, match="batch size mismatch"):
        C.conv_igemm_wgrad_flush(_cl(1, 64, 48, 48), X, g, *ARGS)
    with pytest.raises(RuntimeError, match="dy is 24x24 but .* output of 48x48"):
        C.conv_igemm_wgrad_flush(_cl(2, 64, 24, 24), X, g, *ARGS)


def test_fold_refuses_a_chunk_count_that_does_not_match_the_slab():
    out = torch.zeros(N_OUT)
    for nch in (NCH - 1, NCH + 1):
        with pytest.raises(RuntimeError,
                           match=f"with {nch * N_OUT} elements"):
            C.wgrad_slab_fold(torch.zeros(NCH * N_OUT), nch, out)
    with pytest.raises(RuntimeError, match="bad chunk count 0"):
        C.wgrad_slab_fold(torch.zeros(0), 0, out)


def test_fold_refuses_wrong_dtypes_layouts_and_sizes():
    slab = torch.zeros(NCH * N_OUT)
    with pytest.raises(RuntimeError, match="out must be fp32 .* or bf16"):
        C.wgrad_slab_fold(slab, NCH, torch.zeros(N_OUT, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="out must be contiguous"):
        C.wgrad_slab_fold(slab, NCH, torch.zeros(N_OUT, 2)[:, 0])
    with pytest.raises(RuntimeError, match="slab .* must be contiguous Float"):
        C.wgrad_slab_fold(slab.double(), NCH, torch.zeros(N_OUT))
    with pytest.raises(RuntimeError, match="multiple of 4 elements, got 6"):
        C.wgrad_slab_fold(torch.zeros(12), 2, torch.zeros(6))
    with pytest.raises(RuntimeError, match="out must be aligned"):
        C.wgrad_slab_fold(slab, NCH, torch.zeros(N_OUT + 1)[1:])
    with pytest.raises(RuntimeError, match="out must be aligned"):
        C.wgrad_slab_fold(
            slab, NCH, torch.zeros(N_OUT + 1, dtype=torch.bfloat16)[1:])
    with pytest.raises(RuntimeError, match="slab must be 16-byte aligned"):
        C.wgrad_slab_fold(torch.zeros(NCH * N_OUT + 1)[1:], NCH,
                          torch.zeros(N_OUT))


def test_flush_refuses_a_g_that_is_not_the_flat_slice():
    with pytest.raises(RuntimeError, match="g must be contiguous BFloat16"):
        C.conv_igemm_wgrad_flush(DY, X, torch.zeros(N_OUT), *ARGS)
    with pytest.raises(RuntimeError, match=f"with {N_OUT} elements"):
        C.conv_igemm_wgrad_flush(
            DY, X, torch.zeros(N_OUT - 64, dtype=torch.bfloat16), *ARGS)
    with pytest.raises(RuntimeError, match="g must be contiguous BFloat16"):
        C.conv_igemm_wgrad_flush(
            DY, X, torch.zeros(N_OUT, 2, dtype=torch.bfloat16)[:, 0], *ARGS)
    with pytest.raises(RuntimeError, match="g must be 8-byte aligned"):
        C.conv_igemm_wgrad_flush(
            DY, X, torch.zeros(N_OUT + 1, dtype=torch.bfloat16)[1:], *ARGS)


def test_mode_refuses_bad_geometry():
    with pytest.raises(RuntimeError, match="bad geometry"):
        C.conv_igemm_wgrad_mode(0, 64, 64, 3, 3)
    with pytest.raises(RuntimeError, match="bad geometry"):
        C.conv_igemm_wgrad_mode(4096, 32, 64, 3, 3)


@pytest.mark.parametrize("shape", [s for s in BODY if s[0] <= 4096])
def test_one_or_two_chunks_stay_on_atomics(shape):
    assert C.conv_igemm_wgrad_config(*shape)[2] <= 2
    assert C.conv_igemm_wgrad_mode(*shape) == "atomic"


def test_mode_never_picks_slabs_below_three_chunks():
    for shape in BODY:
        if C.conv_igemm_wgrad_config(*shape)[2] <= 2:
            assert C.conv_igemm_wgrad_mode(*shape) == "atomic", shape


# the measured choice for the ten flagship shapes (profiles/wgrad_slab.md):
# the four FT4 plans, 28 to 33 MB of slabs, gain; the six FT2 ones, 5.5 to
# 12.4 MB, do not
MODE = {shape: "slab" if PINNED[shape][0] == 4 else "atomic"
        for shape in PINNED}


def test_flagship_slab_shapes_are_the_four_measured():
    assert sorted(s for s in MODE if MODE[s] == "slab") == [
        (4704, 256, 512, 3, 3), (4704, 512, 512, 3, 3),
        (18816, 256, 256, 3, 3), (75264, 128, 128, 3, 3)]


@pytest.mark.parametrize("shape", sorted(MODE))
def test_flagship_mode_is_pinned(shape):
    assert C.conv_igemm_wgrad_mode(*shape) == MODE[shape]
