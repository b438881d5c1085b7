"""grad_mean_multi refuses bad operand lists before any launch.

CPU-only by construction: the module is skipped wherever a GPU is visible,
so a regression in a check can never hand a host pointer to a kernel. The
binding makes its shape, dtype, layout, alignment and overlap checks first
and the device check last, so each refusal is reachable with CPU tensors.
"""

import pytest
import torch

from fluxdistributed_amd.ops.native import load_native

if torch.cuda.is_available():  # pragma: no cover
    pytest.skip("CPU-only: must never reach a launch", allow_module_level=True)

C = load_native()
if C is None:  # pragma: no cover
    pytest.skip("native extension not built", allow_module_level=True)

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def _f(n=64, dtype=F32):
    return torch.zeros(n, dtype=dtype)


def _flag():
    return torch.zeros(1, dtype=I32)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("with_flag", [False, True])
def test_valid_call_refused_only_by_device_check(dtype, with_flag):
    grads = [_f(64, dtype), _f(64, dtype)]
    with pytest.raises(RuntimeError, match="device tensors required"):
        if with_flag:
            C.grad_mean_multi(grads, _flag())
        else:
            C.grad_mean_multi(grads)


def _overlapping():
    buf = _f(128)
    return [buf[0:64], buf[32:96]]      # both 16 B aligned, 32 shared


def _same_buffer_twice():
    buf = _f(64)
    return [buf, buf]


REFUSALS = {
    "empty_list": (lambda: C.grad_mean_multi([]), "needs 1..16 buffers"),
    "seventeen": (lambda: C.grad_mean_multi([_f() for _ in range(17)]),
                  "needs 1..16 buffers"),
    "mixed_dtype": (lambda: C.grad_mean_multi([_f(64), _f(64, BF)]),
                    "every buffer must be contiguous"),
    "mixed_numel": (lambda: C.grad_mean_multi([_f(64), _f(128)]),
                    "every buffer must be contiguous"),
    "n_not_multiple_of_v_fp32": (
        lambda: C.grad_mean_multi([_f(66), _f(66)]), "padded to 4"),
    "n_not_multiple_of_v_bf16": (
        lambda: C.grad_mean_multi([_f(68, BF), _f(68, BF)]), "padded to 8"),
    "non_contiguous": (
        lambda: C.grad_mean_multi([_f(64), _f(128)[::2]]),
        "every buffer must be contiguous"),
    "two_dimensional": (
        lambda: C.grad_mean_multi([_f(64), _f(64).view(8, 8)]),
        "must be 1-D"),
    "int_dtype": (lambda: C.grad_mean_multi([_f(64, I32), _f(64, I32)]),
                  "expected f32 or bf16"),
    "misaligned_view": (
        lambda: C.grad_mean_multi([_f(64), _f(65)[1:]]), "16-byte aligned"),
    "overlapping_views": (lambda: C.grad_mean_multi(_overlapping()),
                          "overlap"),
    "same_buffer_twice": (lambda: C.grad_mean_multi(_same_buffer_twice()),
                          "overlap"),
    "flag_dtype": (
        lambda: C.grad_mean_multi([_f(), _f()], torch.zeros(1)),
        "flag must be contiguous"),
    "flag_size": (
        lambda: C.grad_mean_multi([_f(), _f()], torch.zeros(2, dtype=I32)),
        "flag must be contiguous"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refused_before_the_device_check(case):
    call, message = REFUSALS[case]
    with pytest.raises(RuntimeError, match=message) as info:
        call()
    assert "device tensors required" not in str(info.value)
