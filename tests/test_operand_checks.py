"""The non-conv native entry points refuse host tensors and mis-sized operands
before any launch (the conv_igemm entry points: test_conv_operand_checks.py).

CPU-only by construction: the module is skipped wherever a GPU is visible,
so a regression in a check can never hand a host pointer to a kernel. Every
binding makes its shape, dtype and layout checks first and the device check
last, so each refusal is reachable with CPU tensors.
"""

import pytest
import torch

from fluxdistributed_amd.ops.native import load_native

if torch.cuda.is_available():  # pragma: no cover
    pytest.skip("CPU-only: must never reach a launch", allow_module_level=True)

C = load_native()
if C is None:  # pragma: no cover
    pytest.skip("native extension not built", allow_module_level=True)


def _cl(*shape, dtype=torch.bfloat16):
    t = torch.zeros(*shape, dtype=dtype)
    return t.contiguous(memory_format=torch.channels_last)


# --------------------------------------------------------------------------
# non-conv entry points: otherwise valid, smallest arguments on the CPU
# --------------------------------------------------------------------------

BF, F32, I64, I32 = torch.bfloat16, torch.float32, torch.int64, torch.int32


def _f(n, dtype=F32):
    return torch.zeros(n, dtype=dtype)


BX = _cl(1, 64, 2, 2)                   # BN activation, rows = 4
BP = _f(64)                             # any [C] fp32 BN operand
NORES = torch.empty(0, dtype=BF)
PX = _cl(1, 64, 4, 4)                   # pool input; k3 s2 p1 -> 2x2
PG = _cl(1, 64, 2, 2)                   # pooled gradient
PIDX = torch.zeros(1 * 2 * 2 * 64, dtype=torch.uint8)
X8 = _cl(1, 8, 4, 12)                   # stem input: 4 rows, 4 + 8 columns
WPAD = torch.zeros(64, 1, 64, dtype=BF)  # [K][R=1][64]
SDY = _cl(1, 64, 4, 4)                  # stem output gradient, P = Q = 4


def _bn_fwd(x=BX, w=BP, b=BP, rm=BP, rv=BP, res=NORES, part=None,
            training=True):
    return C.bn_act_fwd(x, w, b, rm, rv, training, 0.1, 1e-5, True, res, part)


def _bn_bwd(gout=BX, x=BX, w=BP, mean=BP, invstd=BP, out=BX, gw=None, gb=None,
            want_gres=False, bias=None):
    return C.bn_act_bwd(gout, x, w, mean, invstd, out, True, True, gw, gb,
                        want_gres, bias)


def _pool_fwd(x=PX, w=BP, b=BP, rm=BP, rv=BP, k=3, s=2, p=1, part=None):
    return C.bn_act_pool_fwd(x, w, b, rm, rv, True, 0.1, 1e-5, k, k, s, p,
                             part)


def _pool_bwd(gout=PG, x=PX, w=BP, b=BP, mean=BP, invstd=BP, idx=PIDX,
              gw=None, gb=None):
    return C.bn_act_pool_bwd(gout, x, w, b, mean, invstd, idx, 3, 3, 2, 1,
                             True, gw, gb)


def _sgd(P=None, G=None, M=None, V=None):
    P = _f(8) if P is None else P
    return C.sgd_step(P, _f(8) if G is None else G, P if M is None else M,
                      _f(8) if V is None else V, 0.1, 0.9, 0.0, False)


def _adam(P=None, G=None, M=None, V=None, S=None):
    P = _f(8) if P is None else P
    return C.adam_step(P, _f(8) if G is None else G, P if M is None else M,
                       _f(8) if V is None else V, _f(8) if S is None else S,
                       1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001)


DEVICE_CALLS = {
    "ce_fwd": lambda: C.ce_fwd(torch.zeros(2, 8), _f(2, I64)),
    "add_relu_fwd": lambda: C.add_relu_fwd(BX, BX),
    "add_relu_bwd": lambda: C.add_relu_bwd(BX, BX),
    "bn_act_fwd": _bn_fwd,
    "bn_act_fwd_eval": lambda: _bn_fwd(training=False),
    "bn_act_fwd_conv_part": lambda: _bn_fwd(part=torch.zeros(3, 2, 64)),
    "bn_act_bwd": _bn_bwd,
    "bn_act_bwd_direct": lambda: _bn_bwd(gw=_f(64), gb=_f(64), bias=BP),
    "bn_act_pool_fwd": _pool_fwd,
    "bn_act_pool_bwd": _pool_bwd,
    "maxpool_fwd": lambda: C.maxpool_fwd(PX, 3, 3, 2, 1),
    "maxpool_bwd": lambda: C.maxpool_bwd(PG, PIDX, 4, 4, 3, 3, 2, 1),
    "gap_fwd": lambda: C.gap_fwd(PX),
    "gap_bwd": lambda: C.gap_bwd(torch.zeros(1, 64, dtype=BF), 2, 2),
    "sgd_step": _sgd,
    "adam_step": _adam,
    "conv_stem_fwd": lambda: C.conv_stem_fwd(X8, WPAD, 1, 1, 1, 4, 4),
    "conv_stem_fwd_stats":
        lambda: C.conv_stem_fwd_stats(X8, WPAD, 1, 1, 1, 4, 4),
    "conv_stem_wgrad": lambda: C.conv_stem_wgrad(SDY, X8, 1, 1, 1),
    "pad_rows_bf16": lambda: C.pad_rows_bf16(torch.zeros(2, 8, dtype=BF), 16),
    "pad_rows_bf16_into": lambda: C.pad_rows_bf16_into(
        torch.zeros(2, 16, dtype=BF), torch.zeros(2, 8, dtype=BF)),
    "bias_add_rows_bf16": lambda: C.bias_add_rows_bf16(
        torch.zeros(2, 8, dtype=BF), _f(8, BF)),
    "colsum_accum_bf16": lambda: C.colsum_accum_bf16(
        _f(8, BF), torch.zeros(2, 8, dtype=BF)),
    "grad_accum_bf16": lambda: C.grad_accum_bf16(_f(8, BF), _f(8)),
    "grad_accum_batch": lambda: C.grad_accum_batch(
        _f(2, I64), _f(2, I64), _f(2, I64), 8),
    "wt_transpose_batch": lambda: C.wt_transpose_batch(
        _f(2, I64), _f(2, I64), _f(2, I32), _f(2, I32), _f(2, I32), 1),
}


@pytest.mark.parametrize("entry", sorted(DEVICE_CALLS))
def test_entry_point_refuses_cpu_tensors(entry):
    with pytest.raises(RuntimeError, match="device tensors required"):
        DEVICE_CALLS[entry]()


# One refusal per operand the bindings used to pass to a kernel unchecked;
# each is matched on its own message, which names the operand.
SHAPE_CALLS = {
    # direct-grad slices: both or neither, fp32, contiguous, exactly C
    "bn_bwd_gw_without_gb":
        (lambda: _bn_bwd(gw=_f(64)), "gw_out and gb_out must be given together"),
    "bn_bwd_gb_without_gw":
        (lambda: _bn_bwd(gb=_f(64)), "gw_out and gb_out must be given together"),
    "bn_bwd_gw_bf16":
        (lambda: _bn_bwd(gw=_f(64, BF), gb=_f(64)), "gw_out must be contiguous"),
    "bn_bwd_gb_short":
        (lambda: _bn_bwd(gw=_f(64), gb=_f(63)), "gb_out must be contiguous"),
    "bn_bwd_gw_strided":
        (lambda: _bn_bwd(gw=_f(128)[::2], gb=_f(64)),
         "gw_out must be contiguous"),
    "bn_pool_bwd_gw_without_gb":
        (lambda: _pool_bwd(gw=_f(64)),
         "gw_out and gb_out must be given together"),
    "bn_pool_bwd_gb_bf16":
        (lambda: _pool_bwd(gw=_f(64), gb=_f(64, BF)),
         "gb_out must be contiguous"),
    # bn_act_bwd: gout / out against x; saved statistics
    "bn_bwd_gout_dtype":
        (lambda: _bn_bwd(gout=_cl(1, 64, 2, 2, dtype=F32)), "gout must match x"),
    "bn_bwd_gout_shape":
        (lambda: _bn_bwd(gout=_cl(1, 64, 2, 1)), "gout must match x"),
    "bn_bwd_out_shape":
        (lambda: _bn_bwd(out=_cl(1, 64, 1, 2)), "out must match x"),
    "bn_bwd_out_dtype":
        (lambda: _bn_bwd(out=_cl(1, 64, 2, 2, dtype=F32)), "out must match x"),
    "bn_bwd_save_mean_short":
        (lambda: _bn_bwd(mean=_f(32)), "save_mean must be contiguous"),
    "bn_bwd_save_invstd_short":
        (lambda: _bn_bwd(invstd=_f(63)), "save_invstd must be contiguous"),
    # BN forward: parameter / running-stat lengths, residual
    "bn_fwd_bias_short":
        (lambda: _bn_fwd(b=_f(63)), "bias must be contiguous"),
    "bn_fwd_running_mean_short":
        (lambda: _bn_fwd(rm=_f(32)), "running_mean must be contiguous"),
    "bn_fwd_running_var_short":
        (lambda: _bn_fwd(rv=_f(1)), "running_var must be contiguous"),
    "bn_fwd_residual_dtype":
        (lambda: _bn_fwd(res=_cl(1, 64, 2, 2, dtype=F32)),
         "residual must match x"),
    "bn_fwd_residual_shape":
        (lambda: _bn_fwd(res=_cl(1, 64, 2, 1)), "residual must match x"),
    "bn_fwd_conv_part_channels":
        (lambda: _bn_fwd(part=torch.zeros(3, 2, 32)), "conv_part must be"),
    "bn_pool_fwd_bias_short":
        (lambda: _pool_fwd(b=_f(63)), "bias must be contiguous"),
    "bn_pool_fwd_running_var_short":
        (lambda: _pool_fwd(rv=_f(32)), "running_var must be contiguous"),
    # max-pool
    "maxpool_fwd_256_taps":
        (lambda: C.maxpool_fwd(_cl(1, 64, 16, 16), 16, 16, 1, 0),
         "argmax is one byte"),
    "maxpool_fwd_stride_0":
        (lambda: C.maxpool_fwd(PX, 3, 3, 0, 1), "stride >= 1"),
    "maxpool_bwd_idx_short":
        (lambda: C.maxpool_bwd(PG, PIDX[:-1], 4, 4, 3, 3, 2, 1),
         "argmax bytes do not match"),
    "maxpool_bwd_channels":
        (lambda: C.maxpool_bwd(_cl(1, 4, 2, 2), PIDX[:16], 4, 4, 3, 3, 2, 1),
         "C must be divisible by 8"),
    "maxpool_bwd_geometry":
        (lambda: C.maxpool_bwd(PG, PIDX, 8, 8, 3, 3, 2, 1),
         "not the pooled shape"),
    # global average pool: 16 B accesses
    "gap_fwd_c6":
        (lambda: C.gap_fwd(_cl(1, 6, 2, 2, dtype=F32)),
         "C must be divisible by 4"),
    "gap_bwd_c12":
        (lambda: C.gap_bwd(torch.zeros(1, 12, dtype=BF), 2, 2),
         "C must be divisible by 8"),
    # flat optimizers
    "sgd_g_short": (lambda: _sgd(G=_f(4)), "G must be contiguous"),
    "sgd_g_dtype": (lambda: _sgd(G=_f(8, BF)), "G must be contiguous"),
    "sgd_v_short": (lambda: _sgd(V=_f(4)), "state must be contiguous"),
    "sgd_m_short":
        (lambda: _sgd(P=_f(8, BF), G=_f(8, BF), M=_f(4)),
         "M must be contiguous"),
    "adam_v_short": (lambda: _adam(V=_f(7)), "state must be contiguous"),
    "adam_s_short": (lambda: _adam(S=_f(4)), "state must be contiguous"),
    "adam_g_dtype": (lambda: _adam(G=_f(8, BF)), "G must be contiguous"),
    "adam_p_strided":
        (lambda: _adam(P=_f(16)[::2]), "P must be contiguous"),
    # stem conv
    "stem_fwd_stats_channels":
        (lambda: C.conv_stem_fwd_stats(_cl(1, 4, 4, 12), WPAD, 1, 1, 1, 4, 4),
         r"x8 must be \[N,8,Hp,Wp\]"),
    "stem_fwd_stats_wpad":
        (lambda: C.conv_stem_fwd_stats(
            X8, torch.zeros(64, 1, 32, dtype=BF), 1, 1, 1, 4, 4),
         "wpad must be contiguous bf16"),
    "stem_fwd_stats_k32":
        (lambda: C.conv_stem_fwd_stats(
            X8, torch.zeros(32, 1, 64, dtype=BF), 1, 1, 1, 4, 4),
         "K must be a multiple of 64"),
    "stem_fwd_stats_output_too_wide":
        (lambda: C.conv_stem_fwd_stats(X8, WPAD, 1, 1, 1, 4, 6),
         "reads outside the padded"),
    "stem_wgrad_k32":
        (lambda: C.conv_stem_wgrad(_cl(1, 32, 4, 4), X8, 1, 1, 1),
         "K must be a multiple of 64"),
    "stem_wgrad_channels":
        (lambda: C.conv_stem_wgrad(SDY, _cl(1, 16, 4, 12), 1, 1, 1),
         r"x8 must be \[N,8,Hp,Wp\]"),
    "stem_wgrad_dy_too_tall":
        (lambda: C.conv_stem_wgrad(_cl(1, 64, 5, 4), X8, 1, 1, 1),
         "reads outside the padded"),
    # FC-head padding
    "pad_rows_into_dtype":
        (lambda: C.pad_rows_bf16_into(torch.zeros(2, 16), torch.zeros(2, 8)),
         "bf16 only"),
    "pad_rows_into_src_wider":
        (lambda: C.pad_rows_bf16_into(torch.zeros(2, 8, dtype=BF),
                                      torch.zeros(2, 16, dtype=BF)),
         "row lengths must be multiples of 8"),
    "pad_rows_into_not_8":
        (lambda: C.pad_rows_bf16_into(torch.zeros(2, 12, dtype=BF),
                                      torch.zeros(2, 8, dtype=BF)),
         "row lengths must be multiples of 8"),
    # device pointer arrays
    "wt_transpose_ks_short":
        (lambda: C.wt_transpose_batch(_f(2, I64), _f(2, I64), _f(1, I32),
                                      _f(2, I32), _f(2, I32), 1),
         "Ks must be contiguous"),
    "wt_transpose_dst_dtype":
        (lambda: C.wt_transpose_batch(_f(2, I64), _f(2, I32), _f(2, I32),
                                      _f(2, I32), _f(2, I32), 1),
         "dst_ptrs must be contiguous"),
    "grad_accum_batch_ns_short":
        (lambda: C.grad_accum_batch(_f(2, I64), _f(2, I64), _f(1, I64), 8),
         "ns must be contiguous"),
    "grad_accum_batch_ws_dtype":
        (lambda: C.grad_accum_batch(_f(2, I64), _f(2, I32), _f(2, I64), 8),
         "ws_ptrs must be contiguous"),
    # elementwise, loss
    "add_relu_bwd_dtype":
        (lambda: C.add_relu_bwd(BX, _cl(1, 64, 2, 2, dtype=F32)),
         "operands must agree in shape and dtype"),
    "ce_fwd_target_short":
        (lambda: C.ce_fwd(torch.zeros(2, 8), _f(1, I64)),
         "one class index per row"),
}


@pytest.mark.parametrize("case", sorted(SHAPE_CALLS))
def test_entry_point_refuses_bad_operand(case):
    call, message = SHAPE_CALLS[case]
    with pytest.raises(RuntimeError, match=message):
        call()
