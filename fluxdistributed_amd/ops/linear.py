"""Dense (FC) layer on the native MFMA conv kernels — the last hipBLASLt
user in the ResNet step (round-1 profile `Cijk_*` rows; SURVEY.md §2.4
Dense row: the reference's Flux `Dense(512 => 1000)` FC).

MI355X-native design: an FC is a 1x1 conv over a [M, Cin, 1, 1]
channels_last image, so the battle-tested implicit-GEMM kernels do all
three GEMMs. conv_igemm requires output channels % 64 == 0 and the FC has
1000 classes, so out_features is padded to Kp = ceil(N/64)*64 in-house:

  fwd:   y[M][Kp]  = conv_fwd(x4d, wpad)           wpad rows >= N are zero
         y += bpad (bias_add kernel)               -> narrow view [M][N]
  dgrad: dx[M][Cin] = conv_dgrad(dypad, wt)        wt from the _WtArena
  wgrad: dwpad[Kp][Cin] = conv_wgrad(dypad, x4d);  G += first N rows
  bias:  db = colsum(dypad)[:N] direct into flat G

The padded weight/bias copies live in a per-device arena refreshed once
per optimizer step (the step epoch of ops/step_state.py; ops/arenas.py).
All padding/copy kernels are in-tree (csrc/elementwise.hip) — zero aten
kernels in the FC path.
"""

import os

import torch
import torch.nn.functional as F

from .arenas import fc_pad, wgrad_arena, wt_arena
from .gradflush import queue_or_flush
from .native import load_native, require_native
from .step_state import flat_grad_slice, notify_grad_written


def _as_nhwc_4d(t2d: torch.Tensor) -> torch.Tensor:
    """[M, C] contiguous -> [M, C, 1, 1] that IS channels_last."""
    M, C = t2d.shape
    return t2d.view(M, 1, 1, C).permute(0, 3, 1, 2)


class _FdaLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        C = require_native("fc_fwd")

        N, Cin = weight.shape
        ent = ctx.pad = fc_pad(weight, bias)
        Kp = ent["Kp"]
        xc = x.contiguous()
        y = C.conv_igemm_fwd(_as_nhwc_4d(xc), ent["wpad4"],
                             1, 1, 0, 0)          # [M, Kp, 1, 1]
        y2 = y.view(x.shape[0], Kp)
        if bias is not None:
            C.bias_add_rows_bf16(y2, ent["bpad"])
        ctx.save_for_backward(xc, weight)
        ctx.bias = bias
        ctx.Kp = Kp
        return y2[:, :N]

    @staticmethod
    def backward(ctx, gy):
        C = require_native("fc_bwd")

        x, weight = ctx.saved_tensors
        bias = ctx.bias
        Kp = ctx.Kp
        N, Cin = weight.shape
        M = x.shape[0]
        dyp = C.pad_rows_bf16(gy.contiguous(), Kp)     # [M, Kp], pad zero
        dyp4 = _as_nhwc_4d(dyp)
        dx = dw = db = None
        ent = ctx.pad
        if ctx.needs_input_grad[0]:
            wt = wt_arena(x.device).get(ent["wpad4"])  # [Cin, Kp]
            dx4 = C.conv_igemm_dgrad(dyp4, wt, Cin, 1, 1, 1, 1, 1, 1, 0, 0)
            dx = dx4.permute(0, 2, 3, 1).reshape(M, Cin)
        if ctx.needs_input_grad[1]:
            # step-scoped arena slice (pre-zeroed once per backward epoch)
            # instead of a fresh at::zeros per step
            ws = wgrad_arena(x.device).get(ent["wpad4"])
            C.conv_igemm_wgrad_into(dyp4, _as_nhwc_4d(x), ws, 1, 1, 1, 1, 0, 0)
            g_sl = flat_grad_slice(weight)
            if g_sl is not None:
                queue_or_flush(weight, g_sl, ws.reshape(-1)[: N * Cin])
            else:
                dw = ws.view(Kp, Cin)[:N].to(torch.bfloat16)
        if bias is not None and ctx.needs_input_grad[2]:
            gb_sl = flat_grad_slice(bias)
            if gb_sl is not None:
                C.colsum_accum_bf16(gb_sl, dyp)
                notify_grad_written(bias)
            else:
                db = dyp.float().sum(dim=0)[:N].to(torch.bfloat16)
        return dx, dw, db


def _fda_linear_supported(x, weight) -> bool:
    if os.environ.get("FLUXDIST_FC", "") == "lib":
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16 and x.dim() == 2):
        return False
    # in_features staged as conv reduction channels (%64); out_features
    # only needs %8 for the 16B-vector pad kernels (padded to %64 in-house)
    return (weight.shape[1] % 64 == 0 and weight.shape[0] % 8 == 0
            and load_native() is not None)


class FdaLinear(torch.nn.Linear):
    """nn.Linear dispatched to the native MFMA path for bf16 GPU tensors;
    parameter shapes/layout unchanged (checkpoint-compatible)."""

    def forward(self, x):
        if _fda_linear_supported(x, self.weight):
            return _FdaLinear.apply(x, self.weight, self.bias)
        return F.linear(x, self.weight, self.bias)
