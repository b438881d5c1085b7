"""Conv2d dispatch: hand-written MFMA implicit-GEMM kernels with library
fallback.

The reference gets conv from cuDNN via NNlibCUDA; the
MI355X-native path is fluxdistributed_amd/csrc/conv_igemm.hip —
v_mfma_f32_16x16x32_bf16 tiles, LDS-staged via global_load_lds. Supported
there: NHWC bf16, dilation 1, groups 1, C and K multiples of 64 (all
ResNet body convs) — fwd, dgrad AND wgrad. Small-C stems (C<=5, e.g. the
ImageNet 7x7 and CIFAR 3x3 stems) run on the dedicated CONV_STEM kernels
where K is a multiple of 64; only genuinely unsupported shapes (dilated, odd
channel counts, grouped convs outside the set below) fall back to the
library path.

Narrow stems (3x3, padding 1, stride 1 or 2, Cin <= 3, K a multiple of 8 in
[8, 64] that the CONV_STEM kernels do not take: the MobileNetV1 stem, K = 8
to 32) have csrc/conv_stem_narrow.hip: bf16, x read as stored (no padded
copy, no buffer pool), the whole reduction of 9*Cin values in one MFMA K-step,
the weight [K][3][3][Cin] read as stored and held in registers, wgrad through
per-chunk slabs and the ordered fold. Forward and wgrad only: like the
CONV_STEM kernels it has no dgrad, and an input that requires grad goes to
the library. Plain autograd. The path is opt-in
(FLUXDIST_CONV_STEM_NARROW=1): against the library its forward is faster on
all five measured MobileNetV1 stems (44 vs 58 us for 3 -> 32 at 224x224) but
its wgrad is slower on the four 224x224 ones (78 vs 60 us) and the step does
not gain (profiles/conv_stem_narrow.md), so by the rule that defaults are
measured winners the default is 0.

Grouped 3x3 convs (the ResNeXt bottlenecks) have kernels of their own,
csrc/conv_grouped.hip: bf16, padding 1, stride 1 or 2, C/g == K/g in
{4, 8, 16, 32}, C a multiple of 64; forward, dgrad and wgrad read the weight
as stored and keep it in registers. Plain autograd like the fp32 path. On by
default (FLUXDIST_CONV_GROUPED=1): against the library's grouped conv it is
faster on every ResNeXt-50 shape and leg and the ResNeXt-50 step is 1.58x
faster (profiles/conv_grouped.md).

Depthwise 3x3 convs (groups == C == K, the MobileNet body) have kernels of
their own too, csrc/conv_dw.hip: bf16, padding 1, stride 1 or 2, any C that
is a multiple of 8. A lane owns 8 channels and keeps their taps in registers;
forward and dgrad slide a register window down a strip of columns, wgrad
reduces per channel through per-chunk slabs and the ordered fold. Plain
autograd. On by default (FLUXDIST_CONV_DW=1): against the library's depthwise
conv it is faster on every MobileNetV1 shape and leg and the MobileNetV1 step
is 2.21x faster (profiles/conv_dw.md).

Narrow pointwise convs (1x1, stride 1, padding 0, groups 1, C and K multiples
of 8 in [8, 256]: the pointwise halves of depthwise-separable blocks) have
csrc/conv_pw.hip: bf16, the weight [K][C] read as stored and held in
registers by all of forward and dgrad, the activation read once, wgrad through
per-chunk slabs and the ordered fold. Plain autograd. It sits behind
conv_igemm, so shapes with both channel counts multiples of 64 stay there. The
path is opt-in (FLUXDIST_CONV_PW=1): against the library it is faster in 13 of
15 measured shape-legs of MobileNetV1 but slower in the forward (43 vs 36 us)
and the wgrad (48 vs 47 us) of 32 -> 64 at 112x112, and the MobileNetV1 step
does not move beyond the spread (profiles/conv_pw.md), so by the rule that
defaults are measured winners the default is 0.

fp32 operands have a native path of their own, csrc/conv_f32.hip on the
fp32 MFMA (v_mfma_f32_16x16x4_f32): the same constraints (NHWC, dilation 1,
groups 1, C and K multiples of 64), forward, dgrad from the untransposed
weight and wgrad through per-chunk slabs and an ordered fold. It is plain
autograd: no conv->BN stats, no junction fusion, no arenas, no direct write
into flat G. The fp32 stem (C=3) and the fp32 FC head stay on the library.
The path is opt-in (FLUXDIST_CONV_F32=1): measured against the library's
fp32 conv it is slower on every ResNet-34 shape and leg (profiles/conv_f32.md),
so by the rule that defaults are measured winners the default is 0.

Env:
  FLUXDIST_CONV=miopen   force the library path everywhere (A/B testing)
  FLUXDIST_CONV=fda      force the native path (errors on shapes no native
                         path supports)
  FLUXDIST_CONV_F32=1|0  fp32 body convs on conv_f32.hip (1) or the library
                         (0, the default). Read at call time. FLUXDIST_CONV=fda
                         implies 1.
  FLUXDIST_CONV_GROUPED=1|0  grouped 3x3 convs on conv_grouped.hip (1, the
                         default) or the library (0). Read at call time.
                         FLUXDIST_CONV=miopen overrides it, FLUXDIST_CONV=fda
                         implies 1.
  FLUXDIST_CONV_DW=1|0   depthwise 3x3 convs on conv_dw.hip (1, the default)
                         or the library (0). Read at call time.
                         FLUXDIST_CONV=miopen overrides it, FLUXDIST_CONV=fda
                         implies 1.
  FLUXDIST_CONV_PW=1|0   narrow pointwise convs on conv_pw.hip (1) or the
                         library (0, the default). Read at call time.
                         FLUXDIST_CONV=miopen overrides it, FLUXDIST_CONV=fda
                         implies 1.
  FLUXDIST_CONV_STEM_NARROW=1|0  narrow stem convs on conv_stem_narrow.hip
                         (1) or the library (0, the default). Read at call
                         time. FLUXDIST_CONV=miopen overrides it,
                         FLUXDIST_CONV=fda implies it.
  FLUXDIST_WGRAD_SLAB=0  weight-grads into flat G: atomic workspace + queued
                         flush for every shape (default 1: slabs + ordered
                         fold where conv_igemm_wgrad_mode says "slab")
"""

import os
from typing import Tuple

import torch
import torch.nn.functional as F

from .arenas import stem_pool_get, stem_pool_put, wgrad_arena, wt_arena
from .gradflush import queue_or_flush
from .native import load_native, require_native
from .step_state import (clear_conv_stats, flat_grad_slice,
                         notify_grad_written, stash_conv_stats,
                         take_junction_gres)
# names that callers outside ops/ import from here
from .step_state import bump_step_epoch as bump_conv_wt_marker  # noqa: F401
from .step_state import junction_stash_empty  # noqa: F401


def _pair(v) -> Tuple[int, int]:
    return (v, v) if isinstance(v, int) else tuple(v)


def _native_supported(x: torch.Tensor, w: torch.Tensor, stride, padding,
                      dilation, groups) -> bool:
    if os.environ.get("FLUXDIST_CONV", "") == "miopen":
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16):
        return False
    if groups != 1 or _pair(dilation) != (1, 1):
        return False
    C, K = x.shape[1], w.shape[0]
    if C % 64 != 0 or K % 64 != 0:
        return False
    return load_native() is not None


_CONV_F32_DEFAULT = "0"


def _native_f32_supported(x: torch.Tensor, w: torch.Tensor, stride, padding,
                          dilation, groups) -> bool:
    """fp32 operands the conv_f32 kernels serve, FLUXDIST_CONV_F32 aside."""
    if os.environ.get("FLUXDIST_CONV", "") == "miopen":
        return False
    if not (x.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32):
        return False
    if groups != 1 or _pair(dilation) != (1, 1):
        return False
    C, K = x.shape[1], w.shape[0]
    if C % 64 != 0 or K % 64 != 0:
        return False
    return load_native() is not None


_CONV_GROUPED_DEFAULT = "1"


def _native_grouped_supported(x: torch.Tensor, w: torch.Tensor, stride,
                              padding, dilation, groups) -> bool:
    """Grouped 3x3 convs the conv_grouped kernels serve, FLUXDIST_CONV_GROUPED
    aside: bf16, padding 1, stride 1 or 2, C/g == K/g in {4, 8, 16, 32},
    C a multiple of 64."""
    if os.environ.get("FLUXDIST_CONV", "") == "miopen":
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16):
        return False
    if groups == 1 or _pair(dilation) != (1, 1) or _pair(padding) != (1, 1):
        return False
    if _pair(stride) not in ((1, 1), (2, 2)) or tuple(w.shape[2:]) != (3, 3):
        return False
    C, K = x.shape[1], w.shape[0]
    if C != K or C % 64 != 0 or C % groups != 0:
        return False
    if C // groups not in (4, 8, 16, 32):
        return False
    return load_native() is not None


_CONV_DW_DEFAULT = "1"


def _native_dw_supported(x: torch.Tensor, w: torch.Tensor, stride, padding,
                         dilation, groups) -> bool:
    """Depthwise 3x3 convs the conv_dw kernels serve, FLUXDIST_CONV_DW aside:
    bf16, padding 1, stride 1 or 2, groups == C == K, C a multiple of 8."""
    if os.environ.get("FLUXDIST_CONV", "") == "miopen":
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16):
        return False
    if _pair(dilation) != (1, 1) or _pair(padding) != (1, 1):
        return False
    if _pair(stride) not in ((1, 1), (2, 2)):
        return False
    C = x.shape[1]
    if groups != C or tuple(w.shape) != (C, 1, 3, 3) or C % 8 != 0:
        return False
    return load_native() is not None


_CONV_PW_DEFAULT = "0"


def _native_pw_supported(x: torch.Tensor, w: torch.Tensor, stride, padding,
                         dilation, groups) -> bool:
    """Pointwise convs the conv_pw kernels serve, FLUXDIST_CONV_PW aside:
    bf16, 1x1, stride 1, padding 0, groups 1, C and K multiples of 8 in
    [8, 256]."""
    if os.environ.get("FLUXDIST_CONV", "") == "miopen":
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16):
        return False
    if groups != 1 or _pair(dilation) != (1, 1) or _pair(padding) != (0, 0):
        return False
    if _pair(stride) != (1, 1) or tuple(w.shape[2:]) != (1, 1):
        return False
    C, K = x.shape[1], w.shape[0]
    if C % 8 != 0 or K % 8 != 0 or not (8 <= C <= 256 and 8 <= K <= 256):
        return False
    return load_native() is not None


def _want_conv_stats() -> bool:
    """Decided in the DISPATCHER (fda_conv2d), where grad mode is visible —
    inside Function.forward torch.is_grad_enabled() is always False, which
    silently killed the conv->BN stats fusion (r2 profile: all 36 BNs ran
    their own stats pass despite the handshake)."""
    return (torch.is_grad_enabled()
            and os.environ.get("FLUXDIST_BN_FUSE", "1") != "0")


class _FdaConv2d(torch.autograd.Function):
    """Forward, input-grad and weight-grad on the native implicit-GEMM
    kernels. The weight-grad lands in an fp32 workspace and, when the
    weight lives in a fused optimizer's flat buffer, is flushed straight
    into its G slice; shapes for which conv_igemm_wgrad_mode says "slab"
    skip the workspace and go through per-chunk slabs and an ordered fold
    (conv_igemm_wgrad_flush; FLUXDIST_WGRAD_SLAB=0 keeps them on the atomic
    workspace path). FLUXDIST_WGRAD=miopen routes the weight-grad alone to
    the library (aten convolution_backward with a weight-only mask)."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding, want_stats):
        C = require_native("conv_igemm_fwd")
        clear_conv_stats()
        xc = x.contiguous(memory_format=torch.channels_last)
        wc = weight.contiguous(memory_format=torch.channels_last)
        sy, sx = stride
        py, px = padding
        if want_stats:
            y, part = C.conv_igemm_fwd_stats(xc, wc, sy, sx, py, px)
            stash_conv_stats(y, part)
        else:
            y = C.conv_igemm_fwd(xc, wc, sy, sx, py, px)
        ctx.save_for_backward(xc, wc)
        ctx.conf = (stride, padding, weight is wc)
        if weight is wc:  # already channels_last: cacheable by identity
            wt_arena(wc.device).register(wc)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, padding, cacheable = ctx.conf
        sy, sx = stride
        py, px = padding
        gy = gy.contiguous(memory_format=torch.channels_last)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            C = require_native("conv_igemm_dgrad")
            K, Cin, R, S = w.shape
            if cacheable:
                wt = wt_arena(w.device).get(w)
            else:
                # wt[(r*S+s)*C + c][k]: k-contiguous rows for the B tile
                wt = w.permute(2, 3, 1, 0).reshape(R * S * Cin, K).contiguous()
            # deferred residual-junction grad for this input, if the block
            # routed one here: fused += in the dgrad epilogue
            acc = take_junction_gres(x)
            dx = C.conv_igemm_dgrad(gy, wt, Cin, x.shape[2], x.shape[3],
                                    R, S, sy, sx, py, px, acc)
        if ctx.needs_input_grad[1]:
            K, Cin, R, S = w.shape
            if os.environ.get("FLUXDIST_WGRAD", "") != "miopen":
                C = require_native("conv_igemm_wgrad")
                g_sl = flat_grad_slice(w) if cacheable else None
                if (g_sl is not None
                        and os.environ.get("FLUXDIST_WGRAD_SLAB", "1") != "0"
                        and C.conv_igemm_wgrad_mode(
                            gy.shape[0] * gy.shape[2] * gy.shape[3],
                            Cin, K, R, S) == "slab"):
                    # per-chunk fp32 slabs + ordered fold straight into the
                    # G slice: no arena slot, no zero fill, no queued flush
                    C.conv_igemm_wgrad_flush(gy, x, g_sl, R, S, sy, sx,
                                             py, px)
                    notify_grad_written(w)
                    return dx, None, None, None, None
                if cacheable:
                    ws = wgrad_arena(w.device).get(w)
                    C.conv_igemm_wgrad_into(gy, x, ws, R, S, sy, sx, py, px)
                else:
                    ws = C.conv_igemm_wgrad(gy, x, R, S, sy, sx, py, px)
                if g_sl is not None:
                    # direct grad: G slice memory order == ws order
                    # ([K][R][S][C]); one fused cast+add, no AccumulateGrad.
                    # Queued + batched at backward end unless a DDP
                    # bucketer needs it immediately (ops/gradflush.py).
                    queue_or_flush(w, g_sl, ws.reshape(-1))
                    dw = None
                else:
                    # ws [K][R*S*C] fp32 is exactly the channels_last weight
                    # memory order [K][R][S][C]: one flat cast, no-copy view
                    dw = (ws.to(torch.bfloat16).view(K, R, S, Cin)
                          .permute(0, 3, 1, 2))
            else:
                dw = torch.ops.aten.convolution_backward(
                    gy, x, w, None, list(stride), list(padding), [1, 1],
                    False, [0, 0], 1, [False, True, False])[1]
        return dx, dw, None, None, None


class _FdaConv2dF32(torch.autograd.Function):
    """fp32 forward, input-grad and weight-grad on the conv_f32 kernels. The
    weight is read as stored by all three ([K][R][S][C], channels_last), and
    the weight-grad comes back in that memory order, so dw is a view;
    autograd accumulates it as on the library path."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding):
        C = require_native("conv_f32_fwd")
        clear_conv_stats()
        xc = x.contiguous(memory_format=torch.channels_last)
        wc = weight.contiguous(memory_format=torch.channels_last)
        y = C.conv_f32_fwd(xc, wc, *stride, *padding)
        ctx.save_for_backward(xc, wc)
        ctx.conf = (stride, padding)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, padding = ctx.conf
        C = require_native("conv_f32_dgrad")
        gy = gy.contiguous(memory_format=torch.channels_last)
        K, Cin, R, S = w.shape
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = C.conv_f32_dgrad(gy, w, x.shape[2], x.shape[3], *stride,
                                  *padding)
        if ctx.needs_input_grad[1]:
            ws = C.conv_f32_wgrad(gy, x, R, S, *stride, *padding)
            dw = ws.view(K, R, S, Cin).permute(0, 3, 1, 2)
        return dx, dw, None, None


class _FdaConv2dGrouped(torch.autograd.Function):
    """Grouped 3x3 forward, input-grad and weight-grad on the conv_grouped
    kernels. All three read the weight as stored ([K][3][3][cpg],
    channels_last); the weight-grad comes back fp32 in that memory order and
    is cast once. Plain autograd: no conv->BN stats, no arenas, no direct
    write into flat G."""

    @staticmethod
    def forward(ctx, x, weight, stride, groups):
        C = require_native("conv_grouped_fwd")
        clear_conv_stats()
        xc = x.contiguous(memory_format=torch.channels_last)
        wc = weight.contiguous(memory_format=torch.channels_last)
        y = C.conv_grouped_fwd(xc, wc, *stride, 1, 1, groups)
        ctx.save_for_backward(xc, wc)
        ctx.conf = (stride, groups)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, groups = ctx.conf
        C = require_native("conv_grouped_dgrad")
        gy = gy.contiguous(memory_format=torch.channels_last)
        K, cpg = w.shape[0], w.shape[1]
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = C.conv_grouped_dgrad(gy, w, x.shape[2], x.shape[3], *stride,
                                      1, 1, groups)
        if ctx.needs_input_grad[1]:
            ws = C.conv_grouped_wgrad(gy, x, *stride, 1, 1, groups)
            dw = (ws.to(torch.bfloat16).view(K, 3, 3, cpg)
                  .permute(0, 3, 1, 2))
        return dx, dw, None, None


class _FdaConv2dDepthwise(torch.autograd.Function):
    """Depthwise 3x3 forward, input-grad and weight-grad on the conv_dw
    kernels. All three read the weight as stored ([C,1,3,3]: [C][9] in
    memory, contiguous or channels_last); the weight-grad comes back fp32 in
    that memory order and is cast once. Plain autograd: no conv->BN stats,
    no arenas, no direct write into flat G."""

    @staticmethod
    def forward(ctx, x, weight, stride):
        C = require_native("conv_dw_fwd")
        clear_conv_stats()
        xc = x.contiguous(memory_format=torch.channels_last)
        wc = weight.contiguous(memory_format=torch.channels_last)
        y = C.conv_dw_fwd(xc, wc, *stride)
        ctx.save_for_backward(xc, wc)
        ctx.stride = stride
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride = ctx.stride
        C = require_native("conv_dw_dgrad")
        gy = gy.contiguous(memory_format=torch.channels_last)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = C.conv_dw_dgrad(gy, w, x.shape[2], x.shape[3], *stride)
        if ctx.needs_input_grad[1]:
            ws = C.conv_dw_wgrad(gy, x, *stride)
            dw = ws.to(torch.bfloat16).view(w.shape[0], 1, 3, 3)
        return dx, dw, None


class _FdaConv2dPointwise(torch.autograd.Function):
    """Narrow 1x1 forward, input-grad and weight-grad on the conv_pw kernels.
    All three read the weight as stored ([K,C,1,1]: [K][C] in memory,
    contiguous or channels_last); the weight-grad comes back fp32 in that
    memory order and is cast once. Plain autograd: no conv->BN stats, no
    arenas, no direct write into flat G."""

    @staticmethod
    def forward(ctx, x, weight):
        C = require_native("conv_pw_fwd")
        clear_conv_stats()
        xc = x.contiguous(memory_format=torch.channels_last)
        wc = weight.contiguous(memory_format=torch.channels_last)
        y = C.conv_pw_fwd(xc, wc)
        ctx.save_for_backward(xc, wc)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        C = require_native("conv_pw_dgrad")
        gy = gy.contiguous(memory_format=torch.channels_last)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = C.conv_pw_dgrad(gy, w)
        if ctx.needs_input_grad[1]:
            ws = C.conv_pw_wgrad(gy, x)
            dw = ws.to(torch.bfloat16).view(w.shape[0], w.shape[1], 1, 1)
        return dx, dw


def stem_buffer_key(x, weight, padding):
    """What a padded stem input buffer is reused by: its shape and device."""
    N, _, H, W = x.shape
    return (N, weight.shape[1], H, W, *padding, x.device)


def pack_stem_operands(x, weight, stride, padding, x8=None):
    """Operands of the CONV_STEM kernels: (x8, wpad, P, Q).

    x8 [N,8,H+2py,W+2px+8] is x channel-padded to 8 and spatially pre-padded
    by (py, px), with 8 columns of right-edge slack so the 8-pixel (s=0..7)
    granule row never leaves the image. Pass a buffer of a previous call
    with the same `stem_buffer_key` to reuse it: its zero border survives,
    so only the interior is rewritten. wpad [K][R][64] is the weight as
    [K][R][s<8][c<8], zero where s >= S or c >= Cin."""
    K, Cin, R, S = weight.shape
    sy, sx = stride
    py, px = padding
    N, _, H, W = x.shape
    if x8 is None:
        x8 = torch.empty(N, 8, H + 2 * py, W + 2 * px + 8, dtype=x.dtype,
                         device=x.device,
                         memory_format=torch.channels_last).zero_()
    x8[:, :Cin, py : py + H, px : px + W] = x
    wpad = torch.zeros(K, R, 64, dtype=weight.dtype, device=weight.device)
    wpad.view(K, R, 8, 8)[:, :, :S, :Cin] = (
        weight.contiguous(memory_format=torch.channels_last)
        .permute(0, 2, 3, 1))  # [K][R][S][C]
    return (x8, wpad, (H + 2 * py - R) // sy + 1, (W + 2 * px - S) // sx + 1)


class _FdaStemConv2d(torch.autograd.Function):
    """Small-C stem conv (C<=5, S<=7): channel-pad to 8 + spatial pre-pad,
    then the CONV_STEM kernel (one K-step per filter row r — 8 pixels x 8
    channels as 64 virtual reduction channels). No dgrad (the stem input is
    data); wgrad via conv_stem_wgrad."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding, want_stats):
        C = require_native("conv_stem_fwd")
        clear_conv_stats()
        K, Cin, R, S = weight.shape
        sy, sx = stride
        xc = x.contiguous(memory_format=torch.channels_last)
        # Padded buffers come from a per-shape free-list pool: each
        # checkout only copies the interior, but the buffer is exclusively
        # owned by THIS graph until backward returns it (no aliasing across
        # forwards — round-1 ADVICE #1).
        key = stem_buffer_key(x, weight, padding)
        x8, wpad, P, Q = pack_stem_operands(xc, weight, stride, padding,
                                            stem_pool_get(key))
        if want_stats:
            y, part = C.conv_stem_fwd_stats(x8, wpad, R, sy, sx, P, Q)
            stash_conv_stats(y, part)
        else:
            y = C.conv_stem_fwd(x8, wpad, R, sy, sx, P, Q)
        # NOTE: torch.is_grad_enabled() is ALWAYS False inside
        # Function.forward (autograd disables grad around it), so the keep
        # decision uses requires_grad only. Under no_grad the ctx (and the
        # buffer) are simply GC'd — a pool miss, not a leak.
        if x.requires_grad or weight.requires_grad:
            # plain attribute, not save_for_backward: the pool rewrites the
            # interior on reuse, so the version-counter check would reject
            # the standard fwd->bwd->fwd loop. Ownership (not versioning)
            # is the correctness mechanism here.
            ctx.x8 = x8
            ctx.pool_key = key
        else:
            # pure inference (frozen weights): no backward can reference
            # this buffer; return it now. Stream-ordered reuse on the same
            # stream is safe.
            ctx.x8 = None
            stem_pool_put(key, x8)
        ctx.conf = (K, Cin, R, S, sy, sx)
        return y

    @staticmethod
    def backward(ctx, gy):
        if ctx.needs_input_grad[0]:
            raise RuntimeError(
                "conv_stem has no input-grad path (stem inputs are data); "
                "fda_conv2d should have routed this conv to the library — "
                "x.requires_grad was set after dispatch?")
        x8 = ctx.x8
        K, Cin, R, S, sy, sx = ctx.conf
        dw = None
        if ctx.needs_input_grad[1]:
            C = require_native("conv_stem_wgrad")
            gyc = gy.contiguous(memory_format=torch.channels_last)
            ws = C.conv_stem_wgrad(gyc, x8, R, sy, sx)
            # ws [K][R*64] -> [K][R][s][c] -> weight grad [K,C,R,S]
            dw = (ws.view(K, R, 8, 8)[:, :, :S, :Cin]
                  .to(torch.bfloat16).permute(0, 3, 1, 2))
        ctx.x8 = None
        stem_pool_put(ctx.pool_key, x8)
        return None, dw, None, None, None


def _stem_supported(x, weight, stride, padding, dilation, groups) -> bool:
    if os.environ.get("FLUXDIST_CONV", "") == "miopen":
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16):
        return False
    if groups != 1 or _pair(dilation) != (1, 1):
        return False
    if x.requires_grad and torch.is_grad_enabled():
        # the stem kernel has no dgrad (stem inputs are data); route
        # input-saliency / adversarial passes to the library
        return False
    K, Cin, R, S = weight.shape
    return Cin <= 5 and S <= 7 and K % 64 == 0 and load_native() is not None


_CONV_STEM_NARROW_DEFAULT = "0"


def _native_stem_narrow_supported(x: torch.Tensor, w: torch.Tensor, stride,
                                  padding, dilation, groups) -> bool:
    """Stem convs the conv_stem_narrow kernels serve, FLUXDIST_CONV_STEM_NARROW
    aside: bf16, 3x3, padding 1, stride 1 or 2, groups 1, Cin <= 3, K a
    multiple of 8 in [8, 64], and an input that needs no gradient (there is
    no dgrad, as in the CONV_STEM kernels)."""
    if os.environ.get("FLUXDIST_CONV", "") == "miopen":
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16):
        return False
    if groups != 1 or _pair(dilation) != (1, 1) or _pair(padding) != (1, 1):
        return False
    if _pair(stride) not in ((1, 1), (2, 2)) or tuple(w.shape[2:]) != (3, 3):
        return False
    if x.requires_grad and torch.is_grad_enabled():
        return False
    K, Cin = w.shape[0], w.shape[1]
    if Cin > 3 or K % 8 != 0 or not 8 <= K <= 64:
        return False
    return load_native() is not None


class _FdaStemConv2dNarrow(torch.autograd.Function):
    """Narrow stem forward and weight-grad on the conv_stem_narrow kernels.
    Both read x as stored (no padded copy, no pool: x itself is saved, so a
    second backward works) and the weight as stored ([K][3][3][Cin],
    channels_last); the weight-grad comes back fp32 in that memory order and
    is cast once. No dgrad (the stem input is data). Plain autograd: no
    conv->BN stats, no arenas, no direct write into flat G."""

    @staticmethod
    def forward(ctx, x, weight, stride):
        C = require_native("conv_stem_narrow_fwd")
        clear_conv_stats()
        xc = x.contiguous(memory_format=torch.channels_last)
        wc = weight.contiguous(memory_format=torch.channels_last)
        y = C.conv_stem_narrow_fwd(xc, wc, stride[0])
        ctx.save_for_backward(xc)
        ctx.conf = (stride[0], tuple(weight.shape))
        return y

    @staticmethod
    def backward(ctx, gy):
        if ctx.needs_input_grad[0]:
            raise RuntimeError(
                "conv_stem_narrow has no input-grad path (stem inputs are "
                "data); fda_conv2d should have routed this conv to the "
                "library — x.requires_grad was set after dispatch?")
        (x,) = ctx.saved_tensors
        stride, (K, Cin, _, _) = ctx.conf
        dw = None
        if ctx.needs_input_grad[1]:
            C = require_native("conv_stem_narrow_wgrad")
            gyc = gy.contiguous(memory_format=torch.channels_last)
            ws = C.conv_stem_narrow_wgrad(gyc, x, stride)
            dw = (ws.to(torch.bfloat16).view(K, 3, 3, Cin)
                  .permute(0, 3, 1, 2))
        return None, dw, None


def fda_conv2d(x: torch.Tensor, weight: torch.Tensor, stride=(1, 1),
               padding=(0, 0), dilation=(1, 1), groups: int = 1) -> torch.Tensor:
    """conv2d with per-shape dispatch to the native MFMA kernel."""
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    if _native_supported(x, weight, stride, padding, dilation, groups):
        return _FdaConv2d.apply(x, weight, stride, padding, _want_conv_stats())
    if _stem_supported(x, weight, stride, padding, dilation, groups):
        return _FdaStemConv2d.apply(x, weight, stride, padding,
                                    _want_conv_stats())
    if (_native_stem_narrow_supported(x, weight, stride, padding, dilation,
                                      groups)
            and (os.environ.get("FLUXDIST_CONV_STEM_NARROW",
                                _CONV_STEM_NARROW_DEFAULT) != "0"
                 or os.environ.get("FLUXDIST_CONV", "") == "fda")):
        return _FdaStemConv2dNarrow.apply(x, weight, stride)
    if (_native_f32_supported(x, weight, stride, padding, dilation, groups)
            and (os.environ.get("FLUXDIST_CONV_F32", _CONV_F32_DEFAULT) != "0"
                 or os.environ.get("FLUXDIST_CONV", "") == "fda")):
        return _FdaConv2dF32.apply(x, weight, stride, padding)
    if (_native_grouped_supported(x, weight, stride, padding, dilation, groups)
            and (os.environ.get("FLUXDIST_CONV_GROUPED",
                                _CONV_GROUPED_DEFAULT) != "0"
                 or os.environ.get("FLUXDIST_CONV", "") == "fda")):
        return _FdaConv2dGrouped.apply(x, weight, stride, groups)
    if (_native_dw_supported(x, weight, stride, padding, dilation, groups)
            and (os.environ.get("FLUXDIST_CONV_DW", _CONV_DW_DEFAULT) != "0"
                 or os.environ.get("FLUXDIST_CONV", "") == "fda")):
        return _FdaConv2dDepthwise.apply(x, weight, stride)
    if (_native_pw_supported(x, weight, stride, padding, dilation, groups)
            and (os.environ.get("FLUXDIST_CONV_PW", _CONV_PW_DEFAULT) != "0"
                 or os.environ.get("FLUXDIST_CONV", "") == "fda")):
        return _FdaConv2dPointwise.apply(x, weight)
    if os.environ.get("FLUXDIST_CONV", "") == "fda" and x.is_cuda:
        raise RuntimeError(
            f"FLUXDIST_CONV=fda but shape unsupported by conv_igemm, the "
            f"stem, conv_stem_narrow, conv_f32, conv_grouped, conv_dw and "
            f"conv_pw kernels: "
            f"x={tuple(x.shape)} w={tuple(weight.shape)} groups={groups}")
    return F.conv2d(x, weight, None, stride, padding, dilation, groups)


class FdaConv2d(torch.nn.Conv2d):
    """nn.Conv2d whose forward goes through fda_conv2d (bias-free, as the
    reference's Flux convs are — /root/reference README.md model usage)."""

    def forward(self, x):
        return fda_conv2d(x, self.weight, self.stride, self.padding,
                          self.dilation, self.groups)
