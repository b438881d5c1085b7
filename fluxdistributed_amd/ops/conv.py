"""Conv2d dispatch: hand-written MFMA implicit-GEMM kernels with library
fallback.

The reference gets conv from cuDNN via NNlibCUDA; the
MI355X-native path is fluxdistributed_amd/csrc/conv_igemm.hip —
v_mfma_f32_16x16x32_bf16 tiles, LDS-staged via global_load_lds. Supported
there: NHWC bf16, dilation 1, groups 1, C and K multiples of 64 (all
ResNet body convs) — fwd, dgrad AND wgrad. Small-C stems (C<=5, e.g. the
ImageNet 7x7 and CIFAR 3x3 stems) run on the dedicated CONV_STEM kernels;
only genuinely unsupported shapes (grouped/dilated, odd channel counts)
fall back to the library path.

Env:
  FLUXDIST_CONV=miopen   force the library path everywhere (A/B testing)
  FLUXDIST_CONV=fda      force the native path (errors on unsupported)
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


def fda_conv2d(x: torch.Tensor, weight: torch.Tensor, stride=(1, 1),
               padding=(0, 0), dilation=(1, 1), groups: int = 1) -> torch.Tensor:
    """conv2d with per-shape dispatch to the native MFMA kernel."""
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    if _native_supported(x, weight, stride, padding, dilation, groups):
        return _FdaConv2d.apply(x, weight, stride, padding, _want_conv_stats())
    if _stem_supported(x, weight, stride, padding, dilation, groups):
        return _FdaStemConv2d.apply(x, weight, stride, padding,
                                    _want_conv_stats())
    if os.environ.get("FLUXDIST_CONV", "") == "fda" and x.is_cuda:
        raise RuntimeError(
            f"FLUXDIST_CONV=fda but shape unsupported by conv_igemm: "
            f"x={tuple(x.shape)} w={tuple(weight.shape)} groups={groups}")
    return F.conv2d(x, weight, None, stride, padding, dilation, groups)


class FdaConv2d(torch.nn.Conv2d):
    """nn.Conv2d whose forward goes through fda_conv2d (bias-free, as the
    reference's Flux convs are — /root/reference README.md model usage)."""

    def forward(self, x):
        return fda_conv2d(x, self.weight, self.stride, self.padding,
                          self.dilation, self.groups)
