"""Squeeze-and-Excitation block tail (Hu et al. 2018):

    z = mean_hw(u);  h = relu(W1 z + b1);  s = sigmoid(W2 h + b2)
    out = relu(u * s[n][c] + identity)

On the GPU, for channels_last bf16 activations and bf16 parameters with
C % 64 == 0, 64 <= C <= 2048, Cr % 4 == 0, 4 <= Cr <= 128, the op runs on
csrc/se.hip: three launches forward, four backward, the gate at fp32. Plain
autograd like the grouped conv: no arenas, no direct write into flat G.

Everything else (CPU, fp32, other channel counts) runs the same formula
composed from torch ops, which is also the A/B arm:

  FLUXDIST_SE=1|0  native kernels (1, the default) or the torch composition
                   (0). Read at call time. Measurements: profiles/se.md.
"""

import os

import torch
import torch.nn.functional as F

from .native import require_native

_SE_DEFAULT = "1"


class _SEScaleAddReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, identity, w1, b1, w2, b2):
        C = require_native("se_fwd")
        cl = torch.channels_last
        u = u.contiguous(memory_format=cl)
        out, s, h, z = C.se_fwd(u, identity.contiguous(memory_format=cl),
                                w1.contiguous(), b1.contiguous(),
                                w2.contiguous(), b2.contiguous())
        ctx.save_for_backward(u, out, s, h, z, w1, w2)
        return out

    @staticmethod
    def backward(ctx, gout):
        u, out, s, h, z, w1, w2 = ctx.saved_tensors
        C = require_native("se_bwd")
        gout = gout.contiguous(memory_format=torch.channels_last)
        return C.se_bwd(gout, out, u, s, h, z, w1.contiguous(),
                        w2.contiguous())


def _native_se_supported(u, identity, w1, b1, w2, b2) -> bool:
    """Operands the se.hip kernels serve, FLUXDIST_SE aside."""
    bf16 = torch.bfloat16
    if not (u.is_cuda and u.dim() == 4 and identity.shape == u.shape):
        return False
    if any(t.dtype != bf16 for t in (u, identity, w1, b1, w2, b2)):
        return False
    C, Cr = u.shape[1], w1.shape[0]
    if C % 64 != 0 or not 64 <= C <= 2048:
        return False
    if Cr % 4 != 0 or not 4 <= Cr <= 128:
        return False
    if u.shape[0] > 65535 or u.numel() == 0:
        return False
    return True


def se_scale_add_relu_composed(u, identity, w1, b1, w2, b2):
    """The formula from torch ops, in the operands' dtype."""
    z = u.mean(dim=(2, 3))
    h = torch.relu(F.linear(z, w1, b1))
    s = torch.sigmoid(F.linear(h, w2, b2))
    return torch.relu(u * s[:, :, None, None] + identity)


def se_scale_add_relu(u, identity, w1, b1, w2, b2):
    """relu(u * gate(u) + identity) with the squeeze-and-excitation gate of
    (w1 [Cr, C], b1 [Cr], w2 [C, Cr], b2 [C])."""
    if (os.environ.get("FLUXDIST_SE", _SE_DEFAULT) != "0"
            and _native_se_supported(u, identity, w1, b1, w2, b2)):
        return _SEScaleAddReLU.apply(u, identity, w1, b1, w2, b2)
    return se_scale_add_relu_composed(u, identity, w1, b1, w2, b2)
