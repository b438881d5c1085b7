"""MobileNetV1 (Howard et al. 2017, "MobileNets: Efficient Convolutional
Neural Networks for Mobile Vision Applications"), written from scratch for
this framework from the paper's layer table.

A 3x3 stride-2 stem, 13 depthwise-separable blocks of [depthwise 3x3, BN,
ReLU, pointwise 1x1, BN, ReLU], global average pool and one dense layer.
On the GPU the depthwise convs run on csrc/conv_dw.hip (FLUXDIST_CONV_DW),
the pointwise convs on conv_igemm where both channel counts are multiples of
64 and, with FLUXDIST_CONV_PW=1, on csrc/conv_pw.hip where they are narrower
(the first one at width 1.0, most of them at smaller widths, up to 256
channels); BN+ReLU is the fused op. The stem (K = 32 at width 1.0, 8 to 24 at
smaller widths) runs on csrc/conv_stem_narrow.hip with
FLUXDIST_CONV_STEM_NARROW=1 (opt-in: its wgrad is slower than the library's
at 224x224) and stays on the library otherwise. The BNs whose channel count
is a multiple of 8 but not of 64 (the two 32-channel ones at width 1.0, after
the stem and after the first depthwise conv; more at smaller widths) run on
the fused BN kernels too (FLUXDIST_BN_NARROW, on by default; BNAct below).
With FLUXDIST_CONV_STEM_NARROW=1 and FLUXDIST_CONV_PW=1, or with
FLUXDIST_CONV=fda, no conv or BN of a training step at widths 0.25 to 1.0
goes to the library. Defaults and their measured reasons: docs/kernels.md.

Conv weights are bias-free, like the ResNets'.
"""

import os
from typing import List, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.conv import FdaConv2d
from ..ops.functional import GlobalAvgPool
from ..ops.linear import FdaLinear
from .resnet import _ZOO, FusedBNAct, ResNet

# (output channels, stride) of the 13 depthwise-separable blocks
_BLOCKS: List[Tuple[int, int]] = (
    [(64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2)]
    + [(512, 1)] * 5 + [(1024, 2), (1024, 1)])


def _width(channels: int, mult: float) -> int:
    """channels * mult rounded to a multiple of 8, at least 8."""
    return max(8, int(channels * mult + 4) // 8 * 8)


# On by default: at 32 channels and 96x112x112 the native pair is 4.4x (fwd)
# and 4.5x (bwd) faster than the composition, the step 1.16x
# (profiles/conv_stem_narrow.md).
_BN_NARROW_DEFAULT = "1"


class BNAct(FusedBNAct):
    """FusedBNAct for any channel count. Multiples of 64 channels always run
    the native BN kernels. A narrower layer on the GPU (32 channels at width
    1.0, other widths at other multipliers) runs them too where the count is
    a multiple of 8, in bf16, unless FLUXDIST_BN_NARROW=0 (read at call time);
    with FLUXDIST_BN_NARROW=0 and for other counts it is the composition of
    library ops that batch_norm_act uses as its CPU form, in fp32. Same
    parameters, buffers and state dict either way."""

    def forward(self, x):
        C = self.num_features
        if C % 64 == 0 or not x.is_cuda or (
                C % 8 == 0 and x.dtype == torch.bfloat16
                and os.environ.get("FLUXDIST_BN_NARROW",
                                   _BN_NARROW_DEFAULT) != "0"):
            return super().forward(x)
        if self.training:
            self._nbt_pending += 1
        out = F.batch_norm(x.float(), self.running_mean, self.running_var,
                           self.weight, self.bias, self.training,
                           self.momentum, self.eps)
        return (torch.relu(out) if self.relu else out).to(x.dtype)


class DepthwiseSeparable(nn.Module):
    """depthwise 3x3 (stride) -> BN -> ReLU -> pointwise 1x1 -> BN -> ReLU"""

    def __init__(self, cin: int, cout: int, stride: int):
        super().__init__()
        self.dw = FdaConv2d(cin, cin, 3, stride=stride, padding=1, groups=cin,
                            bias=False)
        self.bn1 = BNAct(cin, relu=True)
        self.pw = FdaConv2d(cin, cout, 1, bias=False)
        self.bn2 = BNAct(cout, relu=True)

    def forward(self, x):
        x = self.bn1(self.dw(x))
        return self.bn2(self.pw(x))


class MobileNetV1(nn.Module):
    def __init__(self, num_classes: int = 1000, small_input: bool = False,
                 width_mult: float = 1.0):
        super().__init__()
        self.small_input = small_input
        cin = _width(32, width_mult)
        # small_input: a stride-1 stem, as the ResNets' CIFAR stem
        self.conv1 = FdaConv2d(3, cin, 3, stride=1 if small_input else 2,
                               padding=1, bias=False)
        self.bn1 = BNAct(cin, relu=True)
        blocks = []
        for cout, stride in _BLOCKS:
            cout = _width(cout, width_mult)
            blocks.append(DepthwiseSeparable(cin, cout, stride))
            cin = cout
        self.features = nn.Sequential(*blocks)
        self.avgpool = GlobalAvgPool()
        self.fc = FdaLinear(cin, num_classes)
        ResNet._init_weights(self)

    def forward(self, x):
        x = self.bn1(self.conv1(x))
        x = self.features(x)
        return self.fc(self.avgpool(x))


def mobilenet_v1(**kw):
    return MobileNetV1(**kw)


_ZOO["mobilenet_v1"] = mobilenet_v1
