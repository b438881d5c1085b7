"""ResNet family (18/34/50/101/152), ResNeXt (50 32x4d, 101 32x4d,
101 64x4d) and their squeeze-and-excitation variants (SE-ResNet 18..152,
SE-ResNeXt 50/101 32x4d), written from scratch for this framework.

Parity: the reference trains Metalhead ResNets — ResNet-34 flagship
(/root/reference/README.md:27), ResNet-50 in the process path
(/root/reference/src/sync.jl:159). Blocks here use the fused BN(+add)+ReLU
op (one HIP kernel on GPU) instead of three separate launches.

Conv weights are bias-free, as in the reference (Flux convs with
`bias=Flux.Zeros` — see SURVEY.md §2.4).
"""

import os
from typing import List, Optional, Tuple, Type

import torch
import torch.nn as nn

from ..ops.conv import FdaConv2d, _native_supported
from ..ops.linear import FdaLinear
from ..ops.se import se_scale_add_relu
from ..ops.functional import (batch_norm_act, batch_norm_act_pool,
                              bn_act_pool_fusible, MaxPool2d, GlobalAvgPool)


class FusedBNAct(nn.Module):
    """BatchNorm2d + optional residual-add + optional ReLU as one op.

    Running stats are per-replica and never synchronized across data-parallel
    replicas — the reference's exact semantic (SURVEY.md §7 hard-part 3:
    grads averaged, running stats drift independently).
    """

    def __init__(self, num_features: int, relu: bool = True,
                 momentum: float = 0.1, eps: float = 1e-5):
        super().__init__()
        self.num_features = num_features
        self.relu = relu
        self.momentum = momentum
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        # batch counter is kept host-side and flushed into the buffer lazily:
        # a per-step GPU scalar add per BN layer was 29 launches/step of pure
        # overhead (profiles/README.md)
        self._nbt_pending = 0

    def _flush_nbt(self):
        if self._nbt_pending:
            self.num_batches_tracked += self._nbt_pending
            self._nbt_pending = 0

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        self._flush_nbt()
        super()._save_to_state_dict(destination, prefix, keep_vars)

    def _load_from_state_dict(self, *args, **kw):
        self._nbt_pending = 0
        super()._load_from_state_dict(*args, **kw)

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None,
                defer_gres: bool = False,
                pool: Optional[Tuple[int, int, int]] = None):
        """`pool=(kernel, stride, padding)` also applies a max-pool to the
        result inside the same native op (ReLU BN without residual only;
        the caller checks bn_act_pool_fusible)."""
        if self.training:
            self._nbt_pending += 1
        if pool is not None:
            if not self.relu or residual is not None:
                raise ValueError("pool fusion needs a ReLU BN without residual")
            return batch_norm_act_pool(
                x, self.weight, self.bias, self.running_mean,
                self.running_var, self.training, self.momentum, self.eps,
                *pool,
            )
        return batch_norm_act(
            x, self.weight, self.bias, self.running_mean, self.running_var,
            self.training, self.momentum, self.eps, self.relu, residual,
            defer_gres,
        )


def _junction_fusible(x: torch.Tensor, conv: nn.Conv2d) -> bool:
    """True when the identity-shortcut junction gradient can be folded into
    `conv`'s native dgrad += epilogue: the SAME tensor x must reach the
    native dgrad (channels_last, native-supported shape) and need a grad.
    The contract is load-bearing — a deferred gres that no dgrad consumes
    raises in ops/step_state.py rather than silently dropping gradient."""
    if os.environ.get("FLUXDIST_JUNCTION", "1") == "0":
        return False
    if not (torch.is_grad_enabled() and x.requires_grad):
        return False
    if not (x.is_cuda and x.is_contiguous(memory_format=torch.channels_last)):
        return False
    return _native_supported(x, conv.weight, conv.stride, conv.padding,
                             conv.dilation, conv.groups)


def conv3x3(cin: int, cout: int, stride: int = 1, groups: int = 1) -> nn.Conv2d:
    return FdaConv2d(cin, cout, 3, stride=stride, padding=1, groups=groups,
                     bias=False)


def conv1x1(cin: int, cout: int, stride: int = 1) -> nn.Conv2d:
    return FdaConv2d(cin, cout, 1, stride=stride, bias=False)


class SqueezeExcite(nn.Module):
    """The gate of a squeeze-and-excitation block (Hu et al. 2018): two
    dense layers C -> C/reduction -> C over the per-image channel means.
    Holds the parameters in the nn.Linear layouts with nn.Linear's default
    initialisation; forward(u, identity) is the whole block tail,
    relu(u * sigmoid(W2 relu(W1 mean_hw(u) + b1) + b2) + identity), one
    native op on the GPU (ops/se.py)."""

    def __init__(self, channels: int, reduction: int = 16):
        super().__init__()
        hidden = channels // reduction
        if hidden < 1:
            raise ValueError(f"SqueezeExcite: {channels} channels cannot be "
                             f"reduced by {reduction}")
        self.channels, self.hidden = channels, hidden
        self.w1 = nn.Parameter(torch.empty(hidden, channels))
        self.b1 = nn.Parameter(torch.empty(hidden))
        self.w2 = nn.Parameter(torch.empty(channels, hidden))
        self.b2 = nn.Parameter(torch.empty(channels))
        self.reset_parameters()

    def reset_parameters(self):
        # nn.Linear.reset_parameters: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for
        # the weight (kaiming_uniform, a = sqrt(5)) and for the bias
        for w, b in ((self.w1, self.b1), (self.w2, self.b2)):
            bound = w.shape[1] ** -0.5
            nn.init.uniform_(w, -bound, bound)
            nn.init.uniform_(b, -bound, bound)

    def forward(self, u, identity):
        return se_scale_add_relu(u, identity, self.w1, self.b1, self.w2,
                                 self.b2)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, cin: int, cout: int, stride: int = 1,
                 downsample: Optional[nn.Module] = None, se: bool = False):
        super().__init__()
        self.conv1 = conv3x3(cin, cout, stride)
        self.bn1 = FusedBNAct(cout, relu=True)
        self.conv2 = conv3x3(cout, cout)
        # fused add+relu via residual arg; an SE block's tail is the SE op
        self.bn2 = FusedBNAct(cout, relu=not se)
        self.downsample = downsample
        if se:
            self.se = SqueezeExcite(cout)

    def forward(self, x):
        if "se" in self._modules:
            # the shortcut first, as below; no junction deferral here
            identity = x if self.downsample is None else self.downsample(x)
            out = self.bn1(self.conv1(x))
            return self.se(self.bn2(self.conv2(out)), identity)
        if self.downsample is not None:
            # downsample runs FIRST: python arg-evaluation order otherwise
            # clobbers conv2's BN-stats stash with the downsample conv's
            # (the 3 residual bn_stats launches in the r2 profile)
            identity = self.downsample(x)
            out = self.bn1(self.conv1(x))
            return self.bn2(self.conv2(out), residual=identity)
        out = self.bn1(self.conv1(x))
        return self.bn2(self.conv2(out), residual=x,
                        defer_gres=_junction_fusible(x, self.conv1))


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, cin: int, cout: int, stride: int = 1,
                 downsample: Optional[nn.Module] = None, groups: int = 1,
                 base_width: int = 64, se: bool = False):
        super().__init__()
        # ResNeXt: the 3x3 conv is grouped and the inner width scales with
        # base_width; groups=1, base_width=64 is the plain bottleneck
        width = int(cout * base_width / 64) * groups
        self.conv1 = conv1x1(cin, width)
        self.bn1 = FusedBNAct(width, relu=True)
        self.conv2 = conv3x3(width, width, stride, groups)
        self.bn2 = FusedBNAct(width, relu=True)
        self.conv3 = conv1x1(width, cout * self.expansion)
        self.bn3 = FusedBNAct(cout * self.expansion, relu=not se)
        self.downsample = downsample
        if se:
            self.se = SqueezeExcite(cout * self.expansion)

    def forward(self, x):
        if "se" in self._modules:
            identity = x if self.downsample is None else self.downsample(x)
            out = self.bn1(self.conv1(x))
            out = self.bn2(self.conv2(out))
            return self.se(self.bn3(self.conv3(out)), identity)
        if self.downsample is not None:
            identity = self.downsample(x)   # first — see BasicBlock note
            out = self.bn1(self.conv1(x))
            out = self.bn2(self.conv2(out))
            return self.bn3(self.conv3(out), residual=identity)
        out = self.bn1(self.conv1(x))
        out = self.bn2(self.conv2(out))
        return self.bn3(self.conv3(out), residual=x,
                        defer_gres=_junction_fusible(x, self.conv1))


class Downsample(nn.Module):
    """1x1 strided conv + BN (no activation) on the identity path."""

    def __init__(self, cin: int, cout: int, stride: int):
        super().__init__()
        self.conv = conv1x1(cin, cout, stride)
        self.bn = FusedBNAct(cout, relu=False)

    def forward(self, x):
        return self.bn(self.conv(x))


class ResNet(nn.Module):
    def __init__(self, block: Type[nn.Module], layers: List[int],
                 num_classes: int = 1000, small_input: bool = False,
                 groups: int = 1, width_per_group: int = 64,
                 se: bool = False):
        super().__init__()
        if (groups, width_per_group) != (1, 64) and block is not Bottleneck:
            raise ValueError("groups / width_per_group need Bottleneck blocks")
        self.small_input = small_input
        # extra block arguments: none for the plain ResNets
        self._block_kw = ({} if (groups, width_per_group) == (1, 64) else
                          dict(groups=groups, base_width=width_per_group))
        if se:
            self._block_kw = dict(self._block_kw, se=True)
        self.cin = 64
        if small_input:  # CIFAR-style stem (BASELINE config 1)
            self.conv1 = FdaConv2d(3, 64, 3, stride=1, padding=1, bias=False)
            self.maxpool = nn.Identity()
        else:
            self.conv1 = FdaConv2d(3, 64, 7, stride=2, padding=3, bias=False)
            self.maxpool = MaxPool2d(3, stride=2, padding=1)
        self.bn1 = FusedBNAct(64, relu=True)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.avgpool = GlobalAvgPool()
        self.fc = FdaLinear(512 * block.expansion, num_classes)
        self._init_weights()

    def _make_layer(self, block, cout, n, stride=1):
        downsample = None
        if stride != 1 or self.cin != cout * block.expansion:
            downsample = Downsample(self.cin, cout * block.expansion, stride)
        kw = self._block_kw
        blocks = [block(self.cin, cout, stride, downsample, **kw)]
        self.cin = cout * block.expansion
        blocks += [block(self.cin, cout, **kw) for _ in range(n - 1)]
        return nn.Sequential(*blocks)

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.zeros_(m.bias)

    def _stem_pool(self, y: torch.Tensor) -> Optional[Tuple[int, int, int]]:
        """Pool geometry when the stem tail (bn1 + ReLU + maxpool) can run
        as one native op, else None. FLUXDIST_STEM_FUSE=0 turns it off."""
        mp = self.maxpool
        if type(mp) is not MaxPool2d or not self.bn1.relu:
            return None
        if os.environ.get("FLUXDIST_STEM_FUSE", "1") == "0":
            return None
        geom = (mp.kernel_size, mp.stride, mp.padding)
        if not (y.is_cuda and all(isinstance(g, int) for g in geom)):
            return None
        return geom if bn_act_pool_fusible(y, *geom) else None

    def forward(self, x):
        y = self.conv1(x)
        pool = self._stem_pool(y)
        if pool is not None:
            x = self.bn1(y, pool=pool)
        else:
            x = self.maxpool(self.bn1(y))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = self.avgpool(x)
        return self.fc(x)


def resnet18(**kw):
    return ResNet(BasicBlock, [2, 2, 2, 2], **kw)


def resnet34(**kw):
    return ResNet(BasicBlock, [3, 4, 6, 3], **kw)


def resnet50(**kw):
    return ResNet(Bottleneck, [3, 4, 6, 3], **kw)


def resnet101(**kw):
    return ResNet(Bottleneck, [3, 4, 23, 3], **kw)


def resnet152(**kw):
    return ResNet(Bottleneck, [3, 8, 36, 3], **kw)


def resnext50_32x4d(**kw):
    return ResNet(Bottleneck, [3, 4, 6, 3], groups=32, width_per_group=4, **kw)


def resnext101_32x4d(**kw):
    return ResNet(Bottleneck, [3, 4, 23, 3], groups=32, width_per_group=4, **kw)


def resnext101_64x4d(**kw):
    return ResNet(Bottleneck, [3, 4, 23, 3], groups=64, width_per_group=4, **kw)


def se_resnet18(**kw):
    return ResNet(BasicBlock, [2, 2, 2, 2], se=True, **kw)


def se_resnet34(**kw):
    return ResNet(BasicBlock, [3, 4, 6, 3], se=True, **kw)


def se_resnet50(**kw):
    return ResNet(Bottleneck, [3, 4, 6, 3], se=True, **kw)


def se_resnet101(**kw):
    return ResNet(Bottleneck, [3, 4, 23, 3], se=True, **kw)


def se_resnet152(**kw):
    return ResNet(Bottleneck, [3, 8, 36, 3], se=True, **kw)


def se_resnext50_32x4d(**kw):
    return ResNet(Bottleneck, [3, 4, 6, 3], groups=32, width_per_group=4,
                  se=True, **kw)


def se_resnext101_32x4d(**kw):
    return ResNet(Bottleneck, [3, 4, 23, 3], groups=32, width_per_group=4,
                  se=True, **kw)


_ZOO = {
    "resnet18": resnet18,
    "resnet34": resnet34,
    "resnet50": resnet50,
    "resnet101": resnet101,
    "resnet152": resnet152,
    "resnext50_32x4d": resnext50_32x4d,
    "resnext101_32x4d": resnext101_32x4d,
    "resnext101_64x4d": resnext101_64x4d,
    "se_resnet18": se_resnet18,
    "se_resnet34": se_resnet34,
    "se_resnet50": se_resnet50,
    "se_resnet101": se_resnet101,
    "se_resnet152": se_resnet152,
    "se_resnext50_32x4d": se_resnext50_32x4d,
    "se_resnext101_32x4d": se_resnext101_32x4d,
}


def build_model(name: str, num_classes: int = 1000,
                small_input: bool = False) -> nn.Module:
    if name not in _ZOO:
        raise ValueError(f"unknown model '{name}'; choose from {sorted(_ZOO)}")
    return _ZOO[name](num_classes=num_classes, small_input=small_input)
