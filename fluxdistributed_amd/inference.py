"""Forward-only ResNet execution with BatchNorm folded into the conv epilogue.

`compile_for_inference(model)` pairs every `FdaConv2d` of a `ResNet` with the
`FusedBNAct` that consumes it. In eval mode that BatchNorm is a per-channel
affine with fixed coefficients, so on the native path a pair runs as ONE
kernel: conv_igemm's inference epilogue computes

    y = bf16(relu(fma(acc, scale[k], shift[k]) + residual))

from the fp32 accumulator, rounded once. The conv output is never written
and read back for a separate BN pass; block tails take the shortcut as the
`residual` operand. scale/shift of ALL layers come from one batched fold
launch (`bn_fold_eval_batch`) into a flat fp32 arena.

Wherever the native kernels do not apply (CPU, fp32, FLUXDIST_CONV=miopen,
unsupported channel counts) or with FLUXDIST_INFER_FUSE=0, a pair runs the
model's own ops (`fda_conv2d`, then `batch_norm_act(training=False)`), and
the output is bit-identical to `model.eval()(x)`.

The wrapped model is only read: `model.training`, the running statistics
and `num_batches_tracked` are never touched.
"""

import os
from typing import List, Optional

import torch
import torch.nn as nn

from .models.resnet import (BasicBlock, Bottleneck, Downsample, FusedBNAct,
                            ResNet)
from .ops.conv import (FdaConv2d, _native_supported, _stem_supported,
                       fda_conv2d, pack_stem_operands, stem_buffer_key)
from .ops.functional import (GlobalAvgPool, MaxPool2d, batch_norm_act,
                             batch_norm_act_pool)
from .ops.linear import FdaLinear
from .ops.native import require_native


def _fuse_enabled() -> bool:
    return os.environ.get("FLUXDIST_INFER_FUSE", "1") != "0"


class _Pair:
    """One conv and the BatchNorm that consumes it; `index` is the pair's
    slot in the fold arena's tables."""

    __slots__ = ("conv", "bn", "index", "offset")

    def __init__(self, conv, bn, index):
        if not isinstance(conv, FdaConv2d):
            raise TypeError(
                f"compile_for_inference: expected FdaConv2d, got "
                f"{type(conv).__name__}")
        if not isinstance(bn, FusedBNAct):
            raise TypeError(
                f"compile_for_inference: expected FusedBNAct after a conv, "
                f"got {type(bn).__name__}")
        if conv.bias is not None:
            raise TypeError("compile_for_inference: conv with a bias has no "
                            "fused form")
        if conv.out_channels != bn.num_features:
            raise ValueError("compile_for_inference: conv/BN channel mismatch")
        self.conv, self.bn, self.index = conv, bn, index
        self.offset = 0


class _Block:
    __slots__ = ("pairs", "down")

    def __init__(self, pairs, down):
        self.pairs, self.down = pairs, down


class _FoldArena:
    """scale/shift of every paired BN in one flat fp32 buffer, recomputed by
    a single bn_fold_eval_batch launch. Pair i owns [offset, offset + 2C):
    scale then shift. The launch reads the BN tensors through device-side
    address tables; those are revalidated on the host before every fold,
    because a `.to()` or a checkpoint load rebinds the storages."""

    def __init__(self, pairs: List[_Pair], device):
        self.pairs = pairs
        self.device = device
        off = 0
        for p in pairs:
            p.offset = off
            off += 2 * p.bn.num_features
        self.arena = torch.empty(off, dtype=torch.float32, device=device)
        self.max_c = max(p.bn.num_features for p in pairs)
        self.ptrs = None
        self.meta = None

    def _tensors(self):
        out = []
        for p in self.pairs:
            bn = p.bn
            out += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
        return out

    def fold(self):
        ts = self._tensors()
        ptrs = [t.data_ptr() for t in ts]
        if ptrs != self.ptrs:
            for t in ts:
                if not (t.device == self.device and t.dtype == torch.float32
                        and t.is_contiguous()):
                    raise RuntimeError(
                        "InferenceModel: BatchNorm parameters and statistics "
                        "must be contiguous fp32 on the model's device")
            dev = self.device
            mk = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
            self.meta = (
                mk(ptrs[0::4], torch.long), mk(ptrs[1::4], torch.long),
                mk(ptrs[2::4], torch.long), mk(ptrs[3::4], torch.long),
                mk([p.bn.num_features for p in self.pairs], torch.int32),
                mk([p.offset for p in self.pairs], torch.long),
                mk([p.bn.eps for p in self.pairs], torch.float32))
            self.ptrs = ptrs
        C = require_native("bn_fold_eval_batch")
        C.bn_fold_eval_batch(*self.meta, self.arena, self.max_c)

    def coeffs(self, p: _Pair):
        n = p.bn.num_features
        return (self.arena[p.offset:p.offset + n],
                self.arena[p.offset + n:p.offset + 2 * n])


class InferenceModel:
    """Forward-only view of a `ResNet` (see the module docstring).

    By default the BN coefficients are recomputed from the live parameters
    and running statistics at the start of every call, so they can never be
    stale. `freeze()` snapshots them once for serving; `refresh()` takes a
    new snapshot.
    """

    def __init__(self, model: nn.Module):
        if not isinstance(model, ResNet):
            raise TypeError(
                f"compile_for_inference: expected a ResNet, got "
                f"{type(model).__name__}")
        self.model = model
        self.pairs: List[_Pair] = []
        claimed = {id(model)}

        def pair(conv, bn):
            p = _Pair(conv, bn, len(self.pairs))
            self.pairs.append(p)
            claimed.update((id(conv), id(bn)))
            return p

        self.stem = pair(model.conv1, model.bn1)
        if not self.stem.bn.relu:
            raise TypeError("compile_for_inference: stem BN without ReLU")
        if not isinstance(model.maxpool, (MaxPool2d, nn.Identity)):
            raise TypeError(
                f"compile_for_inference: unrecognised stem pool "
                f"{type(model.maxpool).__name__}")
        if not isinstance(model.avgpool, GlobalAvgPool):
            raise TypeError(
                f"compile_for_inference: unrecognised head pool "
                f"{type(model.avgpool).__name__}")
        if not isinstance(model.fc, FdaLinear):
            raise TypeError(
                f"compile_for_inference: unrecognised classifier "
                f"{type(model.fc).__name__}")
        claimed.update(id(m) for m in (model.maxpool, model.avgpool, model.fc))

        self.blocks: List[_Block] = []
        for layer in (model.layer1, model.layer2, model.layer3, model.layer4):
            if not isinstance(layer, nn.Sequential):
                raise TypeError("compile_for_inference: a ResNet stage must "
                                "be an nn.Sequential of blocks")
            claimed.add(id(layer))
            for blk in layer:
                claimed.add(id(blk))
                down = None
                if blk.__dict__["_modules"].get("downsample") is not None:
                    ds = blk.downsample
                    if type(ds) is not Downsample:
                        raise TypeError(
                            f"compile_for_inference: unrecognised shortcut "
                            f"{type(ds).__name__}")
                    claimed.add(id(ds))
                    down = pair(ds.conv, ds.bn)
                    if down.bn.relu:
                        raise TypeError("compile_for_inference: shortcut BN "
                                        "with ReLU")
                if type(blk) is BasicBlock:
                    body = [pair(blk.conv1, blk.bn1), pair(blk.conv2, blk.bn2)]
                elif type(blk) is Bottleneck:
                    body = [pair(blk.conv1, blk.bn1), pair(blk.conv2, blk.bn2),
                            pair(blk.conv3, blk.bn3)]
                else:
                    raise TypeError(
                        f"compile_for_inference: unrecognised block "
                        f"{type(blk).__name__}")
                if not all(p.bn.relu for p in body):
                    raise TypeError("compile_for_inference: block BN without "
                                    "ReLU")
                self.blocks.append(_Block(body, down))

        # nothing the walk did not pair may remain: a module this code does
        # not know would otherwise be dropped from the forward silently
        for name, m in model.named_modules():
            if id(m) not in claimed:
                raise TypeError(
                    f"compile_for_inference: unrecognised module '{name}' "
                    f"({type(m).__name__})")

        self._frozen = False
        self._snap = None          # per pair (weight, bias, mean, var) clones
        self._arena: Optional[_FoldArena] = None
        self._arena_fresh = False  # arena folded since it was (re)built
        self._x8 = {}            # padded stem inputs, by shape

    # ---- coefficients ----------------------------------------------------

    def _fold_arena(self, device) -> Optional[_FoldArena]:
        """The fold arena on `device`, or None where the fused kernels cannot
        run at all (no GPU, BN tensors not fp32 there)."""
        if device.type != "cuda":
            return None
        if self._arena is None or self._arena.device != device:
            for p in self.pairs:
                bn = p.bn
                for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
                    if t.device != device or t.dtype != torch.float32:
                        return None
            self._arena = _FoldArena(self.pairs, device)
            self._arena_fresh = False
        return self._arena

    def refresh(self) -> "InferenceModel":
        """Recompute the BN coefficients from the model's current state."""
        self._snap = [tuple(t.detach().clone() for t in
                            (p.bn.weight, p.bn.bias, p.bn.running_mean,
                             p.bn.running_var)) for p in self.pairs]
        arena = self._fold_arena(self.pairs[0].bn.weight.device)
        if arena is not None:
            with torch.no_grad():
                arena.fold()
            self._arena_fresh = True
        return self

    def freeze(self) -> "InferenceModel":
        """Snapshot the BN coefficients now and stop recomputing them per
        call (serving). Later changes to the BN parameters or running
        statistics are ignored until `refresh()`."""
        self.refresh()
        self._frozen = True
        return self

    def _bn_state(self, p: _Pair):
        if self._frozen:
            return self._snap[p.index]
        bn = p.bn
        return bn.weight, bn.bias, bn.running_mean, bn.running_var

    # ---- one conv + BN pair ----------------------------------------------

    def _stem_fused(self, p: _Pair, x, scale, shift):
        C = require_native("conv_stem_fwd_fused")
        conv = p.conv
        # the padded buffer is this object's own, so a captured graph keeps
        # replaying into memory nobody else checks out
        key = stem_buffer_key(x, conv.weight, conv.padding)
        x8, wpad, P, Q = pack_stem_operands(x, conv.weight, conv.stride,
                                            conv.padding, self._x8.get(key))
        self._x8[key] = x8
        return C.conv_stem_fwd_fused(x8, wpad, scale, shift, p.bn.relu,
                                     conv.weight.shape[2], *conv.stride, P, Q)

    def _run_pair(self, p: _Pair, x, residual=None, fuse=False):
        conv, bn = p.conv, p.bn
        geom = (conv.stride, conv.padding, conv.dilation, conv.groups)
        if fuse:
            scale, shift = self._arena.coeffs(p)
            if _native_supported(x, conv.weight, *geom):
                C = require_native("conv_igemm_fwd_fused")
                cl = torch.channels_last
                res = (residual.contiguous(memory_format=cl)
                       if residual is not None
                       else torch.empty(0, device=x.device, dtype=x.dtype))
                return C.conv_igemm_fwd_fused(
                    x.contiguous(memory_format=cl),
                    conv.weight.contiguous(memory_format=cl), scale, shift,
                    res, bn.relu, *conv.stride, *conv.padding)
            if residual is None and _stem_supported(x, conv.weight, *geom):
                return self._stem_fused(p, x, scale, shift)
        y = fda_conv2d(x, conv.weight, *geom)
        w, b, rm, rv = self._bn_state(p)
        return batch_norm_act(y, w, b, rm, rv, False, bn.momentum, bn.eps,
                              bn.relu, residual)

    def _stem(self, x, fuse):
        model, p = self.model, self.stem
        conv = p.conv
        geom = (conv.stride, conv.padding, conv.dilation, conv.groups)
        if fuse and (_native_supported(x, conv.weight, *geom)
                     or _stem_supported(x, conv.weight, *geom)):
            return model.maxpool(self._run_pair(p, x, fuse=True))
        # the model's own stem, BN+ReLU+pool fusion included
        y = fda_conv2d(x, conv.weight, *geom)
        w, b, rm, rv = self._bn_state(p)
        pool = model._stem_pool(y)
        if pool is not None:
            return batch_norm_act_pool(y, w, b, rm, rv, False, p.bn.momentum,
                                       p.bn.eps, *pool)
        return model.maxpool(batch_norm_act(y, w, b, rm, rv, False,
                                            p.bn.momentum, p.bn.eps, True))

    # ---- forward -----------------------------------------------------------

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            fuse = False
            if _fuse_enabled() and x.is_cuda and x.dtype == torch.bfloat16:
                arena = self._fold_arena(x.device)
                if arena is not None:
                    fuse = True
                    if not self._frozen or not self._arena_fresh:
                        arena.fold()
                        self._arena_fresh = True
            x = self._stem(x, fuse)
            for blk in self.blocks:
                identity = x
                if blk.down is not None:
                    identity = self._run_pair(blk.down, x, fuse=fuse)
                out = x
                for p in blk.pairs[:-1]:
                    out = self._run_pair(p, out, fuse=fuse)
                x = self._run_pair(blk.pairs[-1], out, residual=identity,
                                   fuse=fuse)
            return self.model.fc(self.model.avgpool(x))

    def capture(self, example_x: torch.Tensor, warmup: int = 3):
        """Capture the forward for `example_x`'s shape into a hipGraph and
        return a callable that replays it (single stream, static input copy,
        side-stream warmup, as GraphedTrainStep). Unless frozen, the fold
        launch is part of the graph, so a replay sees the current running
        statistics. The returned logits are the graph's static output: clone
        them to keep them past the next call."""
        if not example_x.is_cuda:
            raise ValueError("graph capture needs a GPU tensor")
        static_x = example_x.clone(memory_format=torch.preserve_format)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(max(1, warmup)):
                self(static_x)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = self(static_x)
        return _GraphedForward(graph, static_x, static_out)


class _GraphedForward:
    def __init__(self, graph, static_x, static_out):
        self.graph, self.static_x, self.static_out = graph, static_x, static_out

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if x.shape != self.static_x.shape:
            raise ValueError(
                f"captured for input shape {tuple(self.static_x.shape)}, got "
                f"{tuple(x.shape)}")
        self.static_x.copy_(x, non_blocking=True)
        self.graph.replay()
        return self.static_out


def compile_for_inference(model: nn.Module) -> InferenceModel:
    """Pair every conv of a `ResNet` with its BatchNorm for fused forward-only
    execution. Raises TypeError on a module it does not recognise."""
    return InferenceModel(model)
