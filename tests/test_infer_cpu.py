"""InferenceModel without a GPU: layer pairing, bit-equality with
model.eval() on the fallback path, no side effects on the wrapped model,
freeze()/refresh() semantics, and the operand checks of the three
inference bindings."""

import copy

import pytest
import torch
import torch.nn as nn

import fluxdistributed_amd as fda
from fluxdistributed_amd.inference import InferenceModel, compile_for_inference
from fluxdistributed_amd.models import build_model
from fluxdistributed_amd.models.resnet import FusedBNAct
from fluxdistributed_amd.ops.conv import FdaConv2d
from fluxdistributed_amd.ops.native import load_native


def randomize_bn(model, seed=1):
    """Fresh-init BN makes the fold a near no-op and hides pairing bugs."""
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, FusedBNAct):
            n = m.num_features
            with torch.no_grad():
                m.weight.copy_(0.25 + 1.5 * torch.rand(n, generator=g))
                m.weight.mul_(torch.where(torch.rand(n, generator=g) < 0.5,
                                          -1.0, 1.0))
                m.bias.copy_(0.5 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.5 * torch.randn(n, generator=g))
                m.running_var.copy_(0.5 + 1.5 * torch.rand(n, generator=g))
    return model


def make(name):
    torch.manual_seed(0)
    return randomize_bn(build_model(name, num_classes=10, small_input=True))


def bn_state(model):
    out = {}
    for n, m in model.named_modules():
        if isinstance(m, FusedBNAct):
            m._flush_nbt()
            out[n] = (m.running_mean.clone(), m.running_var.clone(),
                      m.num_batches_tracked.clone(), m._nbt_pending)
    return out


def same_state(a, b):
    return a.keys() == b.keys() and all(
        torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1])
        and torch.equal(a[k][2], b[k][2]) and a[k][3] == b[k][3] for k in a)


@pytest.fixture(scope="module")
def x():
    return torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(7))


@pytest.fixture(scope="module", params=["resnet18", "resnet50"])
def model(request):
    return make(request.param)


def test_exported_from_package_root():
    assert fda.compile_for_inference is compile_for_inference
    assert fda.InferenceModel is InferenceModel


def test_bit_equal_to_eval_and_no_side_effects(model, x):
    ref_model = copy.deepcopy(model).eval()
    with torch.no_grad():
        ref = ref_model(x)
    model.eval()
    before = bn_state(model)
    im = compile_for_inference(model)
    out = im(x)
    assert not out.requires_grad
    assert torch.equal(out, ref)
    assert model.training is False
    assert same_state(before, bn_state(model))


def test_train_mode_model_uses_running_stats_and_is_untouched(model, x):
    ref_model = copy.deepcopy(model).eval()
    with torch.no_grad():
        ref = ref_model(x)
    model.train()
    try:
        before = bn_state(model)
        out = compile_for_inference(model)(x)
        assert torch.equal(out, ref)
        assert model.training is True
        assert all(m.training for m in model.modules())
        assert same_state(before, bn_state(model))
    finally:
        model.eval()


@pytest.mark.parametrize("name,count", [("resnet18", 20), ("resnet50", 53)])
def test_pair_count_equals_conv_count(name, count):
    m = build_model(name, num_classes=10, small_input=True)
    im = compile_for_inference(m)
    assert sum(isinstance(s, FdaConv2d) for s in m.modules()) == count
    assert len(im.pairs) == count
    assert len({id(p.conv) for p in im.pairs}) == count
    assert len({id(p.bn) for p in im.pairs}) == count


def test_unknown_modules_raise():
    with pytest.raises(TypeError, match="ResNet"):
        compile_for_inference(nn.Sequential(nn.Conv2d(3, 8, 3)))
    m = build_model("resnet18", num_classes=10, small_input=True)
    m.extra = nn.Dropout()
    with pytest.raises(TypeError, match="extra"):
        compile_for_inference(m)
    m = build_model("resnet18", num_classes=10, small_input=True)
    m.layer2[1] = nn.Identity()
    with pytest.raises(TypeError, match="unrecognised block"):
        compile_for_inference(m)
    m = build_model("resnet18", num_classes=10, small_input=True)
    m.layer1[0].bn1 = nn.BatchNorm2d(64)
    with pytest.raises(TypeError, match="FusedBNAct"):
        compile_for_inference(m)
    m = build_model("resnet18", num_classes=10, small_input=True)
    m.layer1[0].conv1 = nn.Conv2d(64, 64, 3, padding=1, bias=False)
    with pytest.raises(TypeError, match="FdaConv2d"):
        compile_for_inference(m)


def test_refresh_and_freeze(x):
    m = make("resnet18").eval()
    im = compile_for_inference(m)
    y0 = im(x)
    with torch.no_grad():
        m.layer3[0].bn2.running_mean.add_(0.75)
    y1 = im(x)
    assert not torch.equal(y1, y0)          # live by default
    with torch.no_grad():
        assert torch.equal(y1, m(x))

    assert im.freeze() is im
    yf = im(x)
    assert torch.equal(yf, y1)
    with torch.no_grad():
        m.layer3[0].bn2.running_mean.sub_(0.75)
        m.bn1.running_var.mul_(2.0)
        m.layer1[1].bn1.weight.mul_(0.5)
    assert torch.equal(im(x), yf)            # the snapshot holds
    im.refresh()
    y2 = im(x)
    assert not torch.equal(y2, yf)
    with torch.no_grad():
        assert torch.equal(y2, m(x))


def test_log_loss_and_acc_fused_is_opt_in_and_leaves_the_mode():
    from fluxdistributed_amd.ops import logit_cross_entropy
    from fluxdistributed_amd.parallel.task_ddp import Replica, log_loss_and_acc

    m = make("resnet18").train()
    g = torch.Generator().manual_seed(2)
    val = (torch.randn(4, 3, 32, 32, generator=g),
           torch.randint(0, 10, (4,), generator=g))
    rep = Replica(0, "cpu", m, None)
    before = bn_state(m)
    default = log_loss_and_acc(logit_cross_entropy, rep, val, ks=(1, 5))
    fused = log_loss_and_acc(logit_cross_entropy, rep, val, ks=(1, 5),
                             fused=True)
    assert fused == default          # CPU: the fallback is the eval path
    assert m.training and all(s.training for s in m.modules())
    assert same_state(before, bn_state(m))


# ---- operand checks of the new bindings ------------------------------------
# As tests/test_conv_operand_checks.py: only where no GPU is visible, so a
# regression in a check can never hand a bad pointer to a kernel.

C = load_native()
cpu_only = pytest.mark.skipif(
    torch.cuda.is_available() or C is None,
    reason="CPU-only: must never reach a launch")


def _cl(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype).contiguous(
        memory_format=torch.channels_last)


def _f32(n):
    return torch.zeros(n, dtype=torch.float32)


NONE = torch.empty(0, dtype=torch.bfloat16)


def _fused(x=None, w=None, scale=None, shift=None, res=NONE, sy=1, py=1):
    x = _cl(1, 64, 4, 4) if x is None else x
    w = _cl(128, 64, 3, 3) if w is None else w
    scale = _f32(128) if scale is None else scale
    shift = _f32(128) if shift is None else shift
    return C.conv_igemm_fwd_fused(x, w, scale, shift, res, True, sy, sy, py, py)


@cpu_only
def test_fused_conv_refusals():
    # valid operands get as far as the device check, which comes last
    with pytest.raises(RuntimeError, match="device tensors required"):
        _fused()
    with pytest.raises(RuntimeError, match="device tensors required"):
        _fused(res=_cl(1, 128, 4, 4))
    with pytest.raises(RuntimeError, match="channels_last bf16"):
        _fused(x=_cl(1, 64, 4, 4, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="channels_last bf16"):
        _fused(x=torch.zeros(1, 64, 4, 4, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="multiples of 64"):
        _fused(x=_cl(1, 32, 4, 4), w=_cl(128, 32, 3, 3))
    with pytest.raises(RuntimeError, match="channel mismatch"):
        _fused(w=_cl(128, 128, 3, 3))
    with pytest.raises(RuntimeError, match="stride/padding"):
        _fused(sy=0)
    with pytest.raises(RuntimeError, match="scale must be contiguous"):
        _fused(scale=_f32(64))
    with pytest.raises(RuntimeError, match="scale must be contiguous"):
        _fused(scale=torch.zeros(128, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="shift must be contiguous"):
        _fused(shift=_f32(256)[::2])
    with pytest.raises(RuntimeError, match="residual must be"):
        _fused(res=_cl(1, 128, 2, 2))                     # wrong spatial size
    with pytest.raises(RuntimeError, match="residual must be"):
        _fused(res=_cl(1, 64, 4, 4))                      # input's channels
    with pytest.raises(RuntimeError, match="residual must be"):
        _fused(res=_cl(1, 128, 4, 4, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="residual must be"):
        _fused(res=torch.zeros(1, 128, 4, 4, dtype=torch.bfloat16))  # NCHW
    with pytest.raises(RuntimeError, match="residual must be"):
        _fused(res=_cl(1, 128, 4, 4), sy=2)               # output is 2x2 here
    # the kernels read coefficients and residual as 16-B vectors
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _fused(scale=_f32(129)[1:])
    off = torch.zeros(128 * 16 + 1, dtype=torch.bfloat16)[1:]
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _fused(res=off.view(1, 4, 4, 128).permute(0, 3, 1, 2))


def _stem(x8=None, wpad=None, scale=None, shift=None, P=4, Q=4):
    x8 = _cl(1, 8, 6, 14) if x8 is None else x8
    wpad = (torch.zeros(64, 3, 64, dtype=torch.bfloat16)
            if wpad is None else wpad)
    scale = _f32(64) if scale is None else scale
    shift = _f32(64) if shift is None else shift
    return C.conv_stem_fwd_fused(x8, wpad, scale, shift, True, 3, 1, 1, P, Q)


@cpu_only
def test_fused_stem_refusals():
    with pytest.raises(RuntimeError, match="device tensors required"):
        _stem()
    with pytest.raises(RuntimeError, match="wpad must be"):
        _stem(wpad=torch.zeros(64, 3, 32, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="x8 must be"):
        _stem(x8=_cl(1, 3, 6, 14))
    with pytest.raises(RuntimeError, match="reads outside"):
        _stem(P=5)
    with pytest.raises(RuntimeError, match="scale must be contiguous"):
        _stem(scale=_f32(8))
    with pytest.raises(RuntimeError, match="shift must be contiguous"):
        _stem(shift=torch.zeros(64, dtype=torch.float64))


def _fold(n=2, arena=None, max_c=64, **bad):
    t = dict(w_ptrs=torch.zeros(n, dtype=torch.long),
             b_ptrs=torch.zeros(n, dtype=torch.long),
             rm_ptrs=torch.zeros(n, dtype=torch.long),
             rv_ptrs=torch.zeros(n, dtype=torch.long),
             Cs=torch.full((n,), 64, dtype=torch.int32),
             offs=torch.arange(n, dtype=torch.long) * 128,
             eps=torch.full((n,), 1e-5, dtype=torch.float32))
    t.update(bad)
    arena = _f32(128 * n) if arena is None else arena
    return C.bn_fold_eval_batch(t["w_ptrs"], t["b_ptrs"], t["rm_ptrs"],
                                t["rv_ptrs"], t["Cs"], t["offs"], t["eps"],
                                arena, max_c)


@cpu_only
def test_fold_refusals():
    with pytest.raises(RuntimeError, match="device tensors required"):
        _fold()
    with pytest.raises(RuntimeError, match="layers"):
        _fold(n=0, arena=_f32(128))
    with pytest.raises(RuntimeError, match="b_ptrs must be contiguous"):
        _fold(b_ptrs=torch.zeros(3, dtype=torch.long))
    with pytest.raises(RuntimeError, match="rv_ptrs must be contiguous"):
        _fold(rv_ptrs=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="Cs must be contiguous"):
        _fold(Cs=torch.full((2,), 64, dtype=torch.long))
    with pytest.raises(RuntimeError, match="offs must be contiguous"):
        _fold(offs=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="eps must be contiguous"):
        _fold(eps=torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="arena must be"):
        _fold(arena=torch.zeros(256, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="max_c"):
        _fold(max_c=0)
    with pytest.raises(RuntimeError, match="max_c"):
        _fold(max_c=4096)
