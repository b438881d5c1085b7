"""The fused inference path on the GPU: conv + eval BN + residual + ReLU in
the conv epilogue, on every tile / ring / split-K / stem path.

Full-epilogue bound (per element, fp64 oracle from the bf16-rounded inputs):

    |got - ref| <= 2^-8 |ref| + 2 gamma,  gamma = (R S C + 3) 2^-24 A,
    A = conv(|x|, |w|) |scale| + |shift| + |residual|

2^-8 is bf16's unit roundoff for the single store; gamma is the standard
worst-case bound of an fp32 accumulation of R S C products plus the three
epilogue operations; the second gamma is margin for the MFMA's internal
summation order. A two-pass implementation (bf16 conv output, then BN)
exceeds this bound on the shallow-K shapes.
"""

import copy
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from fluxdistributed_amd.inference import compile_for_inference
from fluxdistributed_amd.models import build_model
from fluxdistributed_amd.models.resnet import FusedBNAct
from fluxdistributed_amd.ops.native import load_native
from fluxdistributed_amd.utils.precision import to_mixed_bf16

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CL = torch.channels_last

# (N, C, H, W, K, R, stride) -> (BM, BN, SK, ring) the shape must reach
BODY = {
    (2, 64, 9, 11, 64, 3, 1): (256, 64, 1, False),     # ragged M
    (2, 64, 9, 11, 128, 3, 2): (128, 128, 1, False),   # stride 2
    (2, 256, 13, 13, 64, 1, 2): (256, 64, 1, False),   # 1x1 s2, odd spatial
    (2, 512, 7, 7, 512, 3, 1): (128, 128, 4, False),   # split-K combine
    (48, 64, 56, 56, 64, 3, 1): (256, 64, 1, True),    # 256x64 BK32 ring
    (96, 128, 28, 28, 128, 3, 1): (128, 128, 1, True),  # 128x128 BK32 ring
}
STEM = [(2, 3, 32, 32, 64, 7, 2), (2, 3, 16, 16, 64, 3, 1)]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _out_hw(H, W, R, stride):
    pad = R // 2
    return ((H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1)


def _coeffs(K, g):
    """|scale| in [0.25, 1.75], about a quarter negative; shift ~ N(0, 0.5)."""
    scale = 0.25 + 1.5 * torch.rand(K, device=DEV, generator=g)
    scale = torch.where(torch.rand(K, device=DEV, generator=g) < 0.25,
                        -scale, scale)
    shift = 0.5 * torch.randn(K, device=DEV, generator=g)
    return scale.contiguous(), shift.contiguous()


def _conv64(x, w, stride, pad):
    """fp64 conv as unfold + matmul (independent of the kernels under test)."""
    N, K, R = x.shape[0], w.shape[0], w.shape[2]
    P = (x.shape[2] + 2 * pad - R) // stride + 1
    Q = (x.shape[3] + 2 * pad - R) // stride + 1
    cols = F.unfold(x.double(), R, padding=pad, stride=stride)
    return (w.double().reshape(K, -1) @ cols).view(N, K, P, Q)


class Case:
    """Inputs and the fp64 pieces of the oracle for one shape, made once."""

    def __init__(self, shape, stem):
        N, C, H, W, K, R, stride = shape
        g = _gen(sum(shape))
        self.shape, self.stem, self.pad = shape, stem, R // 2
        self.x = torch.randn(N, C, H, W, device=DEV, generator=g).bfloat16() \
            .contiguous(memory_format=CL)
        self.w = (torch.randn(K, C, R, R, device=DEV, generator=g)
                  / (R * R * C) ** 0.5).bfloat16().contiguous(memory_format=CL)
        self.P, self.Q = _out_hw(H, W, R, stride)
        self.res = torch.randn(N, K, self.P, self.Q, device=DEV, generator=g) \
            .bfloat16().contiguous(memory_format=CL)
        self.scale, self.shift = _coeffs(K, g)
        self.conv = _conv64(self.x, self.w, stride, self.pad)
        self.conv_abs = _conv64(self.x.abs(), self.w.abs(), stride, self.pad)
        if stem:
            # operands of the stem kernel, as ops/conv.py builds them
            py = self.pad
            x8 = torch.zeros(N, 8, H + 2 * py, W + 2 * py + 8, device=DEV,
                             dtype=torch.bfloat16).contiguous(memory_format=CL)
            x8[:, :C, py:py + H, py:py + W] = self.x
            wpad = torch.zeros(K, R, 64, dtype=torch.bfloat16, device=DEV)
            wpad.view(K, R, 8, 8)[:, :, :R, :C] = self.w.permute(0, 2, 3, 1)
            self.x8, self.wpad = x8, wpad

    def plain(self, C_):
        N, C, H, W, K, R, s = self.shape
        if self.stem:
            return C_.conv_stem_fwd(self.x8, self.wpad, R, s, s, self.P, self.Q)
        return C_.conv_igemm_fwd(self.x, self.w, s, s, self.pad, self.pad)

    def fused(self, C_, scale, shift, res, relu):
        N, C, H, W, K, R, s = self.shape
        if self.stem:
            assert res is None
            return C_.conv_stem_fwd_fused(self.x8, self.wpad, scale, shift,
                                          relu, R, s, s, self.P, self.Q)
        if res is None:
            res = torch.empty(0, device=DEV, dtype=torch.bfloat16)
        return C_.conv_igemm_fwd_fused(self.x, self.w, scale, shift, res,
                                       relu, s, s, self.pad, self.pad)


_CASES = {}


def case(shape, stem=False):
    key = (shape, stem)
    if key not in _CASES:
        _CASES[key] = Case(shape, stem)
    return _CASES[key]


@pytest.fixture(scope="module")
def C_():
    C = load_native()
    assert C is not None, "native extension not built"
    return C


ALL = [(s, False) for s in BODY] + [(s, True) for s in STEM]
IDS = ["x".join(map(str, s)) + ("-stem" if st else "") for s, st in ALL]


@pytest.mark.parametrize("shape", list(BODY), ids=IDS[:len(BODY)])
def test_shape_reaches_its_config(C_, shape):
    N, C, H, W, K, R, stride = shape
    P, Q = _out_hw(H, W, R, stride)
    got = tuple(C_.conv_igemm_fwd_config(N * P * Q, C, K, R, R))
    assert got == BODY[shape]


@pytest.mark.parametrize("shape,stem", ALL, ids=IDS)
def test_identity_epilogue_is_bit_equal(C_, shape, stem):
    c = case(shape, stem)
    K = shape[4]
    one = torch.ones(K, device=DEV)
    zero = torch.zeros(K, device=DEV)
    got = c.fused(C_, one, zero, None, False)
    ref = c.plain(C_)
    assert got.shape == ref.shape and got.is_contiguous(memory_format=CL)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


# {residual on/off} x {ReLU on/off}; the stem binding has no residual operand
FULL = [(s, st, res, relu) for s, st in ALL for res in (False, True)
        for relu in (False, True) if not (st and res)]
FULL_IDS = ["x".join(map(str, s)) + ("-stem" if st else "")
            + ("-res" if res else "-nores") + ("-relu" if relu else "-lin")
            for s, st, res, relu in FULL]


@pytest.mark.parametrize("shape,stem,with_res,relu", FULL, ids=FULL_IDS)
def test_full_epilogue_within_single_rounding_bound(C_, shape, stem, with_res,
                                                    relu):
    c = case(shape, stem)
    N, C, H, W, K, R, stride = shape
    got = c.fused(C_, c.scale, c.shift, c.res if with_res else None, relu)
    sc = c.scale.double().view(1, K, 1, 1)
    sh = c.shift.double().view(1, K, 1, 1)
    pre = c.conv * sc + sh
    A = c.conv_abs * sc.abs() + sh.abs()
    if with_res:
        pre = pre + c.res.double()
        A = A + c.res.double().abs()
    ref = pre.clamp_min(0) if relu else pre
    gamma = (R * R * C + 3) * 2.0 ** -24 * A
    bound = 2.0 ** -8 * ref.abs() + 2 * gamma
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    neg = float((pre < 0).double().mean())
    print(f"infer_fused shape={shape} stem={stem} res={with_res} relu={relu} "
          f"worst err/bound={ratio:.3f} neg_frac={neg:.3f}")
    assert bool((err <= bound).all()), f"worst err/bound = {ratio:.3f}"


def test_fold_matches_eval_finalize_bit_for_bit(C_):
    """Through an identity 1x1 conv the fused output is bf16(fma(x, scale,
    shift)), exactly what bn_act_fwd(eval) stores for the same x, if and
    only if the batched fold produced bn_eval_finalize's coefficients."""
    g = _gen(5)
    Cs = [64, 128]
    bns = []
    for n in Cs:
        sc, bias = _coeffs(n, g)
        bns.append((sc, bias, 0.5 * torch.randn(n, device=DEV, generator=g),
                    0.5 + 1.5 * torch.rand(n, device=DEV, generator=g)))
    offs = [0, 2 * Cs[0]]
    arena = torch.full((2 * sum(Cs),), float("nan"), device=DEV)
    mk = lambda v, dt: torch.tensor(v, dtype=dt, device=DEV)
    C_.bn_fold_eval_batch(
        *(mk([b[i].data_ptr() for b in bns], torch.long) for i in range(4)),
        mk(Cs, torch.int32), mk(offs, torch.long),
        mk([1e-5, 1e-3], torch.float32), arena, max(Cs))
    for n, off, eps, (w, b, rm, rv) in zip(Cs, offs, [1e-5, 1e-3], bns):
        x = torch.randn(2, n, 5, 7, device=DEV, generator=g).bfloat16() \
            .contiguous(memory_format=CL)
        eye = torch.eye(n, device=DEV).bfloat16().view(n, n, 1, 1) \
            .contiguous(memory_format=CL)
        got = C_.conv_igemm_fwd_fused(
            x, eye, arena[off:off + n], arena[off + n:off + 2 * n],
            torch.empty(0, device=DEV, dtype=torch.bfloat16), True, 1, 1, 0, 0)
        ref = C_.bn_act_fwd(x, w, b, rm, rv, False, 0.1, eps, True,
                            torch.empty(0, device=DEV, dtype=torch.bfloat16))[0]
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


# ---- whole model -------------------------------------------------------------

def _randomize_bn(model, seed=1):
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


def _models(name):
    torch.manual_seed(0)
    cpu = _randomize_bn(build_model(name, num_classes=10, small_input=True))
    cpu.eval()
    gpu = to_mixed_bf16(copy.deepcopy(cpu).to(DEV).to(memory_format=CL)).eval()
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(3))
    xg = x.to(DEV).bfloat16().contiguous(memory_format=CL)
    return cpu, gpu, x, xg


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_whole_model_against_cpu_oracle(name):
    cpu, gpu, x, xg = _models(name)
    with torch.no_grad():
        oracle = cpu(x)
        unfused = gpu(xg).float().cpu()
    im = compile_for_inference(gpu)
    fused = im(xg).float().cpu()
    e_fused = float((fused - oracle).abs().max())
    e_unfused = float((unfused - oracle).abs().max())
    print(f"infer_fused model={name} E_fused={e_fused:.5g} "
          f"E_unfused={e_unfused:.5g} logit_scale={float(oracle.abs().max()):.4g}")
    assert e_fused <= 2 * e_unfused
    top2 = oracle.topk(2, dim=1).values
    margin = top2[:, 0] - top2[:, 1]
    sure = margin > 2 * e_unfused
    assert torch.equal(fused.argmax(1)[sure], oracle.argmax(1)[sure])


def test_graph_replay_matches_eager():
    _, gpu, _, xg = _models("resnet18")
    im = compile_for_inference(gpu)
    replay = im.capture(xg)
    x2 = torch.randn(4, 3, 32, 32, device=DEV, generator=_gen(11)).bfloat16() \
        .contiguous(memory_format=CL)
    for inp in (xg, x2):
        assert torch.equal(replay(inp), im(inp))
    before = im(xg).clone()
    with torch.no_grad():
        gpu.layer2[0].bn1.running_mean.add_(0.5)
        gpu.bn1.running_var.mul_(1.5)
    after = im(xg)
    assert not torch.equal(after, before)
    assert torch.equal(replay(xg), after)


_KNOB_CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
from fluxdistributed_amd.inference import compile_for_inference
from fluxdistributed_amd.models import build_model
from fluxdistributed_amd.models.resnet import FusedBNAct
from fluxdistributed_amd.utils.precision import to_mixed_bf16
torch.manual_seed(0)
m = build_model("resnet18", num_classes=10, small_input=True)
for bn in m.modules():
    if isinstance(bn, FusedBNAct):
        with torch.no_grad():
            bn.weight.uniform_(0.25, 1.75)
            bn.bias.normal_(0, 0.5)
            bn.running_mean.normal_(0, 0.5)
            bn.running_var.uniform_(0.5, 2.0)
m = to_mixed_bf16(m.to("cuda:0").to(memory_format=torch.channels_last)).eval()
x = torch.randn(4, 3, 32, 32, device="cuda:0").bfloat16().contiguous(
    memory_format=torch.channels_last)
with torch.no_grad():
    ref = m(x)
out = compile_for_inference(m)(x)
torch.cuda.synchronize()
assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), "differs"
print("KNOB_OK")
"""


def test_knob_off_is_bit_equal_to_eval():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FLUXDIST_INFER_FUSE="0")
    r = subprocess.run([sys.executable, "-c", _KNOB_CHILD.format(root=root)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "KNOB_OK" in r.stdout, r.stdout + r.stderr
