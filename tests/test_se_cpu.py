"""Squeeze-and-excitation without a GPU: the bindings' refusals, the torch
composition against the float64 formula, and the SE models."""

import pytest
import torch

from fluxdistributed_amd.inference import compile_for_inference
from fluxdistributed_amd.models import build_model
from fluxdistributed_amd.models.resnet import FusedBNAct, SqueezeExcite
from fluxdistributed_amd.ops.native import load_native
from fluxdistributed_amd.ops.se import se_scale_add_relu
from fluxdistributed_amd.utils.precision import to_mixed_bf16

C = load_native()
needs_cpu_ext = pytest.mark.skipif(
    C is None or torch.cuda.is_available(),
    reason="CPU-only with the extension built: must never reach a launch")

BF, F32 = torch.bfloat16, torch.float32


def _operands(C_=64, Cr=4, N=1, H=2, W=2, dtype=BF):
    cl = torch.channels_last
    act = lambda: torch.zeros(N, C_, H, W, dtype=dtype).contiguous(  # noqa: E731
        memory_format=cl)
    return dict(u=act(), identity=act(), gout=act(), out=act(),
                w1=torch.zeros(Cr, C_, dtype=dtype),
                b1=torch.zeros(Cr, dtype=dtype),
                w2=torch.zeros(C_, Cr, dtype=dtype),
                b2=torch.zeros(C_, dtype=dtype),
                s=torch.zeros(N, C_), h=torch.zeros(N, Cr),
                z=torch.zeros(N, C_))


def _call(entry, o):
    if entry == "se_fwd":
        return C.se_fwd(o["u"], o["identity"], o["w1"], o["b1"], o["w2"],
                        o["b2"])
    return C.se_bwd(o["gout"], o["out"], o["u"], o["s"], o["h"], o["z"],
                    o["w1"], o["w2"])


# operand to replace -> (replacement, message), every other one the smallest
# valid; all refusals come before the device check
BAD_ACT = torch.zeros(1, 64, 2, 3, dtype=BF).contiguous(
    memory_format=torch.channels_last)
REFUSALS = {
    "se_fwd": {
        "u_fp32": (dict(u=_operands(dtype=F32)["u"]), "channels_last bf16"),
        "u_nchw": (dict(u=torch.zeros(1, 64, 2, 2, dtype=BF)),
                   "channels_last bf16"),
        "identity_shape": (dict(identity=BAD_ACT), "identity must match u"),
        "b1_len": (dict(b1=torch.zeros(8, dtype=BF)), "b1 must be"),
        "b2_fp32": (dict(b2=torch.zeros(64)), "b2 must be"),
    },
    "se_bwd": {
        "gout_shape": (dict(gout=BAD_ACT), "gout must match u"),
        "out_shape": (dict(out=BAD_ACT), "out must match u"),
        "s_bf16": (dict(s=torch.zeros(1, 64, dtype=BF)), "s must be"),
        "h_len": (dict(h=torch.zeros(1, 8)), "h must be"),
        "z_len": (dict(z=torch.zeros(2, 64)), "z must be"),
    },
    "both": {
        "c32": (_operands(C_=32), "C must be a multiple of 64"),
        "c4096": (_operands(C_=4096, Cr=128), "C must be a multiple of 64"),
        "cr6": (_operands(Cr=6), "Cr must be a multiple of 4"),
        "cr256": (_operands(C_=2048, Cr=256), "Cr must be a multiple of 4"),
        "w1_shape": (dict(w1=torch.zeros(4, 128, dtype=BF)), "need w1"),
        "w2_shape": (dict(w2=torch.zeros(64, 8, dtype=BF)), "need w1"),
        "w1_fp32": (dict(w1=torch.zeros(4, 64)), "w1 must be"),
        "w2_strided": (dict(w2=torch.zeros(4, 64, dtype=BF).t()),
                       "w2 must be"),
        "w1_1d": (dict(w1=torch.zeros(256, dtype=BF)), "must be 2-D"),
        "valid": (dict(), "device tensors required"),
    },
}
CASES = [(e, k) for e in ("se_fwd", "se_bwd")
         for k in sorted({**REFUSALS[e], **REFUSALS["both"]})]


@needs_cpu_ext
@pytest.mark.parametrize("entry,case", CASES)
def test_binding_refuses(entry, case):
    repl, msg = {**REFUSALS[entry], **REFUSALS["both"]}[case]
    with pytest.raises(RuntimeError, match=msg):
        _call(entry, {**_operands(), **repl})


@needs_cpu_ext
def test_se_config_refuses_and_plans():
    with pytest.raises(RuntimeError, match="C must be"):
        C.se_config(2, 49, 96, 4)
    with pytest.raises(RuntimeError, match="Cr must be"):
        C.se_config(2, 49, 64, 2)
    assert C.se_config(2, 200, 64, 4) == (3, 67, 2)
    assert C.se_config(1, 4, 2048, 128) == (2, 2, 1)


def test_composition_matches_float64_formula():
    gen = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    ops = [r(3, 32, 5, 4), r(3, 32, 5, 4), r(2, 32), r(2), r(32, 2), r(32)]
    g = r(3, 32, 5, 4)

    def run(dtype, fn):
        leaves = [t.to(dtype).requires_grad_(True) for t in ops]
        out = fn(*leaves)
        return [out.detach()] + list(torch.autograd.grad(out, leaves,
                                                         g.to(dtype)))

    def formula(u, idn, w1, b1, w2, b2):
        z = u.sum((2, 3)) / (u.shape[2] * u.shape[3])
        h = (z @ w1.T + b1).clamp_min(0)
        s = 1 / (1 + torch.exp(-(h @ w2.T + b2)))
        return (u * s[:, :, None, None] + idn).clamp_min(0)

    # fp32 composition (C = 32: no native path anywhere) vs float64
    for got, ref in zip(run(F32, se_scale_add_relu),
                        run(torch.float64, formula)):
        assert torch.allclose(got.double(), ref, rtol=1e-5, atol=1e-5)


def test_parameter_counts():
    count = lambda n: sum(p.numel() for p in build_model(n).parameters())  # noqa: E731
    se = sum(nb * (2 * c * c // 16 + c // 16 + c)
             for nb, c in ((3, 256), (4, 512), (6, 1024), (3, 2048)))
    assert se == 2530992
    assert count("se_resnet50") == 25557032 + se == 28088024
    assert count("se_resnext50_32x4d") == 25028904 + se == 27559896


def test_existing_models_keep_their_keys_and_se_models_add_theirs():
    plain = build_model("resnet18", num_classes=10, small_input=True)
    se = build_model("se_resnet18", num_classes=10, small_input=True)
    keys = list(plain.state_dict())
    assert not any(".se." in k for k in keys)
    extra = [k for k in se.state_dict() if k not in keys]
    assert len(extra) == 8 * 4 and all(".se." in k for k in extra)
    assert [k for k in se.state_dict() if ".se." not in k] == keys
    # default Linear initialisation: bounded by 1/sqrt(fan_in), not N(0, .01)
    m = se.layer4[0].se
    assert float(m.w1.abs().max()) <= 512 ** -0.5
    assert float(m.w1.std()) > 0.02 and float(m.b2.abs().max()) > 0


def test_mixed_bf16_and_inference_on_se_model():
    torch.manual_seed(0)
    model = build_model("se_resnext50_32x4d", num_classes=8, small_input=True)
    x = torch.randn(2, 3, 16, 16)
    model.eval()
    assert torch.equal(compile_for_inference(model)(x), model(x))
    to_mixed_bf16(model)
    for m in model.modules():
        if isinstance(m, SqueezeExcite):
            assert all(p.dtype == BF for p in m.parameters())
        if isinstance(m, FusedBNAct):
            assert all(p.dtype == F32 for p in m.parameters())
