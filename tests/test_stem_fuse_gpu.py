"""Fused stem tail (BN + ReLU + max-pool), ReLU mask recomputed from x in the
generic BN backward, and the wide reduce/finalize.

Oracles: the fp32 PyTorch composition, and the project's own unfused chain
(whose rounding and tie rule the fused kernels reproduce). Tolerances are the
ones tests/test_ops_gpu.py uses for the same ops."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("GPU-only suite", allow_module_level=True)

DEV = "cuda:0"

# (dtype, forward tol, backward tol) — test_bn_act_fwd / test_bn_act_bwd
DTYPES = [(torch.float32, 1e-4, 1e-3), (torch.bfloat16, 3e-2, 5e-2)]

POOL_CASES = [
    ((2, 64, 9, 9), 3, 2, 1),     # odd size, every border case
    ((2, 64, 10, 10), 3, 2, 1),
    ((1, 128, 7, 5), 3, 2, 1),    # non-square, C > 64
    ((3, 64, 8, 11), 3, 2, 1),
    ((2, 64, 10, 10), 2, 2, 0),   # non-overlapping windows
]


def _native():
    from fluxdistributed_amd.ops.native import load_native

    mod = load_native()
    assert mod is not None, "native extension must be present on GPU box"
    return mod


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _tie_free(shape, dtype):
    """Every (image, channel) plane is a random permutation of consecutive
    integers centred on zero: exact in bf16, and after BN with weight in
    [1, 1.5] neighbouring activations differ by more than one bf16 ulp, so
    rounding cannot create a tie inside a pool window."""
    n, c, h, w = shape
    hw = h * w
    planes = torch.stack([torch.randperm(hw) for _ in range(n * c)])
    x = (planes - hw // 2).float().view(n, c, h, w)
    return _cl(x.to(DEV, dtype))


def _params(c):
    w = torch.rand(c, device=DEV) * 0.5 + 1.0
    b = torch.rand(c, device=DEV) - 0.5
    rm = torch.randn(c, device=DEV) * 0.1
    rv = torch.rand(c, device=DEV) + 0.5
    return w, b, rm, rv


def _close(a, b, tol, atol=None):
    atol = tol if atol is None else atol
    return torch.allclose(a, b, rtol=tol, atol=atol)


# --------------------------------------------------------------------------
# 1. fused stem tail vs the fp32 PyTorch composition
# --------------------------------------------------------------------------


@pytest.mark.parametrize("dtype,ftol,btol", DTYPES)
@pytest.mark.parametrize("shape,k,s,p", POOL_CASES)
def test_fused_pool_vs_fp32_oracle(dtype, ftol, btol, shape, k, s, p, seed):
    from fluxdistributed_amd.ops.functional import batch_norm_act_pool

    c = shape[1]
    x = _tie_free(shape, dtype).requires_grad_()
    w, b, rm, rv = _params(c)
    w.requires_grad_()
    b.requires_grad_()
    rm2, rv2 = rm.clone(), rv.clone()

    out = batch_norm_act_pool(x, w, b, rm, rv, True, 0.1, 1e-5, k, s, p)
    gout = _cl(torch.randn_like(out))
    out.backward(gout)

    xr = x.detach().float().requires_grad_()
    wr = w.detach().clone().requires_grad_()
    br = b.detach().clone().requires_grad_()
    ref = F.max_pool2d(
        torch.relu(F.batch_norm(xr, rm2, rv2, wr, br, True, 0.1, 1e-5)),
        k, s, p)
    ref.backward(gout.float())

    assert out.shape == ref.shape
    assert _close(out.float(), ref, ftol), (out.float() - ref).abs().max()
    assert torch.allclose(rm, rm2, rtol=1e-4, atol=1e-5)
    assert torch.allclose(rv, rv2, rtol=1e-4, atol=1e-4)
    assert _close(x.grad.float(), xr.grad, btol), \
        (x.grad.float() - xr.grad).abs().max()
    assert _close(w.grad, wr.grad, btol, btol * 10), (w.grad - wr.grad).abs().max()
    assert _close(b.grad, br.grad, btol, btol * 10), (b.grad - br.grad).abs().max()


def test_fused_pool_eval_mode_vs_fp32_oracle(seed):
    from fluxdistributed_amd.ops.functional import batch_norm_act_pool

    shape, dtype = (2, 64, 9, 9), torch.bfloat16
    x = _tie_free(shape, dtype)
    w, b, rm, rv = _params(64)
    # put the running stats where the planes' own stats are, so activations
    # stay in the tie-free range
    rm = x.float().mean(dim=(0, 2, 3))
    rv = x.float().var(dim=(0, 2, 3), unbiased=False)
    rm2, rv2 = rm.clone(), rv.clone()
    out = batch_norm_act_pool(x, w, b, rm, rv, False, 0.1, 1e-5, 3, 2, 1)
    ref = F.max_pool2d(
        torch.relu(F.batch_norm(x.float(), rm2, rv2, w, b, False, 0.1, 1e-5)),
        3, 2, 1)
    assert _close(out.float(), ref, 3e-2), (out.float() - ref).abs().max()
    assert torch.equal(rm, rm2) and torch.equal(rv, rv2)


# --------------------------------------------------------------------------
# 2. fused vs the project's unfused chain (same rounding, same tie rule)
# --------------------------------------------------------------------------


def _fused_and_chain(C, x, w, b, k, s, p, gout):
    c = x.shape[1]
    h, wd = x.shape[2], x.shape[3]
    empty = torch.empty(0, device=DEV, dtype=x.dtype)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    act, mean, invstd = C.bn_act_fwd(x, w, b, rm, rv, True, 0.1, 1e-5, True,
                                     empty)
    pooled, idx = C.maxpool_fwd(act, k, k, s, p)
    gpool = C.maxpool_bwd(gout, idx, h, wd, k, k, s, p)
    gx, gw, gb, _ = C.bn_act_bwd(gpool, x, w, mean, invstd, act, True, True)

    rm_f, rv_f = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    pooled_f, idx_f, mean_f, invstd_f = C.bn_act_pool_fwd(
        x, w, b, rm_f, rv_f, True, 0.1, 1e-5, k, k, s, p)
    gx_f, gw_f, gb_f = C.bn_act_pool_bwd(gout, x, w, b, mean_f, invstd_f,
                                         idx_f, k, k, s, p, True)
    assert torch.equal(rm, rm_f) and torch.equal(rv, rv_f)
    assert torch.equal(mean, mean_f) and torch.equal(invstd, invstd_f)
    return (pooled, idx, gx, gw, gb), (pooled_f, idx_f, gx_f, gw_f, gb_f)


@pytest.mark.parametrize("dtype,ftol,btol", DTYPES)
@pytest.mark.parametrize("shape,k,s,p,ties", [
    (sh, k, s, p, False) for sh, k, s, p in POOL_CASES
] + [
    ((2, 64, 33, 33), 3, 2, 1, True),    # randn: rounding ties, >1 block/row
    # N*H = 1120 > the backward stats pass's 1024-block cap: each block
    # walks two input rows and the finalize folds its rows in two batches
    # (the path the 96 x 112 stem takes)
    ((40, 64, 28, 28), 3, 2, 1, True),
])
def test_fused_pool_vs_unfused_chain(dtype, ftol, btol, shape, k, s, p, ties,
                                     seed):
    C = _native()
    if ties:
        x = _cl(torch.randn(*shape, device=DEV, dtype=dtype))
    else:
        x = _tie_free(shape, dtype)
    w, b, _, _ = _params(shape[1])
    ho = (shape[2] + 2 * p - k) // s + 1
    wo = (shape[3] + 2 * p - k) // s + 1
    gout = _cl(torch.randn(shape[0], shape[1], ho, wo, device=DEV, dtype=dtype))
    (po, io, gx, gw, gb), (pf, if_, gxf, gwf, gbf) = _fused_and_chain(
        C, x, w, b, k, s, p, gout)
    # identical expression, rounding and scan order: equal, ties included
    n_out = int((po != pf).sum())
    n_idx = int((io != if_).sum())
    print(f"differing pooled={n_out} argmax={n_idx} of {po.numel()}")
    assert n_out == 0 and n_idx == 0
    assert _close(gxf.float(), gx.float(), btol), \
        (gxf.float() - gx.float()).abs().max()
    assert _close(gwf, gw, btol, btol * 10)
    assert _close(gbf, gb, btol, btol * 10)


# --------------------------------------------------------------------------
# 3. generic BN backward: mask from x (bias given) vs mask from `out`
# --------------------------------------------------------------------------


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3),
                                       (torch.bfloat16, 5e-2)])
@pytest.mark.parametrize("Cc", [64, 256])
def test_bn_bwd_mask_from_x(dtype, tol, Cc, seed):
    C = _native()
    N, H, W = 4, 9, 9
    x = _cl(torch.randn(N, Cc, H, W, device=DEV, dtype=dtype))
    w = torch.rand(Cc, device=DEV) + 0.5
    b = torch.randn(Cc, device=DEV)
    rm, rv = torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV)
    out, mean, invstd = C.bn_act_fwd(x, w, b, rm, rv, True, 0.1, 1e-5, True,
                                     torch.empty(0, device=DEV, dtype=dtype))
    gout = _cl(torch.randn_like(x))
    gx0, gw0, gb0, _ = C.bn_act_bwd(gout, x, w, mean, invstd, out, True, True)
    # `out` poisoned: the bias variant must not depend on it
    poison = torch.full_like(out, -1.0)
    gx1, gw1, gb1, _ = C.bn_act_bwd(gout, x, w, mean, invstd, poison, True,
                                    True, None, None, False, b)

    xr = x.float().detach().requires_grad_()
    wr = w.detach().requires_grad_()
    br = b.detach().requires_grad_()
    ref = torch.relu(F.batch_norm(xr, torch.zeros(Cc, device=DEV),
                                  torch.ones(Cc, device=DEV), wr, br, True,
                                  0.1, 1e-5))
    ref.backward(gout.float())
    for gx, gw, gb in ((gx0, gw0, gb0), (gx1, gw1, gb1)):
        assert _close(gx.float(), xr.grad, tol), (gx.float() - xr.grad).abs().max()
        assert _close(gw, wr.grad, tol, tol * 10)
        assert _close(gb, br.grad, tol, tol * 10)
    assert torch.equal(gx0, gx1)
    assert torch.equal(gw0, gw1) and torch.equal(gb0, gb1)


def test_bn_bwd_residual_keeps_reading_out(seed):
    """want_gres (residual ReLU BN): bias is ignored, the mask is `out`'s."""
    C = _native()
    dtype = torch.bfloat16
    x = _cl(torch.randn(4, 64, 9, 9, device=DEV, dtype=dtype))
    res = _cl(torch.randn_like(x))
    w = torch.rand(64, device=DEV) + 0.5
    b = torch.randn(64, device=DEV)
    rm, rv = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
    out, mean, invstd = C.bn_act_fwd(x, w, b, rm, rv, True, 0.1, 1e-5, True, res)
    gout = _cl(torch.randn_like(x))
    a = C.bn_act_bwd(gout, x, w, mean, invstd, out, True, True, None, None, True)
    c = C.bn_act_bwd(gout, x, w, mean, invstd, out, True, True, None, None,
                     True, b)
    for t0, t1 in zip(a, c):
        assert torch.equal(t0, t1)


# --------------------------------------------------------------------------
# 4. wide reduce/finalize: forward and backward statistics
# --------------------------------------------------------------------------

FIN_SHAPES = [
    (4, 64, 7, 7),
    (4, 512, 7, 7),
    (2, 2048, 3, 3),      # chunked path (fp32: two channel chunks)
    (64, 64, 33, 33),     # 512 partial rows: the stats grid cap
]


@pytest.mark.parametrize("dtype,ftol,btol", DTYPES)
@pytest.mark.parametrize("shape", FIN_SHAPES)
def test_finalize_stats_vs_fp32_oracle(dtype, ftol, btol, shape, seed):
    C = _native()
    Cc = shape[1]
    x = _cl(torch.randn(*shape, device=DEV, dtype=dtype))
    w = torch.rand(Cc, device=DEV) + 0.5
    b = torch.randn(Cc, device=DEV)
    rm = torch.randn(Cc, device=DEV) * 0.1
    rv = torch.rand(Cc, device=DEV) + 0.5
    rm2, rv2 = rm.clone(), rv.clone()
    out, mean, invstd = C.bn_act_fwd(x, w, b, rm, rv, True, 0.1, 1e-5, True,
                                     torch.empty(0, device=DEV, dtype=dtype))
    gout = _cl(torch.randn_like(x))
    gx, gw, gb, _ = C.bn_act_bwd(gout, x, w, mean, invstd, out, True, True)
    # accum semantics: += into caller-owned slices
    gw_acc = torch.full((Cc,), 2.0, device=DEV)
    gb_acc = torch.full((Cc,), -3.0, device=DEV)
    C.bn_act_bwd(gout, x, w, mean, invstd, out, True, True, gw_acc, gb_acc)

    xr = x.float().detach().requires_grad_()
    wr = w.detach().requires_grad_()
    br = b.detach().requires_grad_()
    ref = torch.relu(F.batch_norm(xr, rm2, rv2, wr, br, True, 0.1, 1e-5))
    ref.backward(gout.float())
    xf = x.float()
    assert torch.allclose(mean, xf.mean(dim=(0, 2, 3)), rtol=1e-4, atol=1e-5)
    var = xf.var(dim=(0, 2, 3), unbiased=False)
    assert torch.allclose(invstd, torch.rsqrt(var + 1e-5), rtol=1e-4, atol=1e-5)
    assert _close(out.float(), ref, ftol), (out.float() - ref).abs().max()
    assert torch.allclose(rm, rm2, rtol=1e-4, atol=1e-5)
    assert torch.allclose(rv, rv2, rtol=1e-4, atol=1e-4)
    assert _close(gx.float(), xr.grad, btol), (gx.float() - xr.grad).abs().max()
    assert _close(gw, wr.grad, btol, btol * 10), (gw - wr.grad).abs().max()
    assert _close(gb, br.grad, btol, btol * 10), (gb - br.grad).abs().max()
    assert torch.equal(gw_acc, gw + 2.0) and torch.equal(gb_acc, gb - 3.0)


@pytest.mark.parametrize("conv", [
    # (n, cin, h, w, cout, r, stride) — BN input is the conv's output
    (4, 64, 7, 7, 64, 3, 1),
    (4, 512, 7, 7, 512, 3, 1),
    (2, 512, 3, 3, 2048, 1, 1),
    # 69696 output rows: 273 or 545 m-tiles (256- or 128-row tiles), below
    # the 1024-row prefold threshold; 545 is two finalize batches
    (64, 64, 33, 33, 64, 3, 1),
    # 270400 output rows: at least 1057 m-tiles at either tile height, so
    # the prefold (NB2 = 256) runs ahead of the finalize
    (64, 64, 65, 65, 64, 3, 1),
])
def test_finalize_from_conv_partials_matches_own_stats(conv, monkeypatch):
    """test_bn_fusion_gpu's mechanism: the conv epilogue's partials through
    (prefold +) finalize against BN's own stats pass."""
    from fluxdistributed_amd.models.resnet import FusedBNAct
    from fluxdistributed_amd.ops.conv import fda_conv2d

    n, c, h, w, k, r, s = conv
    pad = r // 2
    torch.manual_seed(4)
    x = _cl(torch.randn(n, c, h, w).cuda().bfloat16())
    wt = _cl((torch.randn(k, c, r, r) * (c * r * r) ** -0.5).cuda().bfloat16()) \
        .requires_grad_(True)

    def run(fuse):
        monkeypatch.setenv("FLUXDIST_BN_FUSE", "1" if fuse else "0")
        torch.manual_seed(9)
        bn = FusedBNAct(k, relu=True).cuda().train()
        wt.grad = None
        out = bn(fda_conv2d(x, wt, (s, s), (pad, pad)))
        out.float().square().mean().backward()
        torch.cuda.synchronize()
        return (out.float(), bn.running_mean.clone(), bn.running_var.clone(),
                wt.grad.float().clone())

    out1, rm1, rv1, gw1 = run(True)
    out0, rm0, rv0, gw0 = run(False)
    assert torch.allclose(rm1, rm0, rtol=1e-3, atol=1e-4), (rm1 - rm0).abs().max()
    assert torch.allclose(rv1, rv0, rtol=1e-3, atol=1e-4), (rv1 - rv0).abs().max()
    assert torch.allclose(out1, out0, rtol=2e-2, atol=2e-3), (out1 - out0).abs().max()
    assert torch.allclose(gw1, gw0, rtol=2e-2, atol=2e-3), (gw1 - gw0).abs().max()


# --------------------------------------------------------------------------
# 5. end to end: resnet18, FLUXDIST_STEM_FUSE=0 vs 1
# --------------------------------------------------------------------------


def _resnet18_step(monkeypatch, fuse, x, y):
    import fluxdistributed_amd.models.resnet as resnet_mod
    from fluxdistributed_amd.models import build_model
    from fluxdistributed_amd.ops import logit_cross_entropy
    from fluxdistributed_amd.utils.precision import to_mixed_bf16

    monkeypatch.setenv("FLUXDIST_STEM_FUSE", "1" if fuse else "0")
    # count the fused op's calls: the knob must really switch the path
    calls = []
    real = resnet_mod.batch_norm_act_pool

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(resnet_mod, "batch_norm_act_pool", spy)
    torch.manual_seed(3)
    model = build_model("resnet18", num_classes=10).to(DEV)
    model = to_mixed_bf16(model.to(memory_format=torch.channels_last))
    model.train()
    loss = logit_cross_entropy(model(x), y)
    assert len(calls) == (1 if fuse else 0), (fuse, len(calls))
    loss.backward()
    grads = {n: p.grad.float().clone() for n, p in model.named_parameters()}
    rm = model.bn1.running_mean.clone()
    model.eval()
    with torch.no_grad():
        logits = model(x).float()
    torch.cuda.synchronize()
    return float(loss.detach()), grads, rm, logits


def test_resnet18_stem_fuse_knob(monkeypatch):
    torch.manual_seed(11)
    x = _cl(torch.randn(2, 3, 64, 64, device=DEV, dtype=torch.bfloat16))
    y = torch.randint(0, 10, (2,), device=DEV)
    loss0, g0, rm0, ev0 = _resnet18_step(monkeypatch, False, x, y)
    loss1, g1, rm1, ev1 = _resnet18_step(monkeypatch, True, x, y)
    assert abs(loss1 - loss0) <= 3e-2 * max(1.0, abs(loss0)), (loss0, loss1)
    assert torch.equal(rm0, rm1)
    assert g0.keys() == g1.keys()
    for name in g0:
        atol = 5e-1 if ".bn" in name or name.startswith("bn") else 5e-2
        assert torch.allclose(g1[name], g0[name], rtol=5e-2, atol=atol), \
            (name, float((g1[name] - g0[name]).abs().max()))
    assert _close(ev1, ev0, 3e-2), (ev1 - ev0).abs().max()
