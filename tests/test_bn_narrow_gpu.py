"""Training BatchNorm on channel counts that are multiples of 8 but not of 64
(bn_act_fwd / bn_act_bwd, bf16) against F.batch_norm in float64 on the CPU,
then residual, ReLU and autograd. 24 and 40 channels idle stats lanes and end
inside a 16-channel finalize block; 8 leaves that block half empty; 96 idles
lanes above 64 channels. Tolerances: those of tests/test_ops_gpu.py."""

import pytest
import torch
import torch.nn.functional as F

from fluxdistributed_amd.ops.native import load_native

pytestmark = pytest.mark.gpu

# 4x7x7 as in test_ops_gpu.py; 2x17x19 = 646 rows: more than one block and a
# multiple of no row-group count
EXTENTS = [(4, 7, 7), (2, 17, 19)]
CASES = [(C, relu, False) for C in (8, 24, 32, 40, 96)
         for relu in (True, False)] + [(40, True, True)]


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("extent", EXTENTS)
@pytest.mark.parametrize("C,relu,res", CASES)
def test_bn_narrow_fwd_bwd(C, relu, res, extent):
    N, H, W = extent
    gen = torch.Generator().manual_seed(C + N)
    x = torch.randn(N, C, H, W, generator=gen).bfloat16()
    r = torch.randn(N, C, H, W, generator=gen).bfloat16()
    gout = torch.randn(N, C, H, W, generator=gen).bfloat16()
    w = torch.rand(C, generator=gen) + 0.5
    b = torch.randn(C, generator=gen)
    rm0 = torch.randn(C, generator=gen) * 0.1
    rv0 = torch.rand(C, generator=gen) + 0.5

    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    br = b.double().requires_grad_(True)
    rm_ref, rv_ref = rm0.double(), rv0.double()
    ref = F.batch_norm(xr, rm_ref, rv_ref, wr, br, True, 0.1, 1e-5)
    if res:
        ref = ref + r.double()
    if relu:
        ref = torch.relu(ref)
    ref.backward(gout.double())

    nat = load_native()
    xg, gg = _cl(x).cuda(), _cl(gout).cuda()
    rg = _cl(r).cuda() if res else torch.empty(0).bfloat16().cuda()
    wg, bg, rm, rv = w.cuda(), b.cuda(), rm0.cuda(), rv0.cuda()
    out, mean, invstd = nat.bn_act_fwd(xg, wg, bg, rm, rv, True, 0.1, 1e-5,
                                       relu, rg)
    want_gres = res and relu
    gx, gw, gb, gres = nat.bn_act_bwd(gg, xg, wg, mean, invstd, out, relu,
                                      True, None, None, want_gres, bg)

    def close(got, want, rtol, atol):
        got, want = got.double().cpu(), want.detach()
        assert got.shape == want.shape
        assert torch.allclose(got, want, rtol=rtol, atol=atol), \
            (got - want).abs().max()

    close(out, ref, 3e-2, 3e-2)
    close(rm, rm_ref, 1e-4, 1e-4)
    close(rv, rv_ref, 1e-4, 1e-4)
    close(gx, xr.grad, 5e-2, 5e-2)
    close(gw, wr.grad, 5e-2, 5e-1)
    close(gb, br.grad, 5e-2, 5e-1)
    if want_gres:
        close(gres, gout.double() * (ref > 0), 3e-2, 3e-2)
