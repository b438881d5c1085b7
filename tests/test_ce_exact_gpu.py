"""ce_fwd against the float64 log-softmax of its rounded logits, per element.

Bound (exact_oracles.ce_loss_bound / ce_grad_bound), with D = max over the
row of (max - x) <= 16 by construction of the inputs:

    softmax value   (C + 2 D + 8) 2^-24 p
    dlogits         that / N, plus the store round 2^-8 |ref| (bf16) or
                    2^-24 |ref| (fp32), plus 6 * 2^-24 |p - 1| / N at the
                    target element (the one-hot subtraction and the scaling
                    by fl(1 / N): three fp32 roundings of a value near 1)
    loss            (C + 2 D + 8) 2^-24 (1 + |loss|)

C is the fp32 row sum, 2 D the argument error of the fast exponential (its
argument is scaled by log2 e in fp32), and the remaining 8 units rest on the
ISA's stated 1-ulp hardware exp and log. Nobody has measured that figure
here; the float32 CPU arm of test_exact_oracles_cpu.py stays under a quarter
of the bound with libm's exp/log.

Negative control: the reference with the largest class left out of the row
sum must miss the loss bound on every case with C > 1.

The loss is summed over rows with atomicAdd, so its low bits depend on the
order the blocks arrive in; the pad-column check therefore compares dlogits
bit for bit and holds each loss to the bound.
"""

import pytest
import torch

import exact_oracles as xo

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]


def _native():
    from fluxdistributed_amd.ops.native import require_native

    return require_native("ce_fwd")


def _ids(v):
    return str(v).replace("torch.", "").replace(" ", "")


def _run(x, t, ldl, poison=True):
    """ce_fwd on the [:, :C] view of an [N, ldl] buffer (the tensor itself
    when ldl == C)."""
    xd = x.cuda()
    view = xd if ldl == x.shape[1] else xo.ce_strided(xd, ldl, poison)
    loss, d = _native().ce_fwd(view, t.cuda())
    torch.cuda.synchronize()
    return loss, d


def _check(name, x, t, ldl, dtype):
    N, C = x.shape
    loss, d = _run(x, t, ldl)
    assert d.shape == (N, C) and d.is_contiguous() and d.dtype == dtype
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert torch.isfinite(loss) and torch.isfinite(d).all()
    rloss, rd, p, D = [v.cuda() for v in xo.ce_oracle(x, t)]
    assert float(D.max()) <= 16.0
    lb = xo.ce_loss_bound(C, D, rloss)
    rl = abs(float(loss) - float(rloss)) / lb
    rg = xo.worst((d.double() - rd).abs(), xo.ce_grad_bound(p, t.cuda(), D, dtype))
    rc = float("nan")
    if C > 1:
        closs = xo.ce_oracle(x, t, drop_max=True)[0]
        rc = abs(float(closs) - float(rloss)) / lb
    print(f"EXACT ce_fwd {name}: loss err/bound {rl:.3e}, dlogits err/bound "
          f"{rg:.3e}, control {rc:.3e}")
    assert rl <= 1.0 and rg <= 1.0
    assert C == 1 or rc > 1.0
    return loss, d


@pytest.mark.parametrize("case", xo.CE_CASES, ids=_ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_ce_fwd_matches_float64(case, dtype):
    N, C, ldl = case
    x, t = xo.ce_inputs(N, C, dtype)
    assert int(t[0]) == 0 and int(t[-1]) == C - 1
    loss, d = _check(f"{case} {_ids(dtype)}", x, t, ldl, dtype)
    if C == 1:
        assert float(loss) == 0.0 and not d.any()
    if ldl > C:
        # the NaN / +Inf pad columns change no bit of dlogits
        loss0, d0 = _run(x, t, ldl, poison=False)
        assert xo.same_bits(d, d0)
        assert torch.isfinite(loss0)


def test_ce_fwd_is_shift_invariant():
    """1.0e4 added to every fp32 logit: same bound as the unshifted case."""
    N, C, ldl = xo.CE_CASES[0]
    x, t = xo.ce_inputs(N, C, torch.float32, shift=xo.CE_SHIFT)
    assert float(x.min()) > 9.9e3
    _check(f"{xo.CE_CASES[0]} float32 shift={xo.CE_SHIFT}", x, t, ldl,
           torch.float32)
