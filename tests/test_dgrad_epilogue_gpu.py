"""The conv input-grad (dgrad) epilogue on the GPU: LDS-staged, 16 B per
lane, with the deferred residual-junction gradient (`accum`) added at fp32
before the single bf16 round.

Bound per element, against an fp64 oracle built from the bf16 inputs (the
form of tests/test_infer_fused_gpu.py):

    |got - ref| <= 2^-8 |ref| + 2 gamma,  gamma = (R S K + 1) 2^-24 A,
    A = dgrad(|dy|, |w|) + |accum|

2^-8 is bf16's unit roundoff for the one store; gamma is the worst-case
bound of an fp32 accumulation of R S K products plus the one add of accum;
the second gamma is margin for the MFMA's internal summation order.
"""

import pytest
import torch
import torch.nn.functional as F

from fluxdistributed_amd.ops.native import load_native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CL = torch.channels_last

# (N, C, H, W, K, R, stride): dx is [N,C,H,W], dy is [N,K,P,Q].
# Stride-1 shapes carry the (BM, BN, SK, ring) they must reach.
SHAPES = {
    (2, 64, 9, 11, 64, 3, 1): (256, 64, 1, False),      # ragged last m-tile
    (2, 128, 9, 11, 128, 3, 1): (128, 128, 1, False),   # ragged, 2 m-tiles
    (2, 64, 9, 11, 128, 3, 2): None,                    # parity classes, odd H W
    (2, 64, 13, 13, 256, 1, 2): None,                   # three empty classes
    (2, 512, 7, 7, 512, 3, 1): (128, 128, 4, False),    # split-K, old path
    (48, 64, 56, 56, 64, 3, 1): (256, 64, 1, True),     # 256x64 BK32 ring
    (96, 128, 28, 28, 128, 3, 1): (128, 128, 1, True),  # 128x128 BK32 ring
}
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _dgrad64(dy, w, H, W, stride, pad):
    """fp64 input grad as matmul + fold (independent of the kernels under
    test), a few images at a time."""
    N, K, P, Q = dy.shape
    C, R = w.shape[1], w.shape[2]
    wm = w.double().reshape(K, C * R * R).t().contiguous()
    out = []
    for n0 in range(0, N, 8):
        d = dy[n0:n0 + 8].double().reshape(-1, K, P * Q)
        out.append(F.fold(wm @ d, (H, W), R, padding=pad, stride=stride))
    return torch.cat(out)


class Case:
    """Inputs and the fp64 oracle pieces for one shape, made once."""

    def __init__(self, shape):
        N, C, H, W, K, R, s = shape
        g = torch.Generator(device=DEV).manual_seed(sum(shape))
        self.shape, self.pad = shape, R // 2
        P = (H + 2 * self.pad - R) // s + 1
        Q = (W + 2 * self.pad - R) // s + 1
        self.dy = torch.randn(N, K, P, Q, device=DEV, generator=g).bfloat16() \
            .contiguous(memory_format=CL)
        w = (torch.randn(K, C, R, R, device=DEV, generator=g)
             / (R * R * K) ** 0.5).bfloat16()
        # wt[(r*S+s)*C + c][k], as ops/conv.py builds it
        self.wt = w.permute(2, 3, 1, 0).reshape(R * R * C, K).contiguous()
        self.acc = torch.randn(N, C, H, W, device=DEV, generator=g) \
            .bfloat16().contiguous(memory_format=CL)
        self.ref = _dgrad64(self.dy, w, H, W, s, self.pad)
        self.ref_abs = _dgrad64(self.dy.abs(), w.abs(), H, W, s, self.pad)

    def run(self, C_, acc):
        N, C, H, W, K, R, s = self.shape
        return C_.conv_igemm_dgrad(self.dy, self.wt, C, H, W, R, R, s, s,
                                   self.pad, self.pad, acc)


_CASES = {}


def case(shape):
    if shape not in _CASES:
        _CASES[shape] = Case(shape)
    return _CASES[shape]


@pytest.fixture(scope="module")
def C_():
    C = load_native()
    assert C is not None, "native extension not built"
    return C


@pytest.mark.parametrize("shape", [s for s in SHAPES if SHAPES[s]],
                         ids=[i for i, s in zip(IDS, SHAPES) if SHAPES[s]])
def test_shape_reaches_its_config(C_, shape):
    """A stride-1 dgrad is planned as a forward conv with C and K swapped:
    M = N H W rows, C output channels, R S K / 64 K-steps."""
    N, C, H, W, K, R, stride = shape
    got = tuple(C_.conv_igemm_fwd_config(N * H * W, K, C, R, R))
    assert got == SHAPES[shape]


@pytest.mark.parametrize("with_acc", [False, True], ids=["plain", "accum"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=IDS)
def test_dx_within_single_rounding_bound(C_, shape, with_acc):
    c = case(shape)
    N, C, H, W, K, R, stride = shape
    got = c.run(C_, c.acc if with_acc else None)
    assert got.shape == (N, C, H, W) and got.is_contiguous(memory_format=CL)
    ref, A = c.ref, c.ref_abs
    if with_acc:
        ref = ref + c.acc.double()
        A = A + c.acc.double().abs()
    gamma = (R * R * K + 1) * 2.0 ** -24 * A
    bound = 2.0 ** -8 * ref.abs() + 2 * gamma
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"dgrad_epilogue shape={shape} accum={with_acc} "
          f"worst err/bound={ratio:.3f}")
    assert bool((err <= bound).all()), f"worst err/bound = {ratio:.3f}"


@pytest.mark.parametrize("shape", list(SHAPES), ids=IDS)
def test_zero_accum_is_bit_equal_to_none(C_, shape):
    c = case(shape)
    got = c.run(C_, torch.zeros_like(c.acc))
    ref = c.run(C_, None)
    # -0 + 0 rounds to +0, so compare values, and NaN would fail it
    assert torch.equal(got, ref)


def test_empty_parity_classes_are_exactly_zero(C_):
    """1x1 stride 2, no padding: only pixels with even h and even w have a
    filter tap; the other three classes must come out as exact zeros, and
    as exactly accum where one is given."""
    shape = (2, 64, 13, 13, 256, 1, 2)
    c = case(shape)
    for acc in (None, c.acc):
        got = c.run(C_, acc)
        want = torch.zeros_like(got) if acc is None else acc
        assert torch.equal(got[:, :, 1::2, :], want[:, :, 1::2, :])
        assert torch.equal(got[:, :, :, 1::2], want[:, :, :, 1::2])
        assert bool((got[:, :, ::2, ::2] != want[:, :, ::2, ::2]).any())
