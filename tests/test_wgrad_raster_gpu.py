"""Weight-gradient kernels against a float64 reference, on the smallest
shapes at which the block decode of the 1-D wgrad grid can go wrong.

Reference: torch.nn.grad.conv2d_weight in float64 on the bf16-rounded
operands (exact products, so the only error left is the kernel's fp32
accumulation). Per-element bound, the project's form
(profiles/step_profile_r4.md):

    |got - ref| <= F * M * 2^-23 * sum |dy * x|        (M = N*P*Q)

with the sum taken by the same call on absolute values. F starts at 1/64
and is at least 8 times what the kernels before the 1-D grid measured on
these inputs (profiles/wgrad_raster.md): at most 2.3e-4 of the F = 1 bound
on every shape but the 198-pixel one, where M * 2^-23 is so small that the
accumulator's own rounding reaches 3.0e-3; that shape gets F = 1/32. A
float32 CPU arm sits at 2.2e-5 .. 6.7e-4 (4.1e-3 on the 198-pixel shape).

Negative control, in each test: the reference with one 64-pixel K-step of
dy zeroed must break the bound somewhere, so a block that is dropped (or,
by the same size of error, run twice) cannot pass. The dropped step measures
1.1, 5.1, 88, 27, 20 and 1.2e4 times the F = 1 bound on the body shapes
and 0.16 on the stem.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("GPU-only suite", allow_module_level=True)

from fluxdistributed_amd.ops.conv import pack_stem_operands  # noqa: E402
from fluxdistributed_amd.ops.native import require_native  # noqa: E402

F = 1.0 / 64
F_SHORT = 1.0 / 32    # the single-short-chunk shape (see above)

# (N, C, H, W, K, R, stride)
SHAPES = [
    (7, 128, 56, 56, 256, 3, 1),    # FT4, ktiles != ctiles, 11 chunks, ragged
    (14, 256, 28, 28, 256, 3, 1),   # FT4, 2x2 tiles
    (3, 64, 57, 57, 128, 3, 2),     # FT2, stride 2, odd size, grid % 8 != 0
    (5, 64, 56, 56, 128, 1, 2),     # 1x1 s2, two 2048-pixel chunks
    (6, 64, 56, 56, 128, 1, 2),     # 1x1 s2, 11 chunks of 448, ragged last
    (2, 64, 9, 11, 64, 3, 1),       # a single short chunk (F_SHORT)
]
STEM = (4, 3, 224, 224, 64, 7, 2, 3)   # (N, C, H, W, K, R, stride, pad)


def _weight_grad64(x, dy, k, c, r, s, pad):
    """[K][R][S][C] float64 weight gradient (the kernels' layout)."""
    g = torch.nn.grad.conv2d_weight(x, (k, c, r, r), dy, stride=s, padding=pad)
    return g.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _case(n, c, h, w, k, r, s, pad):
    """Operands and references of one shape, computed once and shared:
    (x bf16, dy bf16, ref, bound at F = 1, ref with one K-step dropped)."""
    gen = torch.Generator(device="cpu").manual_seed(1234 + c + h + k + r)
    P = (h + 2 * pad - r) // s + 1
    Q = (w + 2 * pad - r) // s + 1
    x = torch.randn(n, c, h, w, generator=gen).bfloat16()
    dy = torch.randn(n, k, P, Q, generator=gen).bfloat16()
    x64, dy64 = x.double(), dy.double()
    M = n * P * Q
    ref = _weight_grad64(x64, dy64, k, c, r, s, pad)
    mag = _weight_grad64(x64.abs(), dy64.abs(), k, c, r, s, pad)
    bound1 = M * 2.0 ** -23 * mag
    # drop the 64-pixel K-step in the middle of M: subtract what its pixels
    # add, computed from the images that hold them
    m0 = 64 * ((M // 64) // 2)
    m1 = min(m0 + 64, M)
    n0, n1 = m0 // (P * Q), (m1 - 1) // (P * Q) + 1
    only = torch.zeros(n1 - n0, P * Q, k, dtype=torch.float64)
    rows = dy64.permute(0, 2, 3, 1).reshape(M, k)
    only.view(-1, k)[m0 - n0 * P * Q:m1 - n0 * P * Q] = rows[m0:m1]
    only = only.view(n1 - n0, P, Q, k).permute(0, 3, 1, 2)
    dropped = ref - _weight_grad64(x64[n0:n1], only, k, c, r, s, pad)
    return x, dy, ref, bound1, dropped


def _check(name, got, ref, bound1, dropped, F=F):
    got = got.double().cpu().view_as(ref)
    ratio = ((got - ref).abs() / bound1).max().item()
    control = ((got - dropped).abs() / bound1).max().item()
    print(f"{name}: max |err| / (F=1 bound) = {ratio:.3e}; "
          f"dropped K-step = {control:.3e}; F = {F:.4f}")
    assert torch.isfinite(got).all()
    assert control > F, f"{name}: negative control passes the bound"
    assert ratio <= F, f"{name}: {ratio:.3e} of the F=1 bound, F={F}"


def _f_of(shape):
    return F_SHORT if shape == SHAPES[-1] else F


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("shape", SHAPES)
def test_wgrad_matches_float64(shape):
    n, c, h, w, k, r, s = shape
    x, dy, ref, bound1, dropped = _case(n, c, h, w, k, r, s, r // 2)
    C = require_native("conv_igemm_wgrad")
    ws = C.conv_igemm_wgrad(_cl(dy), _cl(x), r, r, s, s, r // 2, r // 2)
    assert ws.shape == (k, r * r * c)
    _check(f"wgrad {shape}", ws, ref, bound1, dropped, _f_of(shape))


@pytest.mark.parametrize("shape", SHAPES)
def test_wgrad_into_matches_float64(shape):
    n, c, h, w, k, r, s = shape
    x, dy, ref, bound1, dropped = _case(n, c, h, w, k, r, s, r // 2)
    C = require_native("conv_igemm_wgrad_into")
    # a slice of a larger arena, as the train step passes it
    arena = torch.zeros(2 * k * r * r * c + 64, device="cuda")
    ws = arena[64:64 + k * r * r * c]
    C.conv_igemm_wgrad_into(_cl(dy), _cl(x), ws, r, r, s, s, r // 2, r // 2)
    _check(f"wgrad_into {shape}", ws, ref, bound1, dropped, _f_of(shape))
    # nothing outside the slice is touched
    assert not arena[:64].any() and not arena[64 + k * r * r * c:].any()


def test_stem_wgrad_matches_float64():
    n, c, h, w, k, r, s, pad = STEM
    x, dy, ref, bound1, dropped = _case(n, c, h, w, k, r, s, pad)
    C = require_native("conv_stem_wgrad")
    wt = torch.zeros(k, c, r, r, dtype=torch.bfloat16, device="cuda")
    x8, _, P, Q = pack_stem_operands(_cl(x), wt, (s, s), (pad, pad))
    assert (P, Q) == tuple(dy.shape[2:])
    ws = C.conv_stem_wgrad(_cl(dy), x8, r, s, s)
    assert ws.shape == (k, r * 64)
    # ws [K][R][s<8][c<8]: the zero pad channels of x8 give exact zeros (the
    # eighth tap column reads real pixels and is simply not a weight)
    full = ws.view(k, r, 8, 8)
    got = full[:, :, :r, :c].contiguous()
    assert not full[:, :, :, c:].any()
    _check(f"stem wgrad {STEM}", got, ref, bound1, dropped)
