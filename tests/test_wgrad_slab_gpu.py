"""The slab weight-gradient path: per-chunk fp32 slabs written with plain
stores (conv_igemm_wgrad_slabs_into), the ordered fold (wgrad_slab_fold),
the two fused into a flat-G accumulate (conv_igemm_wgrad_flush), and the
train step's use of it.

Shapes, operands, the float64 reference, the bound

    |got - ref| <= F * M * 2^-23 * sum |dy * x|        (M = N*P*Q)

with F = 1/64 (1/32 on the 198-pixel shape) and the dropped-K-step negative
control are those of test_wgrad_raster_gpu.py, whose cached cases this file
shares. The fold is pure fp32 adds in chunk order, so it is compared bit for
bit with a float32 loop on the host over the read-back slabs.

Measured on MI355X, max |err| / (F = 1 bound) of the folded slabs, with the
atomic kernel on the same inputs in brackets (profiles/wgrad_slab.md):
5.1e-6 (5.0e-6), 1.4e-5 (1.3e-5), 2.2e-4 (2.2e-4), 2.4e-5 (2.9e-5) and
3.0e-3 (3.0e-3) in the order of SHAPES; the dropped K-step measures what it
does there. The autograd arms sit at 0.875 of their tolerance with the knob
on and off: the bf16 rounding of G, not the accumulation.

The stem keeps its atomic kernel (its slab form measured slower than the
parent's maximum), so it has no case here.
"""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("GPU-only suite", allow_module_level=True)

from test_wgrad_raster_gpu import F, F_SHORT, _case, _check, _cl  # noqa: E402

from fluxdistributed_amd.ops import step_state  # noqa: E402
from fluxdistributed_amd.ops.arenas import wgrad_arena  # noqa: E402
from fluxdistributed_amd.ops.conv import FdaConv2d  # noqa: E402
from fluxdistributed_amd.ops.native import require_native  # noqa: E402

# (N, C, H, W, K, R, stride)
SHAPES = [
    (7, 128, 56, 56, 256, 3, 1),    # FT4, ktiles != ctiles, ragged chunks
    (14, 256, 28, 28, 256, 3, 1),   # FT4, 2x2 tiles, 14 chunks
    (3, 64, 57, 57, 128, 3, 2),     # FT2, 2 chunks
    (6, 64, 56, 56, 128, 1, 2),     # 11 chunks of 448, ragged last
    (2, 64, 9, 11, 64, 3, 1),       # one short chunk (F_SHORT)
]
GUARD = 64
AUTOGRAD_SHAPE = SHAPES[1]


def _f_of(shape):
    return F_SHORT if shape == SHAPES[4] else F


def _geom(shape):
    n, c, h, w, k, r, s = shape
    pad = r // 2
    P = (h + 2 * pad - r) // s + 1
    Q = (w + 2 * pad - r) // s + 1
    return n * P * Q, k * r * r * c


def _nch(shape):
    n, c, h, w, k, r, s = shape
    C = require_native("conv_igemm_wgrad_config")
    return C.conv_igemm_wgrad_config(_geom(shape)[0], c, k, r, r)[2]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4
                               else torch.int16)


@functools.lru_cache(maxsize=None)
def _slabs(shape):
    """(guarded buffer, nch, n): the slab kernel's output on a buffer
    pre-filled with one NaN pattern, GUARD floats of it on each side. Computed
    once per shape and read by every test below; none of them writes it."""
    n_, c, h, w, k, r, s = shape
    x, dy, *_ = _case(n_, c, h, w, k, r, s, r // 2)
    C = require_native("conv_igemm_wgrad_slabs_into")
    n = _geom(shape)[1]
    nch = _nch(shape)
    buf = torch.full((2 * GUARD + nch * n,), float("nan"), device="cuda")
    C.conv_igemm_wgrad_slabs_into(_cl(dy), _cl(x), buf[GUARD:GUARD + nch * n],
                                  r, r, s, s, r // 2, r // 2)
    torch.cuda.synchronize()
    return buf, nch, n


@functools.lru_cache(maxsize=None)
def _folded(shape):
    buf, nch, n = _slabs(shape)
    C = require_native("wgrad_slab_fold")
    out = torch.full((n,), float("nan"), device="cuda")
    C.wgrad_slab_fold(buf[GUARD:GUARD + nch * n], nch, out)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_every_slab_element_is_written_once_and_nothing_else(shape):
    buf, nch, n = _slabs(shape)
    nan_bits = _bits(torch.full((1,), float("nan"), device="cuda"))[0]
    assert torch.isfinite(buf[GUARD:GUARD + nch * n]).all()
    assert (_bits(buf[:GUARD]) == nan_bits).all()
    assert (_bits(buf[GUARD + nch * n:]) == nan_bits).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_fold_is_the_ordered_float32_sum(shape):
    buf, nch, n = _slabs(shape)
    host = buf[GUARD:GUARD + nch * n].cpu().numpy().reshape(nch, n)
    s = host[0].copy()
    for c in range(1, nch):
        s = s + host[c]
    assert s.dtype == np.float32
    got = _folded(shape).cpu().numpy()
    assert np.array_equal(got.view(np.int32), s.view(np.int32))


@pytest.mark.parametrize("shape", SHAPES)
def test_folded_slabs_match_float64(shape):
    n_, c, h, w, k, r, s = shape
    _, _, ref, bound1, dropped = _case(n_, c, h, w, k, r, s, r // 2)
    _check(f"slab wgrad {shape}", _folded(shape), ref, bound1, dropped,
           _f_of(shape))


def test_the_shapes_cover_the_chunk_counts():
    assert [_nch(s) for s in SHAPES] == [27, 14, 2, 11, 1]


@pytest.mark.parametrize("shape", [s for s in SHAPES if _nch(s) >= 3])
def test_two_calls_give_identical_bits(shape):
    n_, c, h, w, k, r, s = shape
    x, dy, *_ = _case(n_, c, h, w, k, r, s, r // 2)
    C = require_native("conv_igemm_wgrad_slabs_into")
    buf, nch, n = _slabs(shape)
    xd, dyd = _cl(x), _cl(dy)
    a = (r, r, s, s, r // 2, r // 2)
    # a second run of the slab kernel and of the fold, on fresh buffers
    slab = torch.full((nch * n,), float("nan"), device="cuda")
    C.conv_igemm_wgrad_slabs_into(dyd, xd, slab, *a)
    assert torch.equal(_bits(slab), _bits(buf[GUARD:GUARD + nch * n]))
    out = torch.empty(n, device="cuda")
    C.wgrad_slab_fold(slab, nch, out)
    assert torch.equal(_bits(out), _bits(_folded(shape)))
    # the allocating form, where the rule sends the shape to slabs: the
    # fold's bits, twice
    if C.conv_igemm_wgrad_mode(_geom(shape)[0], c, k, r, r) == "slab":
        w1 = C.conv_igemm_wgrad(dyd, xd, *a)
        w2 = C.conv_igemm_wgrad(dyd, xd, *a)
        assert torch.equal(_bits(w1), _bits(w2))
        assert torch.equal(_bits(w1.view(-1)), _bits(_folded(shape)))


def _random_g(n, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(2 * GUARD + n, generator=gen).bfloat16().cuda()


@pytest.mark.parametrize("shape", SHAPES)
def test_flush_accumulates_into_the_slice_only(shape):
    n_, c, h, w, k, r, s = shape
    x, dy, *_ = _case(n_, c, h, w, k, r, s, r // 2)
    C = require_native("conv_igemm_wgrad_flush")
    n = _geom(shape)[1]
    g0 = _random_g(n, 7)
    g = g0.clone()
    C.conv_igemm_wgrad_flush(_cl(dy), _cl(x), g[GUARD:GUARD + n], r, r, s, s,
                             r // 2, r // 2)
    want = (g0[GUARD:GUARD + n].float() + _folded(shape)).bfloat16()
    assert torch.equal(_bits(g[GUARD:GUARD + n]), _bits(want))
    assert torch.equal(_bits(g[:GUARD]), _bits(g0[:GUARD]))
    assert torch.equal(_bits(g[GUARD + n:]), _bits(g0[GUARD + n:]))


@pytest.mark.parametrize("knob", ["1", "0"])
def test_autograd_writes_flat_g(knob, monkeypatch):
    monkeypatch.setenv("FLUXDIST_WGRAD_SLAB", knob)
    shape = AUTOGRAD_SHAPE
    n_, c, h, w, k, r, s = shape
    x, dy, ref, bound1, _ = _case(n_, c, h, w, k, r, s, r // 2)
    conv = FdaConv2d(c, k, r, stride=s, padding=r // 2, bias=False)
    conv = conv.cuda().bfloat16().to(memory_format=torch.channels_last)
    n = _geom(shape)[1]
    G = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    step_state.register_flat_slice(conv.weight, G, 0, n)
    y = conv(_cl(x))
    y.backward(_cl(dy))
    torch.cuda.synchronize()
    assert conv.weight.grad is None
    got = G.double().cpu().view_as(ref)
    tol = 2.0 ** -8 * ref.abs() + F * bound1
    err = ((got - ref).abs() / tol).max().item()
    print(f"autograd knob={knob}: max |err| / tol = {err:.3e}")
    assert torch.isfinite(got).all() and err <= 1.0
    slot = wgrad_arena(conv.weight.device).slots.get(conv.weight)
    assert (slot is None) == (knob == "1")


def test_flush_replays_from_a_captured_graph():
    shape = AUTOGRAD_SHAPE
    n_, c, h, w, k, r, s = shape
    x, dy, *_ = _case(n_, c, h, w, k, r, s, r // 2)
    C = require_native("conv_igemm_wgrad_flush")
    n = _geom(shape)[1]
    xd, dyd = _cl(x), _cl(dy)
    g0 = _random_g(n, 11)[GUARD:GUARD + n].clone()
    g = g0.clone()

    def call():
        C.conv_igemm_wgrad_flush(dyd, xd, g, r, r, s, s, r // 2, r // 2)

    call()
    torch.cuda.synchronize()
    eager = g.clone()
    # warm-up on a side stream, then a single-stream capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        g.copy_(g0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(g), _bits(eager))
