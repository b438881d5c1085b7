"""maxpool_fwd / maxpool_bwd and gap_fwd / gap_bwd, exactly.

Max pool. Inputs are tie-free permutation planes (exact_oracles.tie_free), so
the argmax of every window is unique and everything is decidable: the
forward holds the bits of F.max_pool2d of the rounded input, the index bytes
equal kh * KW + kw recovered from return_indices, and the backward is held
to a float64 scatter of gout through those indices:

    fp32   |err| <= 3 * 2^-24 * sum |g|  over the windows that select the
           pixel (three fp32 adds where four windows meet)
    bf16   that plus 2^-8 |ref|
    pixels no window selects are exact zeros.

Negative control: the reference with the gradient of the last input column
that any window covers set to zero must miss the bound (with k = s = 3 the
last column of the plane belongs to no window and is zero already).

Global average pool. Forward against the float64 mean of the rounded input,
bound (HW + 1) 2^-24 mean|x| plus the store round; negative control the mean
over HW - 1 pixels. Backward bit-exact: the kernel computes
round(g * fl(1 / HW)), a product by the float32 reciprocal, not a division.

One shape per kernel lies past its launcher's block cap, where every lane
runs its grid-stride loop a second time.
"""

import functools

import pytest
import torch

import exact_oracles as xo

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]


def _native():
    from fluxdistributed_amd.ops.native import require_native

    return require_native("maxpool_fwd")


def _ids(v):
    return str(v).replace("torch.", "").replace(" ", "")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _pool_case(geom, shape, dtype):
    """Input, oracle and the kernel's forward, computed once per case and
    read by both tests below."""
    k, s, p = geom
    x = xo.tie_free(shape, dtype, 0).cuda()
    out, idx, ind = xo.maxpool_oracle(x, k, s, p)
    got, gidx = _native().maxpool_fwd(x, k, k, s, p)
    torch.cuda.synchronize()
    return x, out, idx, ind, got, gidx


@pytest.mark.parametrize("geom,shape", xo.MAXPOOL_CASES, ids=_ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_maxpool_fwd_bits_and_index_bytes(geom, shape, dtype):
    x, out, idx, ind, got, gidx = _pool_case(geom, shape, dtype)
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert xo.same_bits(_cl(got), _cl(out))
    assert gidx.dtype == torch.uint8
    assert torch.equal(gidx.view(idx.shape), idx)


@pytest.mark.parametrize("geom,shape", xo.MAXPOOL_CASES, ids=_ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_maxpool_bwd_matches_float64_scatter(geom, shape, dtype):
    k, s, p = geom
    N, C, H, W = shape
    x, out, idx, ind, got, gidx = _pool_case(geom, shape, dtype)
    gout = _cl(xo.rounded(tuple(out.shape), dtype, 31).cuda())
    gx = _native().maxpool_bwd(gout, gidx, H, W, k, k, s, p)
    torch.cuda.synchronize()
    assert gx.shape == (N, C, H, W) and gx.dtype == dtype
    ref, bound, sel = xo.maxpool_bwd_oracle(gout, ind, H, W, dtype)
    assert not gx[~sel].any(), "a pixel no window selects is not zero"
    if geom == (3, 3, 0):
        assert not sel[:, :, :, W - 1].any() and not sel[:, :, H - 2:].any()
    r = xo.worst((gx.double() - ref).abs(), bound)
    ctl = ref.clone()
    ctl[:, :, :, xo.last_covered_column(W, k, s, p)] = 0
    rc = xo.worst((ctl - ref).abs(), bound)
    print(f"EXACT maxpool_bwd {geom} {shape} {_ids(dtype)}: err/bound "
          f"{r:.3e}, control {rc:.3e}")
    assert r <= 1.0 and rc > 1.0


def test_maxpool_fwd_past_the_block_cap():
    (k, s, p), shape = xo.MAXPOOL_CAP_CASE
    # bit equality of the maximum only: ties do not matter to it
    x = _cl(torch.randn(shape, generator=xo.gen(33)).bfloat16().cuda())
    got, _ = _native().maxpool_fwd(x, k, k, s, p)
    ref = torch.nn.functional.max_pool2d(x.float(), k, s, p).bfloat16()
    assert xo.same_bits(_cl(got), _cl(ref))


def _gap_fwd(shape, dtype, name):
    N, C, H, W = shape
    x = _cl(xo.rounded(shape, dtype, 41).cuda())
    y = _native().gap_fwd(x)
    torch.cuda.synchronize()
    assert y.shape == (N, C) and y.dtype == dtype
    ref, bound = xo.gap_oracle(x)
    r = xo.worst((y.double() - ref).abs(), bound)
    rc = float("nan")
    if H * W > 1:
        rc = xo.worst((xo.gap_oracle(x, drop_last=True)[0] - ref).abs(), bound)
    print(f"EXACT gap_fwd {name} {shape} {_ids(dtype)}: err/bound {r:.3e}, "
          f"control {rc:.3e}")
    assert r <= 1.0
    assert H * W == 1 or rc > 1.0


def _gap_bwd(shape, dtype):
    N, C, H, W = shape
    gy = xo.rounded((N, C), dtype, 42).cuda()
    gx = _native().gap_bwd(gy, H, W)
    torch.cuda.synchronize()
    assert gx.is_contiguous(memory_format=torch.channels_last)
    assert xo.same_bits(_cl(gx), xo.gap_bwd_exact(gy, H, W))


@pytest.mark.parametrize("shape", xo.GAP_SHAPES, ids=_ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_gap_fwd_matches_float64(shape, dtype):
    _gap_fwd(shape, dtype, "")


@pytest.mark.parametrize("shape", xo.GAP_SHAPES, ids=_ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_gap_bwd_is_the_product_by_the_reciprocal(shape, dtype):
    _gap_bwd(shape, dtype)


def test_gap_past_the_block_caps():
    _gap_fwd(xo.GAP_FWD_CAP_SHAPE, torch.bfloat16, "past cap")
    _gap_bwd(xo.GAP_BWD_CAP_SHAPE, torch.float32)
