"""Bit-exact tests of the streaming helpers whose result is one fp32
operation and one round, or a pure permutation:

    add_relu_fwd         round(max(fl32(x + r), 0))
    add_relu_bwd         out > 0 ? g : 0
    grad_accum_bf16      g <- bf16(f32(g) + ws)
    grad_accum_batch     the same over several slices, one launch
    pad_rows_bf16(_into) columns [0, C) the source bits, [C, ldl) +0
    bias_add_rows_bf16   y <- bf16(f32(y) + f32(bias))
    colsum_accum_bf16    g <- bf16(f32(g) + s), s the fp32 sum of the column
                         over the rows, in row order
    wt_transpose_batch   wt[rc][k] = w[k][rc]

Every kernel that writes in place or into a slice runs on a slice of a
larger buffer whose guard regions must keep their bits; destinations a
kernel must fill start NaN-filled.
"""

import pytest
import torch

import exact_oracles as xo

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DTYPES = [torch.bfloat16, torch.float32]
GUARD = xo.GUARD


def _native():
    from fluxdistributed_amd.ops.native import require_native

    return require_native("grad_accum_bf16")


def _ids(v):
    return str(v).replace("torch.", "").replace(" ", "")


def _guarded_copy(t):
    """t (CPU) as the middle slice of a NaN-guarded device buffer."""
    buf, sl = xo.guarded(t.numel(), t.dtype, "cuda")
    sl.copy_(t.reshape(-1))
    return buf, sl, xo.guards_of(buf, t.numel()).clone()


@pytest.mark.parametrize("size", [0, 1, 2], ids=["tail_only", "n4099",
                                                 "past_cap"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_add_relu_1d(dtype, size):
    n = xo.add_relu_sizes(dtype)[size]
    C = _native()
    x = xo.rounded(n, dtype, 51)
    r = xo.rounded(n, dtype, 52)
    r[:3] = -x[:3]      # sums that are exactly zero
    x, r = x.cuda(), r.cuda()
    out = C.add_relu_fwd(x, r)
    assert xo.same_bits(out, xo.add_relu_exact(x, r))
    g = xo.rounded(n, dtype, 53).cuda()
    gx = C.add_relu_bwd(g, out)
    assert xo.same_bits(gx, xo.add_relu_bwd_exact(g, out))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_add_relu_channels_last(dtype):
    shape = (2, 64, 5, 7)
    C = _native()
    cl = lambda t: t.cuda().contiguous(memory_format=torch.channels_last)
    x, r = cl(xo.rounded(shape, dtype, 54)), cl(xo.rounded(shape, dtype, 55))
    out = C.add_relu_fwd(x, r)
    assert out.shape == shape
    assert out.is_contiguous(memory_format=torch.channels_last)
    assert xo.same_bits(out, xo.add_relu_exact(x, r))
    g = cl(xo.rounded(shape, dtype, 56))
    gx = C.add_relu_bwd(g, out)
    assert xo.same_bits(gx, xo.add_relu_bwd_exact(g, out))


@pytest.mark.parametrize("n", xo.GRAD_ACCUM_SIZES)
def test_grad_accum_bf16(n):
    g0 = xo.rounded(n, BF16, 61)
    ws = xo.rounded(n, torch.float32, 62).cuda()
    buf, g, guards = _guarded_copy(g0)
    _native().grad_accum_bf16(g, ws)
    assert xo.same_bits(g, xo.accum_bf16_exact(g0.cuda(), ws))
    assert torch.equal(xo.guards_of(buf, n), guards)


def test_grad_accum_batch_equals_single_calls():
    C = _native()
    lengths = xo.GRAD_BATCH_LENGTHS
    offs, total = xo.batch_layout(lengths)
    flat0 = xo.rounded(total, BF16, 63).cuda()
    ws_flat = xo.rounded(total, torch.float32, 64).cuda()
    flat, single = flat0.clone(), flat0.clone()
    mk = lambda v: torch.tensor(v, dtype=torch.long, device="cuda")
    C.grad_accum_batch(mk([flat.data_ptr() + 2 * o for o in offs]),
                       mk([ws_flat.data_ptr() + 4 * o for o in offs]),
                       mk(lengths), max(lengths))
    want = flat0.clone()
    for o, n in zip(offs, lengths):
        C.grad_accum_bf16(single[o:o + n], ws_flat[o:o + n])
        want[o:o + n] = xo.accum_bf16_exact(flat0[o:o + n], ws_flat[o:o + n])
    # the slices hold the expression's bits, the gaps between them (the
    # guards) their own; five single calls give the same buffer
    assert xo.same_bits(flat, want)
    assert xo.same_bits(flat, single)
    assert not xo.same_bits(flat, flat0)


@pytest.mark.parametrize("case", xo.PAD_CASES, ids=_ids)
def test_pad_rows_bf16_and_into(case):
    M, Cc, ldl = case
    C = _native()
    src = xo.rounded((M, Cc), BF16, 71).cuda()
    want = xo.pad_rows_exact(src, ldl)
    got = C.pad_rows_bf16(src, ldl)
    assert got.shape == (M, ldl) and xo.same_bits(got, want)
    buf, sl, guards = _guarded_copy(
        torch.full((M * ldl,), float("nan"), dtype=BF16))
    C.pad_rows_bf16_into(sl.view(M, ldl), src)
    assert xo.same_bits(sl.view(M, ldl), want)   # pads are +0, not -0
    assert torch.equal(xo.guards_of(buf, M * ldl), guards)


@pytest.mark.parametrize("case", xo.BIAS_CASES, ids=_ids)
def test_bias_add_rows_bf16(case):
    M, ldl = case
    y0 = xo.rounded((M, ldl), BF16, 65)
    bias = xo.rounded(ldl, BF16, 66).cuda()
    buf, y, guards = _guarded_copy(y0)
    _native().bias_add_rows_bf16(y.view(M, ldl), bias)
    want = xo.accum_bf16_exact(y0.cuda(), bias.float().expand(M, ldl))
    assert xo.same_bits(y.view(M, ldl), want)
    assert torch.equal(xo.guards_of(buf, M * ldl), guards)


@pytest.mark.parametrize("case", xo.COLSUM_CASES, ids=_ids)
def test_colsum_accum_bf16(case):
    M, ldl, cvalid = case
    dy = xo.rounded((M, ldl), BF16, 67).cuda()
    g0 = xo.rounded(cvalid, BF16, 68)
    # the guard after the slice is where columns >= Cvalid would land
    buf, g, guards = _guarded_copy(g0)
    _native().colsum_accum_bf16(g, dy)
    assert xo.same_bits(g, xo.colsum_exact(g0.cuda(), dy))
    assert torch.equal(xo.guards_of(buf, cvalid), guards)


def test_wt_transpose_batch():
    C = _native()
    dev = "cuda"
    ws, start = [], 0
    for (K, RC) in xo.WT_CASES:
        ws.append(xo.counter_bf16(K, RC, start).to(dev))
        start += K * RC
    # destinations: slices of one arena, a guard before, between and after
    offs, total = xo.batch_layout([K * RC for (K, RC) in xo.WT_CASES])
    arena = torch.full((total,), xo.NAN_BITS16, dtype=torch.int16,
                       device=dev).view(BF16)
    want = xo.bits(arena).clone()
    tiles = [(K // 64) * (RC // 64) for (K, RC) in xo.WT_CASES]
    assert tiles == [1, 18, 18, 8]
    mk = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
    # the tables of ops/arenas.py: source and destination addresses, K, RC
    # and the 64 x 64 tile count per tensor; the grid is the largest count
    C.wt_transpose_batch(
        mk([w.data_ptr() for w in ws], torch.long),
        mk([arena.data_ptr() + 2 * o for o in offs], torch.long),
        mk([K for (K, _) in xo.WT_CASES], torch.int32),
        mk([RC for (_, RC) in xo.WT_CASES], torch.int32),
        mk(tiles, torch.int32), max(tiles))
    torch.cuda.synchronize()
    # compared as integers: the counters run through NaN patterns too
    for w, o, (K, RC) in zip(ws, offs, xo.WT_CASES):
        want[o:o + K * RC] = xo.bits(w).reshape(K, -1).t().reshape(-1)
    assert torch.equal(xo.bits(arena), want)
