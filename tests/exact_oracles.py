"""Float64 and bit-exact references for the streaming kernels, shared by
test_exact_oracles_cpu.py and the four *_exact_gpu.py files.

Everything here is plain torch and runs on whatever device its operands live
on: the GPU tests evaluate the float64 formulas on the device (the sizes past
the grid caps hold millions of elements), the CPU test evaluates the same
functions on the host. Nothing here calls a HIP kernel.

Conventions
  * operands are seeded (a CPU generator) and rounded to the storage dtype
    before anything else sees them;
  * U32 = 2^-24 and UBF = 2^-8 are the unit roundoffs of fp32 and bf16 (the
    largest relative error of one round-to-nearest);
  * every bound is a tensor with one entry per output element; `worst`
    returns max err / bound and is what the tests print and assert on;
  * "cap" is a launcher's block cap times 256 lanes: past cap * V elements a
    lane of a streaming kernel runs its grid-stride loop a second time.
"""

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
UBF = 2.0 ** -8
GUARD = 64          # elements of guard on each side of a slice
NAN_BITS16 = 0x7FC1  # a quiet NaN no arithmetic here produces
CAP_LANES = 4096 * 256
GAP_CAP_LANES = 1024 * 256


def vec(dtype):
    """Elements of one 16 B lane access."""
    return 8 if dtype == torch.bfloat16 else 4


def store_u(dtype):
    return UBF if dtype == torch.bfloat16 else U32


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def rounded(shape, dtype, seed, scale=1.0):
    """Seeded normal values, rounded to the storage dtype (CPU tensor)."""
    return (torch.randn(shape, generator=gen(seed)) * scale).to(dtype)


def bits(t):
    """The tensor's bit patterns as integers (for exact comparison)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[
        t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(bits(a), bits(b))


def worst(err, bound):
    """max over elements of err / bound; an error where the bound is zero
    counts as infinite, 0 / 0 as 0."""
    err = err.double().reshape(-1)
    bound = bound.double().reshape(-1)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")),
                                    torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")),
                        ratio)
    return float(ratio.max()) if ratio.numel() else 0.0


def guarded(n, dtype, device, fill=float("nan")):
    """A buffer of GUARD + n + GUARD elements filled with `fill`, and its
    middle slice. GUARD elements are 128 B or more, so the slice keeps the
    16 B alignment the kernels need."""
    buf = torch.full((2 * GUARD + n,), fill, dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + n]


def guards_of(buf, n):
    return torch.cat([bits(buf[:GUARD]), bits(buf[GUARD + n:])])


# ---- round to nearest even, in integers ------------------------------------

def rne_bf16(x32):
    """float32 -> bfloat16 by integer arithmetic on the bit patterns (finite
    operands): add 0x7fff plus the lowest kept bit, drop the low half."""
    assert x32.dtype == torch.float32
    u = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = u + 0x7FFF + ((u >> 16) & 1)
    hi = ((u >> 16) & 0xFFFF)
    hi = torch.where(hi >= 0x8000, hi - 0x10000, hi).to(torch.int16)
    return hi.view(torch.bfloat16)


def to_storage(x32, dtype, emulate=False):
    if dtype == torch.float32:
        return x32
    return rne_bf16(x32) if emulate else x32.to(dtype)


# ---- cross-entropy ----------------------------------------------------------

# (N, C, row stride)
CE_CASES = [
    (96, 1000, 1000),
    (96, 1000, 1024),
    (7, 10, 64),
    (5, 257, 257),
    (3, 1, 8),
    (2051, 64, 64),
]
CE_SHIFT = 1.0e4


def ce_inputs(N, C, dtype, seed=0, shift=0.0):
    """Logits with max - min <= 16 per row (so D <= 16), rounded to `dtype`,
    and targets that include class 0 and class C - 1."""
    g = gen(1000 + seed)
    x = (torch.randn(N, C, generator=g) * 2).clamp_(-7.9, 7.9)
    if shift:
        x = x + torch.tensor(shift, dtype=torch.float32)
    x = x.to(dtype)
    t = torch.randint(0, C, (N,), generator=g)
    t[0], t[-1] = 0, C - 1
    return x, t


def ce_strided(x, ldl, poison):
    """x as the [:, :C] view of an [N, ldl] buffer whose pad columns hold NaN
    and +Inf alternately (poison) or zeros."""
    N, C = x.shape
    buf = torch.zeros(N, ldl, dtype=x.dtype, device=x.device)
    if poison and ldl > C:
        pad = torch.full((ldl - C,), float("nan"), dtype=x.dtype,
                         device=x.device)
        pad[1::2] = float("inf")
        buf[:, C:] = pad
    buf[:, :C] = x
    return buf[:, :C]


def ce_oracle(x, t, drop_max=False):
    """float64 log-softmax of the rounded logits: (loss, dlogits, p, D) with
    D[n] = max_c (max - x). drop_max leaves the row's largest class out of
    the row sum (the negative control; needs C > 1)."""
    x = x.double()
    N = x.shape[0]
    z = x - x.max(dim=1, keepdim=True).values
    e = torch.exp(z)
    if drop_max:
        e = e.scatter(1, z.argmax(dim=1, keepdim=True), 0.0)
    s = e.sum(dim=1, keepdim=True)
    p = torch.exp(z) / s
    zt = z.gather(1, t.view(-1, 1))
    loss = (-(zt - torch.log(s))).mean()
    onehot = torch.zeros_like(p).scatter_(1, t.view(-1, 1), 1.0)
    return loss, (p - onehot) / N, p, (-z).max(dim=1).values


def ce_loss_bound(C, D, loss):
    return (C + 2 * float(D.max()) + 8) * U32 * (1 + abs(float(loss)))


def ce_grad_bound(p, t, D, dtype):
    """Per element of dlogits = (p - onehot) / N:

        ((C + 2 D + 8) U32 p  +  onehot * 6 U32 |p - 1|) / N  +  u_store |ref|

    The first and last terms are the softmax bound and the store round. The
    middle one exists at the N target elements only: there the kernel forms
    fl(p - 1), fl(1 / N) and their rounded product, three fp32 roundings of a
    value of size |p - 1| ~ 1, which a bound relative to p cannot cover when
    p is small. It is 2 k U32 A with k = 3 and A = |p - 1|, the form the
    optimizer bounds take."""
    N, C = p.shape
    onehot = torch.zeros_like(p).scatter_(1, t.view(-1, 1), 1.0)
    k = (C + 2 * D.view(-1, 1) + 8) * U32
    ref = (p - onehot) / N
    return (k * p + onehot * 6 * U32 * (p - 1).abs()) / N + \
        store_u(dtype) * ref.abs()


def ce_float32_arm(x, t):
    """The kernel's formula in plain float32 torch, unrounded to storage."""
    x = x.float()
    N = x.shape[0]
    m = x.max(dim=1, keepdim=True).values
    e = torch.exp(x - m)
    s = e.sum(dim=1, keepdim=True)
    p = e * (1.0 / s)
    onehot = torch.zeros_like(p).scatter_(1, t.view(-1, 1), 1.0)
    d = (p - onehot) * torch.tensor(1.0 / N, dtype=torch.float32)
    xt = x.gather(1, t.view(-1, 1))
    loss = (-(xt - m - torch.log(s)) *
            torch.tensor(1.0 / N, dtype=torch.float32)).sum()
    return loss, d


# ---- fused SGD / Adam -------------------------------------------------------

def f32(v):
    """A hyper-parameter as the kernel receives it: cast to float."""
    return float(np.float32(v))


OPT_SIZES_SMALL = [64, 640]


def opt_sizes(dtype):
    return OPT_SIZES_SMALL + [CAP_LANES * vec(dtype) + 64 * 5]


def skip_index(n, dtype):
    """First element of the vector the 'one vector skipped' control leaves
    un-updated: the first element of the second pass where the size has one,
    else the last vector."""
    s = CAP_LANES * vec(dtype)
    return s if n > s else n - vec(dtype)


def _exact(t):
    return t


def fp32_points(t):
    """Round a float64 tensor to float32 and back: marks the points where
    the kernels round once the compiler has contracted a*b+c to a fused
    multiply-add (products of float32 values are exact in float64)."""
    return t.float().double()


def sgd_formula(g, m, v, lr, mom, wd, nesterov, r=_exact):
    """One step of sgd_step_kernel on float64 operands. r = identity is the
    oracle; r = fp32_points is the CPU arm: float32 arithmetic with a fused
    multiply-add wherever the kernel's source has a*b+c, which is how the
    compiler builds it. Returns (V', A_V, M', A_M): the outputs and the sum
    of the absolute values of their expressions' terms."""
    lr, mom, wd = f32(lr), f32(mom), f32(wd)
    gp, ag = g, g.abs()
    if wd != 0.0:
        gp = r(g + wd * m)
        ag = g.abs() + (wd * m).abs()
    v1 = r(mom * v + gp)
    av = (mom * v).abs() + ag
    if nesterov:
        upd = r(gp + mom * v1)
        au = ag + mom * av
    else:
        upd, au = v1, av
    m1 = r(m - lr * upd)
    am = m.abs() + lr * au
    return v1, av, m1, am


def sgd_k(wd, nesterov):
    """fp32 roundings on the way to (V', M'), counted in sgd_step_kernel:
    g' = g + wd m: a product and a sum (only if wd != 0); v' = mom v + g':
    a product and a sum; upd = g' + mom v': a product and a sum (nesterov
    only); m' = m - lr upd: a product and a sum."""
    kv = 2 + (2 if wd != 0.0 else 0)
    return kv, kv + 2 + (2 if nesterov else 0)


def adam_formula(g, m, m1, m2, lr, b1, b2, eps, wd, bc1, bc2, r=_exact):
    """One step of adam_step_kernel, as sgd_formula. Returns
    (M1', A_1, M2', A_2, M', A_M). 1 / bc is formed on the host in float, so
    it is an operand."""
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    i1 = float(np.float32(1.0) / np.float32(bc1))
    i2 = float(np.float32(1.0) / np.float32(bc2))
    ob1, ob2 = 1.0 - b1, 1.0 - b2
    if r is not _exact:
        ob1, ob2 = f32(ob1), f32(ob2)
    gp, ag = g, g.abs()
    if wd != 0.0:
        gp = r(g + wd * m)
        ag = g.abs() + (wd * m).abs()
    n1 = r(b1 * m1 + r(ob1 * gp))
    a1 = (b1 * m1).abs() + ob1 * ag
    n2 = r(b2 * m2 + r(r(ob2 * gp) * gp))
    a2 = (b2 * m2).abs() + ob2 * ag * ag
    denom = r(r(torch.sqrt(r(n2 * i2))) + eps)
    mn = r(m - r(r(lr * r(n1 * i1)) / denom))
    am = m.abs() + lr * i1 * a1 / denom
    return n1, a1, n2, a2, mn, am


def adam_k(wd):
    """fp32 roundings counted in adam_step_kernel. g': 2 if wd != 0.
    m1' = b1 m1 + (1 - b1) g': the difference, two products, a sum: 4.
    m2' = b2 m2 + (1 - b2) g' g': the difference, three products, a sum: 5,
    and g' enters twice, so its two roundings count twice.
    m' = m - lr (m1' i1) / (sqrt(m2' i2) + eps): three products, the
    correctly rounded square root and division, two sums: 7, on top of the
    roundings of m1' and of m2' (m2' has no cancellation, so its relative
    error is at most k2 U32, and half of it reaches the root)."""
    w = 2 if wd != 0.0 else 0
    k1, k2 = 4 + w, 5 + 2 * w
    return k1, k2, k1 + k2 + 7


def opt_bound(k, a):
    return 2 * k * U32 * a


def opt_state(n, dtype, seed):
    """(M0, V0, S0): the fp32 master, a signed first moment / momentum and a
    positive second moment."""
    g = gen(2000 + seed)
    m = torch.randn(n, generator=g)
    v = torch.randn(n, generator=g) * 0.5
    s = torch.rand(n, generator=g) * 1e-2 + 1e-3
    return m, v, s


# ---- pools ------------------------------------------------------------------

# (k, s, p), (N, C, H, W)
MAXPOOL_CASES = [
    ((3, 2, 1), (2, 64, 9, 9)),
    ((3, 2, 1), (1, 128, 17, 5)),
    ((3, 2, 1), (1, 128, 5, 17)),
    ((3, 1, 1), (2, 64, 6, 7)),
    ((2, 2, 0), (2, 64, 10, 10)),
    ((3, 3, 0), (1, 64, 11, 10)),
    ((5, 2, 2), (1, 64, 12, 9)),
]
MAXPOOL_CAP_CASE = ((2, 2, 0), (32, 128, 96, 96))
GAP_SHAPES = [(6, 512, 7, 7), (2, 64, 1, 1), (3, 2048, 8, 8)]
GAP_FWD_CAP_SHAPE = (1040, 2048, 1, 2)
GAP_BWD_CAP_SHAPE = (96, 2048, 7, 7)


def tie_free(shape, dtype, seed):
    """Every (image, channel) plane is a seeded permutation of consecutive
    integers centred on zero (the construction of test_stem_fuse_gpu's
    _tie_free). H * W <= 256 keeps them exact in bf16, so no two pixels of a
    plane are equal after rounding. NCHW-logical, channels_last memory."""
    n, c, h, w = shape
    hw = h * w
    assert hw <= 256, "integers beyond 256 are not exact in bf16"
    planes = torch.rand(n * c, hw, generator=gen(3000 + seed)).argsort(dim=1)
    x = (planes - hw // 2).float().view(n, c, h, w).to(dtype)
    return x.contiguous(memory_format=torch.channels_last)


def maxpool_oracle(x, k, s, p):
    """(out, idx bytes [N, HO, WO, C], flat argmax [N, C, HO, WO]) of the
    rounded input, from F.max_pool2d."""
    H, W = x.shape[2:]
    out, ind = F.max_pool2d(x.float(), k, s, p, return_indices=True)
    HO, WO = out.shape[2:]
    ho = torch.arange(HO, device=x.device).view(1, 1, HO, 1)
    wo = torch.arange(WO, device=x.device).view(1, 1, 1, WO)
    kh = ind // W - (ho * s - p)
    kw = ind % W - (wo * s - p)
    assert ((kh >= 0) & (kh < k) & (kw >= 0) & (kw < k)).all()
    idx = (kh * k + kw).permute(0, 2, 3, 1).contiguous().to(torch.uint8)
    return out.to(x.dtype), idx, ind


def maxpool_bwd_oracle(gout, ind, H, W, dtype):
    """float64 scatter of gout through the argmax: (ref, bound, selected).
    bound = 3 U32 sum |g| over the windows that select the pixel, plus the
    bf16 store round; `selected` is False where no window selects the pixel
    (there the result must be an exact zero, and the bound is zero)."""
    N, C = gout.shape[:2]
    g = gout.double().reshape(N, C, -1)
    flat = ind.reshape(N, C, -1)
    ref = torch.zeros(N, C, H * W, dtype=torch.float64, device=gout.device)
    sab = torch.zeros_like(ref)
    cnt = torch.zeros_like(ref)
    ref.scatter_add_(2, flat, g)
    sab.scatter_add_(2, flat, g.abs())
    cnt.scatter_add_(2, flat, torch.ones_like(g))
    bound = 3 * U32 * sab
    if dtype == torch.bfloat16:
        bound = bound + UBF * ref.abs()
    shape = (N, C, H, W)
    return ref.view(shape), bound.view(shape), (cnt > 0).view(shape)


def last_covered_column(W, k, s, p):
    """The last input column some pooling window covers (W - 1 unless
    trailing columns belong to no window)."""
    WO = (W + 2 * p - k) // s + 1
    return min(W - 1, (WO - 1) * s - p + k - 1)


def maxpool_bwd_float32_arm(gout, ind, H, W):
    N, C = gout.shape[:2]
    out = torch.zeros(N, C, H * W, dtype=torch.float32, device=gout.device)
    out.scatter_add_(2, ind.reshape(N, C, -1), gout.float().reshape(N, C, -1))
    return out.view(N, C, H, W)


def gap_oracle(x, drop_last=False):
    """(ref, bound): float64 mean over H x W of the rounded input, and
    (HW + 1) U32 mean|x| plus the store round. drop_last: the mean over the
    first HW - 1 pixels (the negative control; needs HW > 1)."""
    N, C, H, W = x.shape
    v = x.double().permute(0, 2, 3, 1).reshape(N, H * W, C)
    hw = H * W
    ref = v[:, :hw - 1].mean(dim=1) if drop_last else v.mean(dim=1)
    bound = (hw + 1) * U32 * v.abs().mean(dim=1) + \
        store_u(x.dtype) * v.mean(dim=1).abs()
    return ref, bound


def gap_float32_arm(x):
    N, C, H, W = x.shape
    v = x.float().permute(0, 2, 3, 1).reshape(N, H * W, C)
    acc = torch.zeros(N, C, dtype=torch.float32, device=x.device)
    for r in range(H * W):
        acc = acc + v[:, r]
    return acc * torch.tensor(1.0, dtype=torch.float32).div(H * W)


def gap_bwd_exact(gy, H, W, emulate=False):
    """round(g * fl(1 / HW)) broadcast over the plane; a product by the
    float32 reciprocal, not a division."""
    inv = torch.tensor(1.0, dtype=torch.float32, device=gy.device) / (H * W)
    if emulate:
        inv = torch.tensor(float(np.float32(1.0) / np.float32(H * W)),
                           dtype=torch.float32, device=gy.device)
    r = to_storage(gy.float() * inv, gy.dtype, emulate)
    N, C = gy.shape
    return r.view(N, C, 1, 1).expand(N, C, H, W).contiguous(
        memory_format=torch.channels_last)


# ---- bit-exact streaming ops ------------------------------------------------

def add_relu_sizes(dtype):
    return [5, 4099, CAP_LANES * vec(dtype) + 8 * 300 + 5]


def add_relu_exact(x, r, emulate=False):
    """round(max(fl32(x + r), 0)) in the storage dtype."""
    s = x.float() + r.float()
    if emulate:
        return to_storage(torch.where(s > 0, s, torch.zeros_like(s)),
                          x.dtype, True)
    return torch.relu(s).to(x.dtype)


def add_relu_bwd_exact(g, out):
    return torch.where(out.float() > 0, g, torch.zeros_like(g))


def accum_bf16_exact(g, ws, emulate=False):
    """bf16(f32(g) + ws), the expression of every flat-G accumulate."""
    return to_storage(g.float() + ws.float(), torch.bfloat16, emulate)


GRAD_ACCUM_SIZES = [8, 7, 2048 * 3 + 3]
GRAD_BATCH_LENGTHS = [9216, 64, 36864, 7, 2051]
PAD_CASES = [(96, 1000, 1024), (7, 32, 64), (3, 64, 64)]
BIAS_CASES = [(96, 1024), (7, 64)]
COLSUM_CASES = [(96, 1024, 1000), (7, 64, 32), (33, 320, 300)]
WT_CASES = [(64, 64), (128, 576), (64, 1152), (256, 128)]


def batch_layout(lengths):
    """Offsets of slices of the given lengths in one flat buffer: each
    starts on a multiple of 64 elements, with at least GUARD elements of gap
    before, between and after. Returns (offsets, total)."""
    offs, off = [], GUARD
    for n in lengths:
        offs.append(off)
        off = (off + n + 63) // 64 * 64 + GUARD
    return offs, off


def pad_rows_exact(src, ldl):
    M, C = src.shape
    dst = torch.zeros(M, ldl, dtype=src.dtype, device=src.device)
    dst[:, :C] = src
    return dst


def colsum_exact(g, dy, emulate=False):
    """Column sums of dy in float32, rows added one at a time in row order,
    then g <- bf16(f32(g) + sum) on the first g.numel() columns."""
    acc = torch.zeros(dy.shape[1], dtype=torch.float32, device=dy.device)
    if emulate:
        a = acc.cpu().numpy()
        rows = dy.float().cpu().numpy()
        for m in range(rows.shape[0]):
            a = a + rows[m]
        assert a.dtype == np.float32
        acc = torch.from_numpy(a).to(dy.device)
    else:
        for m in range(dy.shape[0]):
            acc = acc + dy[m].float()
    return accum_bf16_exact(g, acc[:g.numel()], emulate)


def counter_bf16(K, RC, start):
    """[K, RC] bf16 whose bit patterns count up from `start` (mod 2^16):
    distinct per element within any 65536 consecutive ones."""
    c = (torch.arange(K * RC, dtype=torch.int64) + start) % 65536
    c = torch.where(c >= 32768, c - 65536, c).to(torch.int16)
    return c.view(torch.bfloat16).view(K, RC)
