"""sgd_step and adam_step against the same recurrence in float64.

Each case runs three consecutive steps with fresh gradients. Before every
step the kernel's own fp32 state (master, momentum / moments) is read back
and the float64 oracle steps from exactly those values, so the errors of one
step never reach the next step's reference.

Bound for every fp32 output: 2 * k * 2^-24 * A, with A the sum of the
absolute values of the expression's terms in float64 and k the number of
fp32 roundings on the path, counted from the kernel source (contraction to a
fused multiply-add only removes some):

    SGD   V' = mom V + g'                    k = 2   (4 with weight decay:
                                                      g' = g + wd M adds 2)
          M' = M - lr V'                     k = k_V + 2
          M' = M - lr (g' + mom V')          k = k_V + 4       (nesterov)
    Adam  M1' = b1 M1 + (1 - b1) g'          k = 4   (6 with weight decay)
          M2' = b2 M2 + (1 - b2) g' g'       k = 5   (9: g' enters twice)
          M'  = M - lr (M1' / bc1) / (sqrt(M2' / bc2) + eps)
                                             k = k_1 + k_2 + 7
          (square root and division are correctly rounded, __fsqrt_rn and
          IEEE /, and count one each)

Exact checks: bf16 P holds the bits of M'.bfloat16(); fp32 P without a
master is M'; with a separate master (check_optimizer_operands lets one
through for fp32: any fp32 M that is not P itself) P holds the bits of M';
G keeps its bits; the guards around every slice keep theirs.

Negative controls, from the reference alone, must miss the bound at every
size: the other nesterov setting, weight decay dropped, and one vector of V
elements left un-updated (at cap * V, the first element of the second pass,
where the size has one; else the last vector).
"""

import pytest
import torch

import exact_oracles as xo

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
# (param dtype, separate fp32 master)
INSTANCES = [(BF16, True), (F32, False), (F32, True)]
INSTANCE_IDS = ["bf16", "fp32_alias", "fp32_master"]
SIZE_IDS = ["n64", "n640", "past_cap"]
STEPS = 3


def _native():
    from fluxdistributed_amd.ops.native import require_native

    return require_native("sgd_step")


class _Flat:
    """P, G, the master and the state buffers as slices of larger buffers
    with guards on both sides."""

    def __init__(self, n, dtype, master, nstate, seed):
        self.n, self.dtype = n, dtype
        m0, v0, s0 = xo.opt_state(n, dtype, seed)
        if nstate == 2:
            v0 = v0 * 0.2
        self.bufs = {}
        self.P = self._slice("P", dtype, m0.to(dtype))
        self.G = self._slice("G", dtype, torch.zeros(n, dtype=dtype))
        # bf16 steps from the fp32 master it was rounded from; a separate
        # fp32 master starts equal to P
        self.M = self._slice("M", F32, m0) if master else self.P
        self.state = [self._slice(f"S{i}", F32, s)
                      for i, s in enumerate((v0, s0)[:nstate])]
        self.guards = {k: xo.guards_of(b, n).clone()
                       for k, b in self.bufs.items()}

    def _slice(self, name, dtype, init):
        buf, sl = xo.guarded(self.n, dtype, "cuda")
        sl.copy_(init)
        self.bufs[name] = buf
        return sl

    def guards_intact(self):
        return all(torch.equal(xo.guards_of(b, self.n), self.guards[k])
                   for k, b in self.bufs.items())

    def check_exact(self, g_before):
        assert xo.same_bits(self.G, g_before), "G changed"
        assert xo.same_bits(self.P, self.M.to(self.dtype)), "P is not round(M)"
        assert self.guards_intact(), "a guard region changed"


def _skip(ref, prev, n, dtype):
    s, V = xo.skip_index(n, dtype), xo.vec(dtype)
    out = ref.clone()
    out[s:s + V] = prev[s:s + V]
    return out


@pytest.mark.parametrize("size", [0, 1, 2], ids=SIZE_IDS)
@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["wd0", "wd1e-2"])
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("inst", INSTANCES, ids=INSTANCE_IDS)
def test_sgd_step_matches_float64(inst, nesterov, wd, size):
    dtype, master = inst
    n = xo.opt_sizes(dtype)[size]
    lr, mom = 0.05, 0.9
    C = _native()
    f = _Flat(n, dtype, master, 1, seed=size)
    kv, km = xo.sgd_k(wd, nesterov)
    worst_v = worst_m = 0.0
    ctl = {}
    for step in range(STEPS):
        f.G.copy_(xo.rounded(n, dtype, 100 * size + step))
        g0 = f.G.clone()
        prev = (f.G.double(), f.M.double(), f.state[0].double())
        C.sgd_step(f.P, f.G, f.M, f.state[0], lr, mom, wd, nesterov)
        torch.cuda.synchronize()
        v1, av, m1, am = xo.sgd_formula(*prev, lr, mom, wd, nesterov)
        bv, bm = xo.opt_bound(kv, av), xo.opt_bound(km, am)
        worst_v = max(worst_v, xo.worst((f.state[0].double() - v1).abs(), bv))
        worst_m = max(worst_m, xo.worst((f.M.double() - m1).abs(), bm))
        f.check_exact(g0)
        if step == 0:
            o = xo.sgd_formula(*prev, lr, mom, wd, not nesterov)
            ctl["nesterov"] = xo.worst((o[2] - m1).abs(), bm)
            if wd != 0.0:
                o = xo.sgd_formula(*prev, lr, mom, 0.0, nesterov)
                ctl["wd"] = min(xo.worst((o[0] - v1).abs(), bv),
                                xo.worst((o[2] - m1).abs(), bm))
            ctl["skip"] = min(
                xo.worst((_skip(v1, prev[2], n, dtype) - v1).abs(), bv),
                xo.worst((_skip(m1, prev[1], n, dtype) - m1).abs(), bm))
    print(f"EXACT sgd_step {INSTANCE_IDS[INSTANCES.index(inst)]} n={n} "
          f"nesterov={nesterov} wd={wd}: V err/bound {worst_v:.3e} (k={kv}), "
          f"M err/bound {worst_m:.3e} (k={km}), controls "
          + ", ".join(f"{k} {v:.3e}" for k, v in ctl.items()))
    assert worst_v <= 1.0 and worst_m <= 1.0
    assert all(v > 1.0 for v in ctl.values()), ctl


@pytest.mark.parametrize("size", [0, 1, 2], ids=SIZE_IDS)
@pytest.mark.parametrize("bc_step", [1, 3], ids=["bc1", "bc3"])
@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["wd0", "wd1e-2"])
@pytest.mark.parametrize("inst", INSTANCES, ids=INSTANCE_IDS)
def test_adam_step_matches_float64(inst, wd, bc_step, size):
    dtype, master = inst
    n = xo.opt_sizes(dtype)[size]
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    bc1, bc2 = 1 - b1 ** bc_step, 1 - b2 ** bc_step
    C = _native()
    f = _Flat(n, dtype, master, 2, seed=size)
    ks = xo.adam_k(wd)
    worst = [0.0, 0.0, 0.0]
    ctl = {}
    for step in range(STEPS):
        f.G.copy_(xo.rounded(n, dtype, 200 * size + step))
        g0 = f.G.clone()
        prev = (f.G.double(), f.M.double(), f.state[0].double(),
                f.state[1].double())
        C.adam_step(f.P, f.G, f.M, f.state[0], f.state[1], lr, b1, b2, eps,
                    wd, bc1, bc2)
        torch.cuda.synchronize()
        ref = xo.adam_formula(*prev, lr, b1, b2, eps, wd, bc1, bc2)
        got = (f.state[0], f.state[1], f.M)
        bounds = [xo.opt_bound(ks[i], ref[2 * i + 1]) for i in range(3)]
        for i in range(3):
            worst[i] = max(worst[i], xo.worst(
                (got[i].double() - ref[2 * i]).abs(), bounds[i]))
        f.check_exact(g0)
        if step == 0:
            if wd != 0.0:
                o = xo.adam_formula(*prev, lr, b1, b2, eps, 0.0, bc1, bc2)
                ctl["wd"] = min(xo.worst((o[2 * i] - ref[2 * i]).abs(),
                                         bounds[i]) for i in range(3))
            before = (prev[2], prev[3], prev[1])
            ctl["skip"] = min(xo.worst(
                (_skip(ref[2 * i], before[i], n, dtype) - ref[2 * i]).abs(),
                bounds[i]) for i in range(3))
    print(f"EXACT adam_step {INSTANCE_IDS[INSTANCES.index(inst)]} n={n} "
          f"wd={wd} bc_step={bc_step}: err/bound M1 {worst[0]:.3e} "
          f"M2 {worst[1]:.3e} M {worst[2]:.3e} (k={ks}), controls "
          + ", ".join(f"{k} {v:.3e}" for k, v in ctl.items()))
    assert max(worst) <= 1.0
    assert all(v > 1.0 for v in ctl.values()), ctl
