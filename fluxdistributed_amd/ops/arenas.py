"""Per-device arenas behind the conv and FC ops: transposed weights for
dgrad, the fp32 wgrad workspace, padded FC weights, and the pool of padded
stem inputs. All are shared by task-DDP replica threads; `wt_arena` and
`wgrad_arena` are the only way to get the per-device ones."""

import threading

import torch
from torch.utils.weak import WeakIdKeyDictionary

from .native import require_native
from .step_state import step_epoch


class _WtArena:
    """Per-device cache of transposed conv weights wt[rs*C+c][k] for dgrad.

    All registered weights are transposed in ONE kernel launch per training
    step (wt_transpose_batch) instead of 36 per-layer permutes. Freshness:
    the step epoch (the fused optimizers write params through raw kernels,
    invisible to autograd) plus the sum of the weights' `_version` counters
    (covers torch.optim in-place updates).

    Registered weights are held STRONGLY, on purpose: the device-side table
    has their pointers baked in, and the strong reference keeps those valid
    and makes the id-keyed slice table safe without a guard. Weights of a
    deleted model stay registered for the life of the process; dropping
    them would force a table rebuild (a host-to-device upload) at a moment
    the arena does not choose, possibly inside a graph capture.
    """

    def __init__(self, device):
        self.device = device
        self.weights = []               # [(weight, K, RC)]
        self.slices = {}                # id(weight) -> (offset, RC, K)
        self.arena = None
        self.meta = None
        self.fresh_key = None
        # arenas are shared per-device across task-DDP replica threads:
        # register/rebuild/refresh are check-then-act and must not interleave
        self.lock = threading.Lock()

    def register(self, weight):
        with self.lock:
            if id(weight) in self.slices:
                return
            K, Cin, R, S = weight.shape
            RC = R * S * Cin
            self.weights.append((weight, K, RC))
            self.slices[id(weight)] = (None, RC, K)
            self.arena = None           # rebuild on next get

    def _build(self):
        dev = self.device
        total = sum(K * RC for (_, K, RC) in self.weights)
        self.arena = torch.empty(total, dtype=torch.bfloat16, device=dev)
        off = 0
        srcs, dsts, Ks, RCs, tiles = [], [], [], [], []
        for (w, K, RC) in self.weights:
            self.slices[id(w)] = (off, RC, K)
            srcs.append(w.data_ptr())
            dsts.append(self.arena.data_ptr() + off * 2)
            Ks.append(K)
            RCs.append(RC)
            tiles.append((K // 64) * (RC // 64))
            off += K * RC
        self.src_ptrs = srcs
        mk = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
        self.meta = (mk(srcs, torch.long), mk(dsts, torch.long),
                     mk(Ks, torch.int32), mk(RCs, torch.int32),
                     mk(tiles, torch.int32), max(tiles))

    def get(self, weight):
        with self.lock:
            key = (step_epoch(), sum(w._version for (w, _, _) in self.weights))
            if self.arena is None:
                self._build()
                self.fresh_key = None
            if self.fresh_key != key:
                # Revalidate source pointers before re-transposing: a p.data
                # rebind (flat-optimizer construction after a warmup backward,
                # model.to(), checkpoint load) leaves the baked device-side
                # meta pointing at freed storage. Checked only on refresh
                # (once per step), not per get().
                if [w.data_ptr() for (w, _, _) in self.weights] != self.src_ptrs:
                    self._build()
                C = require_native("wt_transpose_batch")
                s, d, k, rc, t, mt = self.meta
                C.wt_transpose_batch(s, d, k, rc, t, mt)
                self.fresh_key = key
            off, RC, K = self.slices[id(weight)]
            return self.arena[off : off + RC * K].view(RC, K)


class _WgradArena:
    """Step-scoped fp32 wgrad workspace: zeroed in ONE launch per backward
    epoch instead of a per-layer `zeros` each (the wgrad kernel accumulates
    into its slice with atomicAdd). Only weights whose wgrad runs the atomic
    kernel ever ask for a slot: the slab path (conv_igemm_wgrad_flush) writes
    flat G itself. A second wgrad call for the same weight
    inside one epoch (gradient micro-accumulation) re-zeros just its slice
    so the returned dw stays the per-backward gradient. Slot offsets are
    append-only: a dead weight's slot is not reused."""

    def __init__(self, device):
        self.device = device
        self.slots = WeakIdKeyDictionary()   # weight -> [offset, numel, seen]
        self.total = 0
        self.arena = None
        self.zero_epoch = None
        self.zeroings = 0       # whole-arena zeroings; slot[2] == this: seen
        # shared per-device across replica threads; without the lock two
        # threads can BOTH see zero_epoch stale and the second whole-arena
        # zero_() lands after the first thread's wgrad kernel (silent wipe)
        self.lock = threading.Lock()

    def get(self, weight):
        with self.lock:
            K, Cin, R, S = weight.shape
            slot = self.slots.get(weight)
            if slot is None:
                n = K * Cin * R * S
                slot = self.slots[weight] = [self.total, n, None]
                self.total += n
                self.arena = None
            if self.arena is None:
                self.arena = torch.empty(self.total, dtype=torch.float32,
                                         device=self.device)
                self.zero_epoch = None
            epoch = step_epoch()
            off, n, seen = slot
            sl = self.arena[off : off + n]
            if self.zero_epoch != epoch:
                self.arena.zero_()
                self.zero_epoch = epoch
                self.zeroings += 1
            elif seen == self.zeroings:
                sl.zero_()
            slot[2] = self.zeroings
            return sl.view(K, R * S * Cin)


class _FcPadArena:
    """Per-weight padded FC weight/bias: wpad [Kp, Cin] bf16 with zero rows
    >= N, bpad [Kp]. Refreshed when the step epoch moves (raw-kernel param
    updates are invisible to version counters) or the parameter storage is
    rebound."""

    def __init__(self):
        self.entries = WeakIdKeyDictionary()   # weight -> dict

    def get(self, weight, bias):
        ent = self.entries.get(weight)
        N, Cin = weight.shape
        Kp = (N + 63) // 64 * 64
        if ent is None:
            wpad = torch.zeros(Kp, Cin, dtype=weight.dtype,
                               device=weight.device)
            bpad = torch.zeros(Kp, dtype=weight.dtype, device=weight.device)
            # ONE canonical 4D channels_last view: the transpose arena keys
            # by id(), so the same view object must be reused everywhere
            wpad4 = wpad.view(Kp, 1, 1, Cin).permute(0, 3, 1, 2)
            ent = dict(wpad=wpad, bpad=bpad, wpad4=wpad4, key=None, Kp=Kp)
            self.entries[weight] = ent
            # register for the batched dgrad transpose: wt[c][k] k-contig
            wt_arena(wpad4.device).register(wpad4)
        key = (step_epoch(), weight._version,
               bias._version if bias is not None else 0,
               weight.data_ptr())
        if ent["key"] != key:
            C = require_native("fc_pad")
            # weight pads along ROWS: rows are contiguous, so the [N,Cin]
            # -> [Kp,Cin] row pad is a flat [1, N*Cin] -> [1, Kp*Cin] pad
            C.pad_rows_bf16_into(ent["wpad"].view(1, -1),
                                 weight.detach().contiguous().view(1, -1))
            if bias is not None:
                C.pad_rows_bf16_into(ent["bpad"].view(1, -1),
                                     bias.detach().reshape(1, -1).contiguous())
            ent["key"] = key
        return ent


_LOCK = threading.Lock()
_WT_BY_DEVICE: dict = {}
_WGRAD_BY_DEVICE: dict = {}
_PADS = _FcPadArena()


def _per_device(table, cls, device):
    arena = table.get(device)
    if arena is None:
        # created under the lock, after a second look: two replica threads
        # can never make two arenas for one device
        with _LOCK:
            arena = table.get(device)
            if arena is None:
                arena = table[device] = cls(device)
    return arena


def wt_arena(device) -> _WtArena:
    return _per_device(_WT_BY_DEVICE, _WtArena, device)


def wgrad_arena(device) -> _WgradArena:
    return _per_device(_WGRAD_BY_DEVICE, _WgradArena, device)


def fc_pad(weight, bias) -> dict:
    """The padded operands of an FC weight, refreshed if stale."""
    return _PADS.get(weight, bias)


# Free-list pool of padded stem inputs, keyed by shape. A buffer is checked
# OUT at stem forward (exclusively owned by that autograd graph via ctx.x8)
# and returned at backward — so concurrent task-DDP replica threads,
# gradient micro-accumulation, or two same-shape stems each get their own
# buffer and wgrad always reads the input of ITS forward. Pool reuse keeps
# the zero border: only the interior is rewritten on checkout.
_STEM_POOL: dict = {}
_STEM_POOL_LOCK = threading.Lock()
_STEM_POOL_CAP = 8   # per shape; beyond this, dropped buffers are GC'd


def stem_pool_get(key):
    with _STEM_POOL_LOCK:
        lst = _STEM_POOL.get(key)
        if lst:
            return lst.pop()
    return None


def stem_pool_put(key, buf):
    with _STEM_POOL_LOCK:
        lst = _STEM_POOL.setdefault(key, [])
        if len(lst) < _STEM_POOL_CAP:
            lst.append(buf)
