"""Cross-op step state (ops/step_state.py) and the arenas over it
(ops/arenas.py) on the CPU: no GPU, no native extension."""

import gc
import threading

import pytest
import torch

from fluxdistributed_amd.ops import arenas, step_state as ss


def _in_thread(fn):
    out = []
    t = threading.Thread(target=lambda: out.append(fn()))
    t.start()
    t.join()
    return out[0]


def _same_memory(a, b):
    return (a.data_ptr() == b.data_ptr() and a.shape == b.shape
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr())


# ------------------------------------------------------------------ registry

def test_registry_slice_shares_storage_with_G():
    G = torch.zeros(64)
    p = torch.nn.Parameter(torch.zeros(3, 4))
    ss.register_flat_slice(p, G, 16, 12)
    sl = ss.flat_grad_slice(p)
    assert _same_memory(sl, G[16:28])
    sl.fill_(2.0)
    assert G[16:28].eq(2).all() and G.sum() == 24


def test_registry_unregistered_param_gives_none():
    assert ss.flat_grad_slice(torch.nn.Parameter(torch.zeros(3))) is None


def test_registry_drops_dead_params():
    G = torch.zeros(8)
    before = len(ss._FLAT)
    p = torch.nn.Parameter(torch.zeros(8))
    ss.register_flat_slice(p, G, 0, 8)
    assert len(ss._FLAT) == before + 1
    del p
    gc.collect()
    assert len(ss._FLAT) == before


# -------------------------------------------------------------- notification

def test_notify_calls_each_subscriber_once_until_unsubscribed():
    a, b = [], []
    p = torch.nn.Parameter(torch.zeros(1))
    assert not ss.has_grad_subscribers()
    ss.subscribe_grad_written(a.append)
    ss.subscribe_grad_written(b.append)
    try:
        assert ss.has_grad_subscribers()
        ss.notify_grad_written(p)
        assert len(a) == 1 and a[0] is p and len(b) == 1 and b[0] is p
    finally:
        ss.unsubscribe_grad_written(a.append)
        ss.unsubscribe_grad_written(b.append)
    ss.unsubscribe_grad_written(a.append)       # twice: harmless
    assert not ss.has_grad_subscribers()
    ss.notify_grad_written(p)
    assert len(a) == 1 and len(b) == 1


# ------------------------------------------------------------------ no_defer

def test_no_defer_nests_and_survives_exceptions():
    assert ss.deferral_ok()
    with ss.no_defer():
        assert not ss.deferral_ok()
        with ss.no_defer():
            assert not ss.deferral_ok()
        assert not ss.deferral_ok()
    assert ss.deferral_ok()
    with pytest.raises(ZeroDivisionError):
        with ss.no_defer():
            1 / 0
    assert ss.deferral_ok()


def test_no_defer_counter_is_exact_under_threads():
    def work():
        for _ in range(2000):
            with ss.no_defer():
                pass

    ts = [threading.Thread(target=work) for _ in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert ss.deferral_ok()


# ----------------------------------------------------------- conv-stats slot

def test_conv_stats_taken_once():
    y, part = torch.zeros(2, 3), torch.ones(4)
    ss.stash_conv_stats(y, part)
    assert ss.take_conv_stats(y) is part
    assert ss.take_conv_stats(y) is None


def test_conv_stats_other_tensor_misses_and_clears():
    y, part = torch.zeros(2, 3), torch.ones(4)
    ss.stash_conv_stats(y, part)
    assert ss.take_conv_stats(torch.zeros(2, 3)) is None
    assert ss.take_conv_stats(y) is None
    ss.stash_conv_stats(y, part)
    ss.clear_conv_stats()
    assert ss.take_conv_stats(y) is None


def test_conv_stats_slot_is_per_thread():
    y, part = torch.zeros(2, 3), torch.ones(4)
    ss.stash_conv_stats(y, part)
    assert _in_thread(lambda: ss.take_conv_stats(y)) is None
    assert ss.take_conv_stats(y) is part


# ------------------------------------------------------------ junction stash

def test_junction_stash_take_and_collision():
    x, g = torch.zeros(2, 3), torch.ones(2, 3)
    key = (x.data_ptr(), tuple(x.shape))
    assert ss.junction_stash_empty()
    ss.stash_junction_gres(key, g)
    assert not ss.junction_stash_empty()
    with pytest.raises(RuntimeError, match="gres stash collision"):
        ss.stash_junction_gres(key, g)
    assert ss.take_junction_gres(x) is g
    assert ss.junction_stash_empty()
    assert ss.take_junction_gres(x) is None


def test_junction_stash_is_per_thread():
    x, g = torch.zeros(2, 3), torch.ones(2, 3)
    ss.stash_junction_gres((x.data_ptr(), tuple(x.shape)), g)
    try:
        assert _in_thread(ss.junction_stash_empty)
        assert _in_thread(lambda: ss.take_junction_gres(x)) is None
    finally:
        assert ss.take_junction_gres(x) is g


# --------------------------------------------------------------- _WgradArena

def _weight(K, C, R=3, S=3):
    return torch.nn.Parameter(torch.randn(K, C, R, S))


def test_wgrad_arena_zeroing_rules():
    A = arenas._WgradArena(torch.device("cpu"))
    w1, w2 = _weight(4, 2), _weight(6, 3, 1, 1)
    s1 = A.get(w1)
    assert s1.shape == (4, 18) and s1.eq(0).all()
    s1.fill_(1)
    s2 = A.get(w2)          # new weight: a new arena, un-zeroed until now
    assert s2.shape == (6, 3) and s2.eq(0).all()
    assert A.arena.eq(0).all() and s1.eq(1).all()   # s1 views the old arena

    ss.bump_step_epoch()
    s1, s2 = A.get(w1), A.get(w2)
    s1.fill_(1)
    s2.fill_(1)
    again = A.get(w1)       # repeated get in one epoch: its own slice only
    assert again.data_ptr() == s1.data_ptr()
    assert s1.eq(0).all() and s2.eq(1).all()
    s1.fill_(1)
    ss.bump_step_epoch()
    A.get(w2)               # first get of the epoch: one whole-arena zero
    assert s1.eq(0).all() and s2.eq(0).all()


def test_wgrad_arena_first_get_of_epoch_does_not_rezero_slices():
    """Within an epoch only a REPEATED get of a weight zeroes its slice: the
    first get of another weight leaves what the first one accumulated."""
    A = arenas._WgradArena(torch.device("cpu"))
    w1, w2 = _weight(4, 2), _weight(6, 3, 1, 1)
    A.get(w1), A.get(w2)
    ss.bump_step_epoch()
    s1 = A.get(w1)
    s1.fill_(1)
    s2 = A.get(w2)              # first get of w2 in this epoch
    assert s1.eq(1).all() and s2.eq(0).all()


def test_wgrad_arena_dead_weight_slot_is_not_reused():
    A = arenas._WgradArena(torch.device("cpu"))
    w1, w2 = _weight(4, 2), _weight(6, 3, 1, 1)
    A.get(w1), A.get(w2)
    total = A.total
    del w2
    gc.collect()
    assert len(A.slots) == 1
    w3 = _weight(2, 5)
    s3 = A.get(w3)
    assert s3.shape == (2, 45) and s3.eq(0).all()
    assert A.total == total + 90 and A.slots[w3][0] == total   # appended
    s1 = A.get(w1)
    s1.fill_(1)
    s3.fill_(2)
    assert s1.eq(1).all() and s3.eq(2).all()        # disjoint, same arena
    assert A.arena.sum() == 72 + 180
    ss.bump_step_epoch()
    assert A.get(w1).eq(0).all() and s3.eq(0).all()


# ------------------------------------------------------------------ _WtArena

class _Recorder:
    def __init__(self):
        self.calls = []

    def wt_transpose_batch(self, *args):
        self.calls.append(args)


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(arenas, "require_native", lambda what: rec)
    return rec


def test_wt_arena_launches_once_per_refresh(recorder):
    A = arenas._WtArena(torch.device("cpu"))
    w1 = torch.nn.Parameter(torch.randn(64, 64, 3, 3).to(torch.bfloat16))
    w2 = torch.nn.Parameter(torch.randn(128, 64, 1, 1).to(torch.bfloat16))
    A.register(w1)
    A.register(w2)
    A.register(w1)              # again: no second slot
    assert len(A.weights) == 2
    t1 = A.get(w1)
    assert len(recorder.calls) == 1
    t2 = A.get(w2)
    A.get(w1)
    assert len(recorder.calls) == 1             # same epoch: fresh
    assert t1.shape == (9 * 64, 64) and t2.shape == (64, 128)
    lo1, lo2 = t1.data_ptr(), t2.data_ptr()
    assert lo1 + t1.numel() * 2 <= lo2 or lo2 + t2.numel() * 2 <= lo1

    ss.bump_step_epoch()
    A.get(w2)
    assert len(recorder.calls) == 2             # the epoch moved
    with torch.no_grad():
        w1.add_(1)
    A.get(w1)
    assert len(recorder.calls) == 3             # a _version moved
    A.get(w1)
    assert len(recorder.calls) == 3

    meta = A.meta
    w2.data = w2.data.clone()                   # rebound storage
    ss.bump_step_epoch()
    A.get(w2)
    assert len(recorder.calls) == 4
    assert A.meta is not meta                   # tables rebuilt first ...
    srcs = recorder.calls[-1][0]                # ... and the launch saw them
    assert srcs.tolist() == [w1.data_ptr(), w2.data_ptr()]


# ----------------------------------------------------------------- accessors

@pytest.mark.parametrize("accessor", [arenas.wt_arena, arenas.wgrad_arena])
def test_arena_accessor_gives_one_arena_per_device(accessor):
    dev = torch.device("meta")      # a device no other test has touched
    barrier = threading.Barrier(8)
    got = []

    def ask():
        barrier.wait()
        got.append(accessor(dev))

    ts = [threading.Thread(target=ask) for _ in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert len(got) == 8 and all(a is got[0] for a in got)
    assert accessor(torch.device("meta")) is got[0]
