"""Flat gradient sync (parallel/flatsync.py) on logical CPU devices: the
torch path of FlatGradReducer, the flat mode of prepare_training/train, its
validation errors and the CLI switch. The definition under test is a
sequential fp32 sum in replica order, one division by R, one cast."""

import copy
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

import fluxdistributed_amd
from fluxdistributed_amd.ops import FusedSGDMomentum, logit_cross_entropy
from fluxdistributed_amd.parallel import FlatGradReducer
from fluxdistributed_amd.parallel.gradtree import (
    ensure_synced, grads_of, sync_buffer,
)
from fluxdistributed_amd.parallel.task_ddp import (
    Replica, prepare_training, train, train_step,
)


def _mlp(seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Flatten(), nn.Linear(12, 16), nn.ReLU(), nn.Linear(16, 4))


def _loss(out, y):
    return logit_cross_entropy(out, y)


def _sgd(lr=0.05, momentum=0.9):
    return lambda m: FusedSGDMomentum(m.parameters(), lr=lr, momentum=momentum)


def _batches(n):
    def batches(j):
        torch.manual_seed(100 + j)
        return [(torch.randn(2, 3, 2, 2), torch.randint(0, 4, (2,)))
                for _ in range(n)]
    return batches


def test_exports():
    assert fluxdistributed_amd.FlatGradReducer is FlatGradReducer


def test_flat_reduce_equals_sync_buffer(seed):
    """fp32: the tree fold is itself a sequential fp32 sum and a divide, so
    the two must agree exactly, on every replica."""
    st = prepare_training(_mlp(), None, devices=[0, 1, 2], opt_factory=_sgd())
    x = torch.randn(6, 3, 2, 2)
    y = torch.randint(0, 4, (6,))
    for i, r in enumerate(st.replicas):
        sl = slice(2 * i, 2 * i + 2)
        train_step(_loss, st.buffer, r, x[sl], y[sl])
    final = sync_buffer(st.buffer)

    red = FlatGradReducer(st.replicas)
    red.reduce()
    for r in st.replicas:
        for k, g in grads_of(r.model).items():
            assert torch.equal(g, final[k]), (r.index, k)
    assert red.pop_nonfinite() is False


def test_flat_reduce_bf16_is_the_definition(seed):
    """bf16 groups: fp32 accumulation in replica order, rounded once."""
    reps = []
    for i in range(3):
        m = _mlp().bfloat16()
        reps.append(Replica(i, i, m, FusedSGDMomentum(m.parameters(), lr=0.1)))
    scales = [1.0, 1e-3, 1e3]
    snaps = []
    for r, s in zip(reps, scales):
        G = r.optimizer.groups[0].G
        G.copy_((torch.randn(G.numel()) * s).bfloat16())
        snaps.append(G.clone())
    FlatGradReducer(reps).reduce()
    acc = snaps[0].float().clone()
    for t in snaps[1:]:
        acc += t.float()
    expect = (acc / 3).to(torch.bfloat16)
    for r in reps:
        assert torch.equal(r.optimizer.groups[0].G, expect), r.index


def test_flat_mode_allocates_no_buffer_tree():
    st = prepare_training(_mlp(), None, devices=[0, 1], opt_factory=_sgd(),
                          grad_sync="flat")
    assert st.buffer == {}
    assert isinstance(st.reducer, FlatGradReducer)
    assert st.nonfinite_steps == 0
    tree = prepare_training(_mlp(), None, devices=[0, 1], opt_factory=_sgd())
    assert tree.reducer is None and len(tree.buffer) == 2


def test_flat_matches_large_batch(seed):
    """test_task_ddp_matches_large_batch in flat mode, same tolerance."""
    model = _mlp(7)
    xs = [torch.randn(4, 3, 2, 2) for _ in range(3)]
    ys = [torch.randint(0, 4, (4,)) for _ in range(3)]

    solo = copy.deepcopy(model)
    opt = FusedSGDMomentum(solo.parameters(), lr=0.05, momentum=0.9)
    for x, y in zip(xs, ys):
        opt.zero_grad()
        _loss(solo(x), y).backward()
        opt.step()

    st = prepare_training(model, None, devices=[0, 1], opt_factory=_sgd(),
                          grad_sync="flat")
    train(_loss, st, steps=3, log_every=0, val_every=0,
          batches=lambda j: [(xs[j][:2], ys[j][:2]), (xs[j][2:], ys[j][2:])])

    for (k, p_solo), (_, p_ddp) in zip(
        solo.named_parameters(), st.replicas[0].model.named_parameters()
    ):
        assert torch.allclose(p_solo, p_ddp, rtol=1e-4, atol=1e-5), k


def test_flat_matches_tree_mode_exactly(seed):
    """fp32 on the CPU: both modes apply the same arithmetic, so three steps
    end in bit-identical parameters."""
    out = {}
    for mode in ("tree", "flat"):
        st = prepare_training(_mlp(3), None, devices=[0, 1, 2],
                              opt_factory=_sgd(), grad_sync=mode)
        train(_loss, st, steps=3, batches=_batches(3), log_every=0,
              val_every=0)
        out[mode] = [p.detach().clone()
                     for p in st.replicas[0].model.parameters()]
    for a, b in zip(out["tree"], out["flat"]):
        assert torch.equal(a, b)


def test_flat_replicas_stay_in_sync(seed):
    st = prepare_training(_mlp(), None, devices=[0, 1, 2], opt_factory=_sgd(),
                          grad_sync="flat")
    train(_loss, st, steps=3, batches=_batches(3), log_every=1, val_every=0)
    trees = [{k: p.detach() for k, p in r.model.named_parameters()}
             for r in st.replicas]
    assert ensure_synced(trees, rtol=0, atol=0)
    assert st.nonfinite_steps == 0
    assert st.cycles == 3


def test_non_flat_optimizer_is_refused():
    with pytest.raises(ValueError, match=r"replica 0.*SGD"):
        prepare_training(
            _mlp(), None, devices=[0, 1], grad_sync="flat",
            opt_factory=lambda m: torch.optim.SGD(m.parameters(), lr=0.1))


def test_mismatched_layout_is_refused():
    a, b = _mlp(), nn.Sequential(nn.Flatten(), nn.Linear(12, 4))
    reps = [Replica(0, 0, a, FusedSGDMomentum(a.parameters(), lr=0.1)),
            Replica(1, 1, b, FusedSGDMomentum(b.parameters(), lr=0.1))]
    with pytest.raises(ValueError, match="replica 1"):
        FlatGradReducer(reps)
    c = _mlp().bfloat16()
    reps[1] = Replica(1, 1, c, FusedSGDMomentum(c.parameters(), lr=0.1))
    with pytest.raises(ValueError, match="replica 1"):
        FlatGradReducer(reps)


def test_unknown_grad_sync_is_refused():
    with pytest.raises(ValueError, match="grad_sync"):
        prepare_training(_mlp(), None, devices=[0], opt_factory=_sgd(),
                         grad_sync="ring")


def test_pop_nonfinite(seed):
    st = prepare_training(_mlp(), None, devices=[0, 1], opt_factory=_sgd(),
                          grad_sync="flat")
    red = st.reducer
    for r in st.replicas:
        r.optimizer.groups[0].G.normal_()
    red.reduce()
    assert red.pop_nonfinite() is False
    st.replicas[1].optimizer.groups[0].G[5] = float("nan")
    red.reduce()
    assert red.pop_nonfinite() is True
    assert red.pop_nonfinite() is False   # cleared by the read


def test_train_counts_nonfinite_steps(seed):
    st = prepare_training(_mlp(), None, devices=[0, 1], opt_factory=_sgd(),
                          grad_sync="flat")

    def batches(j):
        xs = _batches(2)(j)
        if j == 1:
            xs[0][0][0, 0, 0, 0] = float("inf")
        return xs

    train(_loss, st, steps=2, batches=batches, log_every=1, val_every=0)
    assert st.nonfinite_steps == 1


def test_flat_oom_skip_counts_missed(seed, monkeypatch):
    st = prepare_training(_mlp(), None, devices=[0, 1],
                          opt_factory=_sgd(0.1, 0.0), grad_sync="flat")
    calls = {"n": 0}
    real_step = train_step

    def flaky(loss_fn, buffer, replica, x, y):
        calls["n"] += 1
        if calls["n"] == 1:
            raise RuntimeError("HIP out of memory: simulated")
        return real_step(loss_fn, buffer, replica, x, y)

    monkeypatch.setattr("fluxdistributed_amd.parallel.task_ddp.train_step", flaky)
    before = [p.detach().clone() for p in st.replicas[0].model.parameters()]
    train(_loss, st, steps=1, log_every=0, val_every=0, batches=_batches(2))
    assert st.num_missed == 1
    # the skipped batch took no optimizer step
    for a, p in zip(before, st.replicas[0].model.parameters()):
        assert torch.equal(a, p.detach())
    train(_loss, st, steps=1, log_every=0, val_every=0, batches=_batches(2))
    assert st.num_missed == 1 and st.cycles == 2


def test_train_cli_flat(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ckdir = tmp_path / "w"
    cmd = [sys.executable, os.path.join(root, "train.py"),
           "--mode", "task", "--grad-sync", "flat", "--devices", "2",
           "--model", "resnet18", "--small-input", "--steps", "2",
           "--batch", "4", "--image-size", "32", "--num-classes", "8",
           "--dtype", "fp32", "--data", "synthetic",
           "--checkpoint-dir", str(ckdir), "--log-every", "1",
           "--val-every", "0"]
    # the CPU contract on every machine: hide any GPU from the child
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (ckdir / "resnet18_final.pt").exists()
