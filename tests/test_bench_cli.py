"""bench.py command line: the result line, --full, and --dump-outputs
(same arguments -> same inputs -> comparable .npy outputs)."""

import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 4


def _bench(outdir, steps, warmup, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
           "--steps", str(steps), "--warmup", str(warmup), "--allow-cpu",
           "--model", "resnet18", "--batch", str(BATCH), "--image-size", "32",
           "--num-classes", "8", "--dtype", "fp32",
           "--dump-outputs", str(outdir), *extra]
    # CPU on every machine (an out-of-range ordinal leaves HIP no devices):
    # this checks the command line's plumbing, and CPU steps are exactly
    # repeatable, so the runs below must agree to rounding.
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == steps and res["warmup"] == warmup
    assert res["ms_per_step"] > 0
    # value is images/sec over exactly --steps steps of --batch images
    assert abs(res["value"] * res["ms_per_step"] / 1e3 - BATCH) < 0.01 * BATCH
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in res
    return res


def _load(d):
    return {n: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_bench_dump_outputs_repeatable(tmp_path):
    a = _bench(tmp_path / "a", 2, 1)
    _bench(tmp_path / "b", 2, 1, "--full")
    # the last timed step starts from the seeded initial state, so a run
    # whose last step sees the same batch (3rd of the pool) by another
    # split of warm-up and timed steps writes the same files
    _bench(tmp_path / "c", 3, 0)
    xa, xb, xc = (_load(tmp_path / d) for d in "abc")
    assert list(xa) == list(xb) == list(xc) == ["loss.npy", "params.npy"]
    for n, x in xa.items():
        assert x.dtype == np.float32 and np.isfinite(x).all()
        # one fp32 CPU step from identical state and batch; the slack is
        # for thread-count-dependent summation order in the CPU kernels
        np.testing.assert_allclose(x, xb[n], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(x, xc[n], rtol=1e-4, atol=1e-5)
    assert sum(x.nbytes for x in xa.values()) <= 64 * 2**20
    assert abs(float(xa["loss.npy"][0]) - a["final_loss"]) < 1e-3
