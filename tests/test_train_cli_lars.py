"""train.py with --optimizer lars and the warm-up schedule, task mode on the
CPU with 2 logical devices (the invocation of test_train_cli.py)."""

import os
import subprocess
import sys


def test_train_cli_lars_warmup_poly(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ckdir = tmp_path / "w"
    cmd = [sys.executable, os.path.join(root, "train.py"),
           "--mode", "task", "--devices", "2", "--model", "resnet18",
           "--small-input", "--steps", "2", "--batch", "4",
           "--image-size", "32", "--num-classes", "8", "--dtype", "fp32",
           "--data", "synthetic", "--checkpoint-dir", str(ckdir),
           "--log-every", "1", "--val-every", "0",
           "--optimizer", "lars", "--lr-schedule", "warmup-poly",
           "--warmup-steps", "1"]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "grad_norm=" in r.stderr and "skipped_steps=0" in r.stderr

    import torch

    ck = torch.load(ckdir / "resnet18_final.pt", map_location="cpu",
                    weights_only=False)
    assert "model" in ck
    opt = ck["optimizer"]
    assert opt["skipped_steps"] == 0
    V = opt["flat_state"][0]["V"]
    # step 1 ran at lr 0 (start of the ramp), step 2 at --lr: momentum moved
    assert V.abs().sum() > 0
    # the schedule reached the end of the run: (1 - t)^2 = 0
    assert opt["param_groups"][0]["lr"] == 0.0
