#!/usr/bin/env python3
"""Host vs device image preprocessing throughput.

For a batch of synthetic uint8 images (default 96 of 375x500) it measures
  1. the CPU path (`preprocess` + per-image standardize on a thread pool,
     as `imagenet._fproc` runs it after the decode), in images/s;
  2. the device path: ms per batch of H2D + kernels for
     `preprocess_batch(standardize=True)` from a pinned RawBatch, timed with
     device events after warm-up, plus kernels alone (arena already on the
     device) and the host-side `pack_images` that stays on the loader
     thread;
  3. both again with real PIL JPEG decode, through `minibatch` and
     `minibatch_raw` on a generated temporary ILSVRC tree.
Prints one JSON line (and writes it to --out). The device numbers need a
GPU; --rehearse runs the host parts only and reports the rest as null.
"""

import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fluxdistributed_amd.data import imagenet  # noqa: E402
from fluxdistributed_amd.data.preprocess import (  # noqa: E402
    pack_images, preprocess, preprocess_batch,
)


def synth_images(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([yy / (h - 1), xx / (w - 1),
                     1.0 - (yy + xx) / (h + w - 2)], axis=-1) * 255.0
    return [(0.6 * base + 0.4 * rng.integers(0, 256, size=(h, w, 3)))
            .astype(np.uint8) for _ in range(n)]


def cpu_one(img, out_view, crop, resize):
    """What imagenet._fproc does after the decode."""
    arr = img.astype(np.float32) / 255.0
    x = preprocess(torch.from_numpy(arr).permute(2, 0, 1), crop=crop,
                   resize=resize)
    out_view.copy_((x - x.mean()) / (x.std() + 1e-5))


def time_host(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t0) / iters


def time_device(fn, iters, warmup):
    """ms per call from device events; the window holds `iters` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def make_tree(root, images):
    from PIL import Image

    syn = "n01440764"
    with open(os.path.join(root, "LOC_synset_mapping.txt"), "w") as f:
        f.write(f"{syn} tench\n")
    d = os.path.join(root, "ILSVRC", "Data", "CLS-LOC", "train", syn)
    os.makedirs(d)
    nbytes = 0
    with open(os.path.join(root, "LOC_train_solution.csv"), "w") as f:
        f.write("ImageId,PredictionString\n")
        for i, img in enumerate(images):
            path = os.path.join(d, f"{syn}_{i}.JPEG")
            Image.fromarray(img).save(path, quality=90)
            nbytes += os.path.getsize(path)
            f.write(f"{syn}_{i},{syn} 1 2 3 4\n")
    return nbytes / len(images)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=96)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--width", type=int, default=500)
    ap.add_argument("--resize", type=int, default=256)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--num-workers", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200,
                    help="timed device batches")
    ap.add_argument("--host-iters", type=int, default=5,
                    help="timed host batches")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--rehearse", action="store_true",
                    help="host parts only; device numbers reported as null")
    ap.add_argument("--device-only", action="store_true",
                    help="skip the host measurements (for profiler runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    workers = max(1, min(a.num_workers, 16))
    gpu = torch.cuda.is_available()
    if not gpu and not a.rehearse:
        sys.exit("bench_preprocess: no GPU (use --rehearse for the host "
                 "parts only)")
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    imgs = synth_images(a.batch, a.height, a.width)
    B = a.batch
    res = {"batch": B, "image": [a.height, a.width], "resize": a.resize,
           "crop": a.crop, "num_workers": workers, "dtype": a.dtype,
           "torch_threads": torch.get_num_threads()}

    # 1. CPU path, no decode
    x = torch.zeros(B, 3, a.crop, a.crop)

    def cpu_batch():
        with ThreadPoolExecutor(max_workers=workers) as pool:
            for f in [pool.submit(cpu_one, imgs[i], x[i], a.crop, a.resize)
                      for i in range(B)]:
                f.result()

    res["cpu_img_per_s"] = res["pack_ms_per_batch"] = None
    if not a.device_only:
        res["cpu_img_per_s"] = B / time_host(cpu_batch, a.host_iters, 1)
        # host side of the device path: the byte copy into the arena
        res["pack_ms_per_batch"] = 1e3 * time_host(
            lambda: pack_images(imgs, a.resize, a.crop), a.host_iters, 1)

    # 2. device path
    res["device_ms_per_batch_h2d_kernels"] = None
    res["device_ms_per_batch_kernels"] = None
    res["arena_mb"] = None
    if gpu:
        dev = torch.device("cuda:0")
        raw = pack_images(imgs, a.resize, a.crop, pin=True)
        res["arena_mb"] = raw.arena.numel() / 1e6
        res["device_ms_per_batch_h2d_kernels"] = time_device(
            lambda: preprocess_batch(raw, device=dev, standardize=True,
                                     dtype=dtype), a.iters, a.warmup)
        rawd = raw.to(dev)
        res["device_ms_per_batch_kernels"] = time_device(
            lambda: preprocess_batch(rawd, standardize=True, dtype=dtype),
            a.iters, a.warmup)
        ms = res["device_ms_per_batch_h2d_kernels"]
        res["device_img_per_s"] = B / (ms * 1e-3)

    # 3. with JPEG decode
    if a.device_only:
        print(json.dumps(res))
        return
    with tempfile.TemporaryDirectory() as root:
        res["jpeg_kb_per_image"] = make_tree(root, imgs) / 1e3
        key = imagenet.train_solutions(root)
        ids = list(range(B))
        if (a.resize, a.crop) == (256, 224):   # minibatch's fixed geometry
            res["cpu_decode_img_per_s"] = B / time_host(
                lambda: imagenet.minibatch(root, key, ids=ids,
                                           num_workers=workers),
                a.host_iters, 1)
        else:
            res["cpu_decode_img_per_s"] = None

        def raw_batch():
            return imagenet.minibatch_raw(root, key, ids=ids,
                                          num_workers=workers,
                                          resize=a.resize, crop=a.crop)

        t_raw = time_host(raw_batch, a.host_iters, 1)
        res["decode_pack_img_per_s"] = B / t_raw
        res["device_decode_img_per_s"] = None
        if gpu:
            # host decode + pack, then pin + H2D + kernels, end to end and
            # unpipelined (one thread does both, with a device sync)
            def full():
                r, _ = raw_batch()
                preprocess_batch(r.pin_memory(), device=dev,
                                 standardize=True, dtype=dtype)
                torch.cuda.synchronize()

            res["device_decode_img_per_s"] = B / time_host(
                full, a.host_iters, 1)

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
