"""Batched preprocessing on the CPU: the math contract against a float64
oracle, image packing, the CPU fallback of `preprocess_batch`, the raw
ImageNet minibatch and the loader's device_transform hook."""

import numpy as np
import pytest
import torch

from preprocess_oracle import CASES, case_id, case_image, make_image, oracle

from fluxdistributed_amd import data as fdata
from fluxdistributed_amd.data import imagenet
from fluxdistributed_amd.data.loader import PrefetchLoader
from fluxdistributed_amd.data.preprocess import (
    META_INTS, RawBatch, image_geometry, pack_images, preprocess,
    preprocess_batch, resize_smallest_dimension,
)


def _chw(img):
    """HWC uint8 ndarray -> CHW float [0,1], the way imagenet._fproc does."""
    return torch.from_numpy(img.astype(np.float32) / 255.0).permute(2, 0, 1)


def _standardize(x):
    return (x - x.mean()) / (x.std() + 1e-5)


# ---- the yardstick itself --------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cpu_preprocess_matches_float64_oracle(case):
    """The existing CPU pipeline is the composed separable form of the math
    contract: within 2e-4 of the dense float64 oracle (3x the 6.7e-5 seen
    when the contract was written), before and after standardize."""
    h, w, crop, resize = case
    img = case_image(case)
    x = preprocess(_chw(img), crop=crop, resize=resize)
    ref = oracle(img, resize, crop)
    assert ref.std() >= 0.1
    err = np.abs(x.double().numpy() - ref).max()
    xs = _standardize(x)
    errs = np.abs(xs.double().numpy()
                  - oracle(img, resize, crop, standardize=True)).max()
    print(f"{case_id(case)}: max err {err:.3g}, standardized {errs:.3g}")
    assert err <= 2e-4
    assert errs <= 2e-4


# ---- packing ---------------------------------------------------------------

RAGGED = [(20, 31), (33, 47), (97, 61), (32, 32), (5, 7)]


def test_pack_images_roundtrip_and_alignment():
    imgs = [make_image(h, w, seed=i) for i, (h, w) in enumerate(RAGGED)]
    # tensors and ndarrays both pack
    mixed = [torch.from_numpy(a) if i % 2 else a for i, a in enumerate(imgs)]
    raw = pack_images(mixed, resize=4, crop=3)
    assert isinstance(raw, RawBatch)
    assert (raw.n, raw.resize, raw.crop) == (len(imgs), 4, 3)
    assert raw.arena.dtype == torch.uint8 and raw.arena.dim() == 1
    assert raw.meta.dtype == torch.int32
    assert tuple(raw.meta.shape) == (len(imgs), META_INTS)
    offs = raw.meta[:, :2].contiguous().view(torch.int64).flatten().tolist()
    end = 0
    for i, a in enumerate(imgs):
        assert offs[i] % 16 == 0
        assert offs[i] >= end            # images do not overlap
        end = offs[i] + a.size
        assert np.array_equal(raw.image(i).numpy(), a)
        assert raw.meta[i, 2:4].tolist() == list(a.shape[:2])
    assert end <= raw.arena.numel()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_pack_geometry_matches_resize(case):
    h, w, crop, resize = case
    raw = pack_images([case_image(case)], resize=resize, crop=crop)
    _, _, nh, nw, top, left, r = raw.meta[0, 2:9].tolist()
    resized = resize_smallest_dimension(torch.zeros(3, h, w), resize)
    assert (nh, nw) == tuple(resized.shape[1:])
    assert (top, left) == ((nh - crop) // 2, (nw - crop) // 2)
    scale = resize / min(h, w)
    if scale < 1.0:
        sigma = 0.75 / scale
        assert r == max(1, int(np.ceil(3.0 * sigma)))
        got = raw.meta[0, 9:10].view(torch.float32).item()
        assert got == np.float32(sigma)
    else:
        assert r == 0
    assert image_geometry(h, w, resize, crop)[:5] == (nh, nw, top, left, r)


def test_pack_rejects_radius_not_smaller_than_image():
    # 8x200 -> resize 2: scale 0.25, sigma 3, r = 9 >= min(h, w) = 8
    with pytest.raises(ValueError, match="radius"):
        pack_images([make_image(8, 200, 0)], resize=2, crop=2)
    # 10x200 -> resize 2: sigma 3.75, r = 12 >= 10 as well
    with pytest.raises(ValueError, match="radius"):
        pack_images([make_image(10, 200, 0)], resize=2, crop=2)
    # 40x200 -> resize 4: sigma 7.5, r = 23 < 40 packs
    assert pack_images([make_image(40, 200, 0)], resize=4, crop=2).n == 1


def test_pack_rejects_crop_larger_than_resize():
    with pytest.raises(ValueError, match="crop"):
        pack_images([make_image(40, 40, 0)], resize=32, crop=33)


def test_pack_rejects_non_uint8_hwc():
    with pytest.raises(ValueError):
        pack_images([np.zeros((3, 8, 8), dtype=np.uint8)], resize=4, crop=4)
    with pytest.raises(ValueError):
        pack_images([np.zeros((8, 8, 3), dtype=np.float32)], resize=4, crop=4)


# ---- CPU preprocess_batch --------------------------------------------------

@pytest.mark.parametrize("standardize", [False, True])
def test_cpu_preprocess_batch_equals_per_image_bitwise(standardize):
    group = [c for c in CASES if c[2:] == (24, 32)]
    imgs = [case_image(c) for c in group]
    raw = pack_images(imgs, resize=32, crop=24)
    out = preprocess_batch(raw, standardize=standardize)
    assert out.shape == (len(imgs), 3, 24, 24)
    assert out.dtype == torch.float32 and out.device.type == "cpu"
    assert out.is_contiguous(memory_format=torch.channels_last)
    assert out.stride() == (3 * 24 * 24, 1, 3 * 24, 3)
    for i, img in enumerate(imgs):
        x = preprocess(_chw(img), crop=24, resize=32)
        if standardize:
            x = _standardize(x)
        assert torch.equal(out[i], x)


def test_cpu_preprocess_batch_dtype_and_normalize_flag():
    img = case_image((32, 32, 24, 32))
    raw = pack_images([img], resize=32, crop=24)
    plain = preprocess_batch(raw, normalize=False)
    assert torch.equal(plain[0], preprocess(_chw(img), crop=24, resize=32,
                                            normalize=False))
    bf = preprocess_batch(raw, dtype=torch.bfloat16)
    assert bf.dtype == torch.bfloat16
    assert bf.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(bf, preprocess_batch(raw).to(torch.bfloat16))
    with pytest.raises(ValueError):
        preprocess_batch(raw, dtype=torch.float16)


def test_native_binding_refuses_cpu_tensors():
    """Like the conv entry points: host tensors are refused by the operand
    check, before any launch could see a host pointer."""
    from fluxdistributed_amd.ops.native import require_native

    C = require_native("preprocess_batch")
    raw = pack_images([make_image(20, 31, 0)], resize=32, crop=24)
    with pytest.raises(RuntimeError, match="device tensors required"):
        C.preprocess_batch(raw.arena, raw.meta, 24, True, False, False)


def test_new_names_exported():
    import fluxdistributed_amd as pkg

    for name in ("RawBatch", "pack_images", "preprocess_batch",
                 "minibatch_raw"):
        assert hasattr(pkg, name), name
        assert hasattr(fdata, name), name


# ---- raw ImageNet minibatch ------------------------------------------------

@pytest.fixture
def fake_imagenet(tmp_path):
    """Two-class ILSVRC tree, built as in tests/test_data.py."""
    root = tmp_path
    (root / "LOC_synset_mapping.txt").write_text(
        "n01440764 tench, Tinca tinca\nn01443537 goldfish\n"
    )
    (root / "LOC_train_solution.csv").write_text(
        "ImageId,PredictionString\n"
        "n01440764_10026,n01440764 1 2 3 4\n"
        "n01443537_200,n01443537 5 6 7 8\n"
    )
    from PIL import Image

    rng = np.random.default_rng(3)
    for img_id, (h, w) in [("n01440764_10026", (64, 80)),
                           ("n01443537_200", (300, 280))]:
        syn = img_id.split("_")[0]
        d = root / "ILSVRC" / "Data" / "CLS-LOC" / "train" / syn
        d.mkdir(parents=True, exist_ok=True)
        arr = (rng.random((h, w, 3)) * 255).astype(np.uint8)
        Image.fromarray(arr).save(d / f"{img_id}.JPEG")
    return str(root)


def test_minibatch_raw_plus_cpu_transform_equals_minibatch(fake_imagenet):
    key = imagenet.train_solutions(fake_imagenet)
    ids = [1, 0, 0, 1]
    x, y = imagenet.minibatch(fake_imagenet, key, ids=ids)
    raw, yr = imagenet.minibatch_raw(fake_imagenet, key, ids=ids)
    assert isinstance(raw, RawBatch) and raw.n == 4
    assert (raw.resize, raw.crop) == (256, 224)
    assert torch.equal(y, yr)
    xr = preprocess_batch(raw, standardize=True)
    assert xr.shape == x.shape
    assert torch.equal(xr, x)


def test_minibatch_raw_samples_like_minibatch(fake_imagenet):
    import random

    key = imagenet.train_solutions(fake_imagenet)
    _, y = imagenet.minibatch(fake_imagenet, key, nsamples=6,
                              rng=random.Random(11))
    raw, yr = imagenet.minibatch_raw(fake_imagenet, key, nsamples=6,
                                     rng=random.Random(11))
    assert raw.n == 6 and torch.equal(y, yr)


# ---- loader ----------------------------------------------------------------

def test_prefetch_loader_calls_device_transform_on_cpu():
    imgs = [make_image(20, 31, s) for s in range(3)]
    calls = []

    def make():
        return pack_images(imgs, resize=32, crop=24), torch.arange(3)

    def transform(raw, device):
        calls.append((raw, device))
        return preprocess_batch(raw, standardize=True)

    ld = PrefetchLoader(make, device=None, buffersize=2,
                        device_transform=transform)
    x, y = next(ld)
    x2, _ = next(ld)
    ld.close()
    assert len(calls) == 2
    assert isinstance(calls[0][0], RawBatch) and calls[0][1] is None
    want = preprocess_batch(pack_images(imgs, resize=32, crop=24),
                            standardize=True)
    assert torch.equal(x, want) and torch.equal(x2, want)
    assert y.tolist() == [0, 1, 2]


def test_prefetch_loader_without_transform_is_unchanged():
    calls = {"n": 0}

    def make():
        calls["n"] += 1
        return (torch.full((2, 3), float(calls["n"])),
                torch.zeros(2, dtype=torch.long))

    ld = PrefetchLoader(make, device=None, buffersize=3)
    assert ld.device_transform is None
    out = [next(ld) for _ in range(4)]
    ld.close()
    assert [float(x[0, 0]) for x, _ in out] == [1.0, 2.0, 3.0, 4.0]
    assert all(isinstance(x, torch.Tensor) and x.shape == (2, 3)
               for x, _ in out)


def test_train_py_device_preprocess_batch_fn(fake_imagenet, monkeypatch):
    """--device-preprocess: the batch function hands out raw batches and the
    loader transform turns them into what the plain path yields."""
    import fluxdistributed_amd.data.registry as reg
    import train as train_mod

    monkeypatch.setattr(reg, "dataset", lambda name: str(fake_imagenet))

    class A:
        data = str(fake_imagenet)
        classes = None
        nsamples = 2
        batch = 2
        seed = 5
        dtype = "fp32"
        num_classes = 10
        image_size = 224
        device_preprocess = True

    raw, y = train_mod.make_batch_fn(A())()
    assert isinstance(raw, RawBatch) and raw.n == 2
    tf = train_mod.make_device_transform(A())
    x = tf(raw, torch.device("cpu"))
    assert x.shape == (2, 3, 224, 224) and x.dtype == torch.float32
    assert torch.equal(x, preprocess_batch(raw, standardize=True))

    A.device_preprocess = False
    assert train_mod.make_device_transform(A()) is None
    xs, _ = train_mod.make_batch_fn(A())()
    assert isinstance(xs, torch.Tensor)
    A.device_preprocess = True
    A.data = "synthetic"          # the flag has no effect on synthetic data
    assert train_mod.make_device_transform(A()) is None
