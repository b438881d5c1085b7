"""Device-side preprocessing (csrc/preprocess.hip) against the float64
oracle of the math contract, plus the loader and graph-engine plumbing
around it."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("GPU-only suite", allow_module_level=True)

from preprocess_oracle import CASES, case_id, case_image, make_image, oracle

from fluxdistributed_amd.data.loader import PrefetchLoader
from fluxdistributed_amd.data.preprocess import pack_images, preprocess_batch

DEV = torch.device("cuda:0")
GROUPS = sorted({c[2:] for c in CASES})          # distinct (crop, resize)


def _group(crop, resize):
    return [c for c in CASES if c[2:] == (crop, resize)]


@pytest.fixture(scope="module")
def refs():
    """Float64 oracle per case, computed once: (plain, standardized), both
    ImageNet-normalized. Read-only."""
    out = {}
    for case in CASES:
        _, _, crop, resize = case
        v = oracle(case_image(case), resize, crop)
        assert v.std() >= 0.1
        vs = (v - v.mean()) / (v.std(ddof=1) + 1e-5)
        v.setflags(write=False)
        vs.setflags(write=False)
        out[case] = (v, vs)
    return out


@pytest.fixture(scope="module")
def singles():
    """Every case run alone through the device path: case -> {standardize:
    fp32 output [1,3,crop,crop]}."""
    out = {}
    for case in CASES:
        _, _, crop, resize = case
        raw = pack_images([case_image(case)], resize=resize, crop=crop)
        out[case] = {s: preprocess_batch(raw, device=DEV, standardize=s)
                     for s in (False, True)}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_single_image_matches_oracle(case, refs, singles):
    _, _, crop, _ = case
    for standardize in (False, True):
        got = singles[case][standardize]
        assert got.shape == (1, 3, crop, crop)
        assert got.dtype == torch.float32 and got.device == DEV
        assert got.stride() == (3 * crop * crop, 1, 3 * crop, 3)
        err = np.abs(got[0].double().cpu().numpy()
                     - refs[case][int(standardize)]).max()
        print(f"{case_id(case)} standardize={standardize}: max err {err:.3g}")
        assert err <= 2e-4


def test_identity_scale_is_exact_crop():
    """32x32 -> resize 32: lambda is exactly 0 and there is no blur, so the
    raw output is the cropped pixels / 255."""
    case = (32, 32, 24, 32)
    img = case_image(case)
    raw = pack_images([img], resize=32, crop=24)
    got = preprocess_batch(raw, device=DEV, normalize=False)
    ref = oracle(img, 32, 24, normalize=False)
    assert np.array_equal(ref, img[4:28, 4:28].transpose(2, 0, 1) / 255.0)
    err = np.abs(got[0].double().cpu().numpy() - ref).max()
    print(f"identity: max err {err:.3g}")
    assert err <= 1e-6


@pytest.mark.parametrize("crop,resize", GROUPS)
@pytest.mark.parametrize("standardize", [False, True])
def test_ragged_batch_equals_singles_bitwise(crop, resize, standardize,
                                             singles):
    """No leakage between images through offsets or the partials."""
    group = _group(crop, resize)
    raw = pack_images([case_image(c) for c in group], resize=resize,
                      crop=crop)
    got = preprocess_batch(raw, device=DEV, standardize=standardize)
    assert got.shape == (len(group), 3, crop, crop)
    assert got.is_contiguous(memory_format=torch.channels_last)
    for i, case in enumerate(group):
        assert torch.equal(got[i], singles[case][standardize][0]), case


@pytest.mark.parametrize("crop,resize", GROUPS)
def test_bf16_is_the_rounded_fp32_and_runs_repeat(crop, resize):
    group = _group(crop, resize)
    raw = pack_images([case_image(c) for c in group], resize=resize,
                      crop=crop).to(DEV)
    for standardize in (False, True):
        f32 = preprocess_batch(raw, standardize=standardize)
        again = preprocess_batch(raw, standardize=standardize)
        bf = preprocess_batch(raw, standardize=standardize,
                              dtype=torch.bfloat16)
        assert bf.dtype == torch.bfloat16
        assert bf.stride() == f32.stride()
        assert torch.equal(f32, again)
        assert torch.equal(bf, f32.to(torch.bfloat16))


def test_odd_crop_takes_the_unaligned_store_path():
    """crop 23: 3*23*23 elements per image is no multiple of 4 or 8, so
    every image but the first starts off a 16-byte boundary (scalar head
    and tail around the vector body)."""
    imgs = [make_image(h, w, seed=h) for h, w in
            [(50, 41), (33, 47), (97, 61), (64, 64), (31, 90)]]
    raw = pack_images(imgs, resize=32, crop=23).to(DEV)
    for standardize in (False, True):
        f32 = preprocess_batch(raw, standardize=standardize)
        bf = preprocess_batch(raw, standardize=standardize,
                              dtype=torch.bfloat16)
        assert torch.equal(bf, f32.to(torch.bfloat16))
        for i, img in enumerate(imgs):
            ref = oracle(img, 32, 23, standardize=standardize)
            err = np.abs(f32[i].double().cpu().numpy() - ref).max()
            assert err <= 2e-4, (i, err)


def test_device_resident_raw_batch_is_not_copied():
    case = (20, 31, 24, 32)
    raw = pack_images([case_image(case)], resize=32, crop=24).to(DEV)
    assert raw.arena.device == DEV and raw.meta.device == DEV
    assert raw.arena.to(DEV).data_ptr() == raw.arena.data_ptr()
    out = preprocess_batch(raw)           # device taken from the arena
    assert out.device == DEV


def test_work_stays_on_the_current_stream(refs):
    """Called under a side stream, everything (upload, kernels, the
    allocations' stream ownership) belongs to that stream: syncing it alone
    completes the result, and the default stream never saw any work."""
    case = (300, 401, 24, 32)
    raw = pack_images([case_image(case)], resize=32, crop=24, pin=True)
    assert raw.arena.is_pinned() and raw.meta.is_pinned()
    torch.cuda.synchronize()
    default = torch.cuda.default_stream(DEV)
    side = torch.cuda.Stream(DEV)
    marker = torch.cuda.Event()
    marker.record(default)
    with torch.cuda.stream(side):
        out = preprocess_batch(raw, device=DEV, standardize=True)
    side.synchronize()
    assert default.query() and marker.query()
    err = np.abs(out[0].double().cpu().numpy() - refs[case][1]).max()
    assert err <= 2e-4


def _loader_batches():
    """Four different ragged (crop 32) batches of four images each."""
    sizes = [(33, 47), (300, 401), (40, 36), (97, 61), (64, 80), (32, 32)]
    out = []
    for b in range(4):
        imgs = [make_image(*sizes[(b + i) % len(sizes)], seed=10 * b + i)
                for i in range(4)]
        out.append((imgs, torch.tensor([(b + i) % 16 for i in range(4)])))
    return out


def _standardized(raw, device):
    return preprocess_batch(raw, device=device, standardize=True,
                            dtype=torch.bfloat16)


def test_prefetch_loader_device_transform_equals_direct_calls():
    batches = _loader_batches()
    it = iter(range(10_000))

    def make():
        imgs, y = batches[next(it) % 4]
        return pack_images(imgs, resize=32, crop=32), y

    loader = PrefetchLoader(make, device=DEV, buffersize=2,
                            device_transform=_standardized)
    got = [next(loader) for _ in range(4)]
    torch.cuda.synchronize()
    loader.close()
    for (x, y), (imgs, yh) in zip(got, batches):
        want = _standardized(pack_images(imgs, resize=32, crop=32), DEV)
        assert x.device == DEV and y.device == DEV
        assert x.dtype == torch.bfloat16
        assert x.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(x, want)
        assert torch.equal(y.cpu(), yh)


def test_graphed_train_step_fed_by_the_transforming_loader():
    from fluxdistributed_amd.engine import GraphedTrainStep, make_train_step
    from fluxdistributed_amd.models import build_model
    from fluxdistributed_amd.ops import FusedSGDMomentum, logit_cross_entropy
    from fluxdistributed_amd.utils.precision import to_mixed_bf16

    torch.manual_seed(7)
    model = build_model("resnet18", num_classes=16, small_input=True).cuda() \
        .to(memory_format=torch.channels_last)
    model = to_mixed_bf16(model).train()
    opt = FusedSGDMomentum(model.parameters(), lr=0.05, momentum=0.9)
    batches = _loader_batches()
    it = iter(range(10_000))

    def make():
        imgs, y = batches[next(it) % 4]
        return pack_images(imgs, resize=32, crop=32), y

    loader = PrefetchLoader(make, device=DEV, buffersize=2,
                            device_transform=_standardized)
    example = next(loader)
    step = make_train_step(model, opt, logit_cross_entropy,
                           example_batch=example, use_graph=True)
    assert isinstance(step, GraphedTrainStep)
    x, y = next(loader)
    loss = step(x, y)
    torch.cuda.synchronize()
    loader.close()
    assert torch.isfinite(loss.float()).item()


def test_untrusted_meta_row_yields_nans_for_that_image_only(singles):
    """The meta table is device memory the host checks cannot see. A row
    the kernel cannot trust (here r == min(h, w), which the reflect border
    does not allow) gives NaNs for that image and leaves its neighbours
    alone."""
    group = _group(24, 32)
    raw = pack_images([case_image(c) for c in group], resize=32, crop=24)
    bad = 1
    raw.meta[bad, 8] = int(min(raw.meta[bad, 2], raw.meta[bad, 3]))
    for standardize in (False, True):
        got = preprocess_batch(raw, device=DEV, standardize=standardize)
        assert torch.isnan(got[bad]).all()
        for i, case in enumerate(group):
            if i != bad:
                assert torch.equal(got[i], singles[case][standardize][0])


def test_binding_rejects_bad_operands():
    from fluxdistributed_amd.ops.native import require_native

    C = require_native("preprocess_batch")
    raw = pack_images([make_image(20, 31, 0)], resize=32, crop=24)
    with pytest.raises(RuntimeError, match="device tensors required"):
        C.preprocess_batch(raw.arena, raw.meta, 24, True, False, False)
    d = raw.to(DEV)
    with pytest.raises(RuntimeError, match="meta must be"):
        C.preprocess_batch(d.arena, d.meta[:, :9].contiguous(), 24, True,
                           False, False)
    with pytest.raises(RuntimeError, match="arena must be"):
        C.preprocess_batch(d.arena.to(torch.int8), d.meta, 24, True, False,
                           False)
