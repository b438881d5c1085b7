"""Image preprocessing (reference /root/reference/src/preprocess.jl:26-81):
resize smallest dimension to 256 with Gaussian lowpass when downscaling,
center-crop 224, ImageNet mean/std normalize. Implemented on torch CPU
tensors (CHW float in [0,1]).

`pack_images` / `preprocess_batch` are the batched form over raw uint8
images: the same pipeline as one HIP kernel on a GPU (csrc/preprocess.hip),
the per-image CPU pipeline elsewhere."""

import math
from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from ..utils.device import is_real_gpu

IMAGENET_MEAN = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
IMAGENET_STD = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)


def _gaussian_kernel1d(sigma: float) -> torch.Tensor:
    radius = max(1, int(math.ceil(3.0 * sigma)))
    x = torch.arange(-radius, radius + 1, dtype=torch.float32)
    k = torch.exp(-(x ** 2) / (2 * sigma * sigma))
    return k / k.sum()


def resize_smallest_dimension(img: torch.Tensor, target: int = 256) -> torch.Tensor:
    """Resize so min(H, W) == target; Gaussian lowpass before downscaling
    (reference preprocess.jl:30-42 uses σ = 0.75 * inv_scale)."""
    c, h, w = img.shape
    scale = target / min(h, w)
    nh, nw = max(target, round(h * scale)), max(target, round(w * scale))
    x = img.unsqueeze(0)
    if scale < 1.0:
        sigma = 0.75 / scale
        k = _gaussian_kernel1d(sigma).to(img.dtype)
        r = (len(k) - 1) // 2
        kx = k.view(1, 1, 1, -1).expand(c, 1, 1, -1)
        ky = k.view(1, 1, -1, 1).expand(c, 1, -1, 1)
        x = F.pad(x, (r, r, r, r), mode="reflect")
        x = F.conv2d(x, ky, groups=c)
        x = F.conv2d(x, kx, groups=c)
    x = F.interpolate(x, size=(nh, nw), mode="bilinear", align_corners=False,
                      antialias=False)
    return x.squeeze(0)


def center_crop(img: torch.Tensor, size: int = 224) -> torch.Tensor:
    """(reference preprocess.jl:45-49)"""
    c, h, w = img.shape
    top = (h - size) // 2
    left = (w - size) // 2
    return img[:, top : top + size, left : left + size]


def preprocess(img: torch.Tensor, crop: int = 224, resize: int = 256,
               normalize: bool = True) -> torch.Tensor:
    """Full pipeline (reference preprocess.jl:51-70). Input CHW float [0,1];
    output CHW float32, ImageNet-normalized."""
    x = resize_smallest_dimension(img, resize)
    x = center_crop(x, crop)
    if normalize:
        x = (x - IMAGENET_MEAN.to(x.dtype)) / IMAGENET_STD.to(x.dtype)
    return x.float()


# ---- batched preprocessing of raw uint8 images (device path) ---------------
# One row per image, the layout csrc/fda_kernels.h documents: int64 arena
# offset, int32 h, w, nh, nw, top, left, r, float32 sigma (40 bytes, seen by
# the kernel as 10 int32 words).
_META = np.dtype([("off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("nh", "<i4"),
                  ("nw", "<i4"), ("top", "<i4"), ("left", "<i4"),
                  ("r", "<i4"), ("sigma", "<f4")])
META_INTS = _META.itemsize // 4


@dataclass
class RawBatch:
    """Decoded but unprocessed images: `arena` is one uint8 buffer holding
    every image as HWC RGB at a 16-byte-aligned offset, `meta` the int32
    [n, META_INTS] geometry table that `preprocess_batch` consumes."""
    arena: torch.Tensor
    meta: torch.Tensor
    n: int
    resize: int
    crop: int

    def pin_memory(self) -> "RawBatch":
        return RawBatch(self.arena.pin_memory(), self.meta.pin_memory(),
                        self.n, self.resize, self.crop)

    def is_pinned(self) -> bool:
        return self.arena.is_pinned() and self.meta.is_pinned()

    def to(self, device, non_blocking: bool = False) -> "RawBatch":
        return RawBatch(self.arena.to(device, non_blocking=non_blocking),
                        self.meta.to(device, non_blocking=non_blocking),
                        self.n, self.resize, self.crop)

    def image(self, i: int) -> torch.Tensor:
        """Image i as an HWC uint8 view of a host arena."""
        row = self.meta.cpu().numpy().view(_META)[i, 0]
        h, w, off = int(row["h"]), int(row["w"]), int(row["off"])
        return self.arena[off:off + h * w * 3].view(h, w, 3)


def image_geometry(h: int, w: int, resize: int, crop: int):
    """(nh, nw, top, left, r, sigma) for one h x w image: the sizes
    `resize_smallest_dimension` resizes to, the `center_crop` origin, and
    the low-pass radius / sigma (r = 0, sigma = 0 when not downscaling)."""
    scale = resize / min(h, w)
    nh, nw = max(resize, round(h * scale)), max(resize, round(w * scale))
    top, left = (nh - crop) // 2, (nw - crop) // 2
    if scale < 1.0:
        sigma = 0.75 / scale
        r = max(1, int(math.ceil(3.0 * sigma)))
    else:
        sigma, r = 0.0, 0
    return nh, nw, top, left, r, sigma


def pack_images(images: Sequence, resize: int = 256, crop: int = 224,
                pin: bool = False) -> RawBatch:
    """Pack HWC uint8 RGB images (tensors or ndarrays, any sizes) into one
    arena and compute each image's resize / crop geometry on the host."""
    if not 1 <= crop <= resize:
        raise ValueError(f"crop {crop} must be in [1, resize={resize}]")
    arrs = []
    meta = np.zeros(len(images), dtype=_META)
    total = 0
    for i, img in enumerate(images):
        a = img.numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"image {i}: expected HWC uint8 RGB, got "
                             f"{a.dtype} {a.shape}")
        h, w = int(a.shape[0]), int(a.shape[1])
        if h < 1 or w < 1:
            raise ValueError(f"image {i}: empty image {a.shape}")
        nh, nw, top, left, r, sigma = image_geometry(h, w, resize, crop)
        if r >= min(h, w):
            raise ValueError(f"image {i}: low-pass radius {r} does not fit "
                             f"a {h}x{w} image (reflect border)")
        meta[i] = (total, h, w, nh, nw, top, left, r, sigma)
        arrs.append(a)
        total += -(-(h * w * 3) // 16) * 16
    arena = torch.zeros(total, dtype=torch.uint8, pin_memory=pin)
    view = arena.numpy()
    for a, off in zip(arrs, meta["off"]):
        view[off:off + a.size] = a.reshape(-1)
    mt = torch.from_numpy(meta.view(np.int32).reshape(len(images), META_INTS))
    if pin:
        mt = mt.pin_memory()
    return RawBatch(arena, mt, len(images), resize, crop)


def preprocess_batch(raw: RawBatch, device=None, normalize: bool = True,
                     standardize: bool = False,
                     dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """`preprocess` (+ the per-image standardize of `imagenet._fproc`) over a
    whole RawBatch. Returns [n, 3, crop, crop] with channels_last strides.

    On a GPU device the arena and the meta table are uploaded on the current
    stream (not at all if they are already there) and the native resample
    kernel does the work; the extension is required there. On the CPU the
    existing per-image `preprocess` runs, so both give the same API.
    """
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"dtype must be float32 or bfloat16, got {dtype}")
    device = torch.device(device) if device is not None else raw.arena.device
    if is_real_gpu(device):
        from ..ops.native import require_native

        native = require_native("preprocess_batch")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(device):
            arena = raw.arena.to(device, non_blocking=True)
            meta = raw.meta.to(device, non_blocking=True)
            return native.preprocess_batch(arena, meta, raw.crop, normalize,
                                           standardize,
                                           dtype == torch.bfloat16)
    out = torch.empty(raw.n, 3, raw.crop, raw.crop, dtype=dtype).contiguous(
        memory_format=torch.channels_last)
    host = RawBatch(raw.arena.cpu(), raw.meta.cpu(), raw.n, raw.resize,
                    raw.crop)
    for i in range(raw.n):
        img = (host.image(i).float() / 255.0).permute(2, 0, 1)  # HWC -> CHW
        x = preprocess(img, crop=raw.crop, resize=raw.resize,
                       normalize=normalize)
        if standardize:
            x = (x - x.mean()) / (x.std() + 1e-5)
        out[i].copy_(x)
    return out


def topk_probs(logits: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(reference preprocess.jl:74-75)"""
    probs = torch.softmax(logits.float(), dim=-1)
    return torch.topk(probs, k, dim=-1)
