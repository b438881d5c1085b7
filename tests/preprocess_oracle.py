"""Dense float64 oracle of the batched-preprocessing math contract, shared by
test_preprocess_batch.py (CPU) and test_preprocess_gpu.py.

Written from the contract, not from the kernel: per axis a dense weight
matrix W[out, src] built tap by tap (Gaussian taps k[i] around both bilinear
taps, reflect indexing), then einsum('oy,cyx,px').
"""

import math

import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32).astype(np.float64)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32).astype(np.float64)

# (h, w, crop, resize) and what each case exercises
CASES = [
    (300, 401, 24, 32),    # r=22, odd nw-crop
    (300, 401, 32, 32),    # reflect border
    (700, 500, 40, 40),    # r=29
    (97, 61, 24, 32),      # portrait
    (33, 47, 32, 32),      # r=3, scale just under 1
    (20, 31, 24, 32),      # upscale, no blur
    (32, 32, 24, 32),      # identity scale
    (64, 80, 224, 256),    # full-size crop with upscale
    (300, 400, 224, 256),  # standard
]


def case_id(case):
    return "{}x{}_c{}_r{}".format(*case)


def make_image(h, w, seed):
    """Seeded uint8 HWC image: smooth gradients plus noise (the gradients
    keep the post-normalize std well above 0.1 even under a wide blur)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([yy / max(h - 1, 1), xx / max(w - 1, 1),
                     1.0 - (yy + xx) / max(h + w - 2, 1)], axis=-1) * 255.0
    noise = rng.integers(0, 256, size=(h, w, 3)).astype(np.float64)
    return (0.6 * base + 0.4 * noise).astype(np.uint8)


def case_image(case):
    h, w, crop, resize = case
    return make_image(h, w, seed=1000 * h + w + crop)


def _reflect(i, n):
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    return i


def _gauss(scale):
    if scale < 1.0:
        sigma = 0.75 / scale
        r = max(1, int(math.ceil(3.0 * sigma)))
        i = np.arange(-r, r + 1, dtype=np.float64)
        k = np.exp(-(i * i) / (2.0 * sigma * sigma))
        return r, k / k.sum()
    return 0, np.ones(1, dtype=np.float64)


def _axis_matrix(n, nn, origin, crop, r, k):
    W = np.zeros((crop, n), dtype=np.float64)
    den = 2 * nn
    for o in range(crop):
        num = max(0, (2 * (o + origin) + 1) * n - nn)
        t0, lam = num // den, (num % den) / den
        t1 = min(t0 + 1, n - 1)
        for t, wt in ((t0, 1.0 - lam), (t1, lam)):
            for i in range(-r, r + 1):
                W[o, _reflect(t + i, n)] += wt * k[i + r]
    return W


def oracle(img, resize, crop, normalize=True, standardize=False):
    """img: HWC uint8 ndarray -> float64 [3, crop, crop]."""
    h, w = img.shape[:2]
    scale = resize / min(h, w)
    nh, nw = max(resize, round(h * scale)), max(resize, round(w * scale))
    top, left = (nh - crop) // 2, (nw - crop) // 2
    r, k = _gauss(scale)
    assert r < min(h, w)
    Wy = _axis_matrix(h, nh, top, crop, r, k)
    Wx = _axis_matrix(w, nw, left, crop, r, k)
    src = img.astype(np.float64).transpose(2, 0, 1) / 255.0
    v = np.einsum("oy,cyx,px->cop", Wy, src, Wx, optimize=True)
    if normalize:
        v = (v - MEAN[:, None, None]) / STD[:, None, None]
    if standardize:
        v = (v - v.mean()) / (v.std(ddof=1) + 1e-5)
    return v
