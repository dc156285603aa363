"""The expectation of the crop-shim tests: `rescale_and_crop` (src/dataset/shims/crop_shim.py:11-75) restated in numpy integers.  A helper
module like tests/cleanfid_ref.py: imported by tests/test_cropshim_cpu.py, tests/test_hip_cropshim.py, tests/test_hip_dataset.py and
tests/golden/make_cropshim_golden.py (which pins it -- and the device -- against PIL's own output, tests/golden/cropshim.npz).

PIL's 8-bit resample (Resample.c): `precompute_coeffs` in double, `normalize_coeffs_8bpc` to 22 fractional bits, then per pass
clip((2^21 + sum px k) >> 22, 0, 255) in int32, horizontally first with a uint8 image in between; a pass whose size stays is skipped.
`math.sin` is the C library's, the one PIL calls."""
import functools
import hashlib
import math

import numpy as np

BITS = 22

# (name, h, w, (h_out, w_out), content): the small cases of tests/golden/cropshim.npz, two images each
CASES = (
    ("col_crop", 45, 80, (32, 32), "noise"),            # scaled 32 x 57, column crop 12
    ("row_crop", 80, 45, (32, 32), "noise"),            # scaled 57 x 32, row crop 12
    ("odd", 37, 53, (16, 16), "noise"),                 # scaled 16 x 23: odd crop, ragged tap counts at both borders
    ("even", 40, 72, (32, 32), "noise"),                # scaled 32 x 58 (57.6 rounds up): an even column crop of 13
    ("wide", 23, 200, (8, 8), "noise"),                 # scaled 8 x 70: wide support, taps clipped at the edges for most outputs
    ("pure_crop", 32, 57, (32, 32), "noise"),           # scale 1: both passes skipped
    ("copy", 32, 32, (32, 32), "noise"),
    ("checker", 45, 80, (32, 32), "checker"),           # 0 / 255 noise: the negative lobes reach both clips
)
FULL = ("full", 360, 640, (256, 256), "noise")          # by digest: the input is regenerated from the seed
N_IMG = 2


def make_images(name: str, h: int, w: int, content: str, n: int = N_IMG) -> np.ndarray:
    """uint8 [n, h, w, 3], seeded by the case's name"""
    rng = np.random.default_rng(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"))
    x = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    return np.where(x < 128, 0, 255).astype(np.uint8) if content == "checker" else x


def geometry(h: int, w: int, shape):
    """(h_scaled, w_scaled, row, col) of rescale_and_crop + center_crop"""
    h_out, w_out = shape
    assert h_out <= h and w_out <= w
    scale = max(h_out / h, w_out / w)
    h_s, w_s = round(h * scale), round(w * scale)
    assert h_s == h_out or w_s == w_out
    return h_s, w_s, (h_s - h_out) // 2, (w_s - w_out) // 2


def scale_intrinsics(intrinsics: np.ndarray, h_s: int, w_s: int, shape) -> np.ndarray:
    """center_crop's fx *= w_in / w_out, fy *= h_in / h_out on a float32 array (the factor rounded to float32 first, as torch does)"""
    out = np.array(intrinsics, dtype=np.float32, copy=True)
    out[..., 0, 0] *= np.float32(w_s / shape[1])
    out[..., 1, 1] *= np.float32(h_s / shape[0])
    return out


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


@functools.lru_cache(maxsize=None)
def axis_tables(n_in: int, n_out: int, off: int = 0, count: int = None):
    """(ksize, bounds int32 [count, 2] (first tap, taps), coefs int32 [count, ksize]) of outputs [off, off + count) of an axis n_in -> n_out;
    the identity (one tap of 2^22) where the size stays"""
    count = n_out - off if count is None else count
    if n_in == n_out:
        return 1, np.stack([np.arange(off, off + count), np.ones(count, np.int64)], 1).astype(np.int32), np.full((count, 1), 1 << BITS, np.int32)
    scl = float(n_in) / n_out
    fs = max(scl, 1.0)
    support, ss = 3.0 * fs, 1.0 / fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, coefs = np.zeros((count, 2), np.int32), np.zeros((count, ksize), np.int32)
    for i in range(count):
        center = (off + i + 0.5) * scl
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5)) - xmin
        k = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        coefs[i, :xmax] = [int(-0.5 + v * (1 << BITS)) if v < 0 else int(0.5 + v * (1 << BITS)) for v in k]
        bounds[i] = xmin, xmax
    return ksize, bounds, coefs


def _pass(img: np.ndarray, axis: int, bounds, coefs) -> np.ndarray:
    """one pass along `axis` of a uint8 array: clip((2^21 + sum px k) >> 22, 0, 255), int32 as PIL's `int`"""
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((len(bounds),) + src.shape[1:], np.uint8)
    for i, (xmin, n) in enumerate(bounds):
        acc = np.full(src.shape[1:], 1 << (BITS - 1), np.int32)
        for t in range(n):
            acc += src[xmin + t] * coefs[i, t]
        out[i] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_crop_u8(images: np.ndarray, shape) -> np.ndarray:
    """uint8 [n, h, w, 3] -> uint8 [n, h_out, w_out, 3]: Image.resize((w_s, h_s), LANCZOS) and the centre crop, only the window computed"""
    n, h, w, _ = images.shape
    h_s, w_s, row, col = geometry(h, w, shape)
    _, bx, cx = axis_tables(w, w_s, col, shape[1])
    _, by, cy = axis_tables(h, h_s, row, shape[0])
    return _pass(_pass(images, 2, bx, cx), 1, by, cy)


def quantise(images: np.ndarray) -> np.ndarray:
    """float32 [..., 3, h, w] in [0, 1] -> uint8 [..., h, w, 3]: (image * 255).clip(0, 255).type(uint8), in float32, truncating"""
    q = np.clip(images.astype(np.float32) * np.float32(255), np.float32(0), np.float32(255)).astype(np.uint8)
    return np.moveaxis(q, -3, -1)


def to_float(pixels: np.ndarray) -> np.ndarray:
    """uint8 [n, h, w, 3] -> float32 [n, 3, h, w]: np.array(image) / 255 (double), then the cast to the image's dtype"""
    return np.ascontiguousarray(np.moveaxis((pixels / 255).astype(np.float32), -1, -3))


def crop_shim(images: np.ndarray, shape) -> np.ndarray:
    """uint8 [n, h, w, 3] or float32 [n, 3, h, w] -> float32 [n, 3, h_out, w_out]"""
    if images.dtype != np.uint8:
        images = quantise(images)
    return to_float(resize_crop_u8(images, shape))


def digest(pixels: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(pixels).tobytes()).hexdigest()
