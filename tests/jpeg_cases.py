"""The frames of the JPEG decoder's tests (tests/test_jpeg_cpu.py, tests/test_hip_jpeg.py, tests/golden/make_jpeg_golden.py): seeded
content, encoded by Pillow where the test runs; the expectation is always Pillow's own decode of the same bytes.  A helper module like
tests/cropshim_ref.py."""
import hashlib
from io import BytesIO

import numpy as np

# (h, w): one pixel; one block; odd sizes on both sides of a block edge; more than one MCU in both directions; and 5 x 3 / 6 x 4, whose
# subsampled chroma is one or two samples wide -- the widths at which libjpeg replicates instead of filtering
SIZES = [(1, 1), (8, 8), (9, 7), (16, 16), (17, 33), (24, 40), (45, 81), (5, 3), (6, 4)]
SUBSAMPLING = [0, 1, 2]                 # Pillow's: 4:4:4, 4:2:2, 4:2:0 = sampling layout 1, 2, 3 of the library
QUALITY = [50, 90, 100]
CONTENT = ["noise", "smooth"]
BIG = (360, 640)                        # the dataset's frame size


def _seed(*key) -> int:
    return int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:4], "little")


def pixels(h: int, w: int, content: str, channels: int = 3) -> np.ndarray:
    """uint8 [h, w, 3] (or [h, w] for one channel), integer arithmetic only: uniform noise, ramps, or ramps plus +-12 of noise ("photo")"""
    rng = np.random.default_rng(_seed(h, w, content, channels))
    yy, xx = np.mgrid[0:h, 0:w]
    ramps = np.stack([(yy * 7 + xx * 3) % 256, 255 - (xx * 5) % 256, (yy * 2 + xx) % 256], axis=-1)
    if content == "noise":
        a = rng.integers(0, 256, (h, w, 3))
    elif content == "smooth":
        a = ramps
    else:
        a = np.clip(np.stack([yy * 255 // max(h - 1, 1), xx * 255 // max(w - 1, 1), (yy + xx) * 255 // max(h + w - 2, 1)], axis=-1) + rng.integers(-12, 13, (h, w, 3)), 0, 255)
    a = a.astype(np.uint8)
    return a if channels == 3 else np.ascontiguousarray(a[..., 0])


def encode(a: np.ndarray, **kw) -> bytes:
    from PIL import Image
    buf = BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def pillow(blob: bytes) -> np.ndarray:
    """what the library has to reproduce: `dataset.decode_image`'s expression"""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(BytesIO(blob)).convert("RGB")))


def small_cases(h: int, w: int):
    """(name, blob) of every subsampling x quality x content at one size"""
    for sub in SUBSAMPLING:
        for q in QUALITY:
            for content in CONTENT:
                yield f"{h}x{w}-s{sub}-q{q}-{content}", encode(pixels(h, w, content), quality=q, subsampling=sub)


def gray_case() -> bytes:
    return encode(pixels(45, 81, "noise", channels=1), quality=90)


def restart_case() -> bytes:
    return encode(pixels(45, 81, "noise"), quality=90, subsampling=2, restart_marker_rows=1)


def big_case() -> bytes:
    return encode(pixels(*BIG, "photo"), quality=90, subsampling=2)


def with_dqt(blob: bytes, value: int) -> bytes:
    """the stream with every entry of every (8-bit) quantisation table overwritten"""
    out, pos = bytearray(blob), 2
    while pos + 4 <= len(out) and out[pos] == 0xFF and out[pos + 1] != 0xDA:
        seg = int.from_bytes(out[pos + 2:pos + 4], "big")
        if out[pos + 1] == 0xDB:
            at = pos + 4
            while at < pos + 2 + seg:
                assert out[at] >> 4 == 0
                out[at + 1:at + 65] = bytes([value]) * 64
                at += 65
        pos += 2 + seg
    return bytes(out)


def scan_start(blob: bytes) -> int:
    """index of the first byte of entropy-coded data"""
    pos = 2
    while blob[pos + 1] != 0xDA:
        pos += 2 + int.from_bytes(blob[pos + 2:pos + 4], "big")
    return pos + 2 + int.from_bytes(blob[pos + 2:pos + 4], "big")


def sha256(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes() if isinstance(a, np.ndarray) else a).hexdigest()
