"""Image output for the generation harness: the counterpart of `src/misc/image_io.py:42-73`
(`prep_image`: clip to [0,1], x255, truncate to uint8, HWC; `save_image`: create the parent directory, write).
The reference writes through PIL; here the PNG container is produced directly (zlib + CRC from the standard
library: an 8-bit RGB / RGBA / grey image is a filter byte + raw row per scanline, deflated).
Reading: `load_image` / `decode_png` read this writer's own files (filter 0 on every row); `load_images` reads a batch of ANY PNG files --
what Pillow writes, filtered rows, grey, palette -- through `ops.png_decode`: inflate on the host, unfiltering and expansion on the device."""
from __future__ import annotations

import struct
import zlib
from pathlib import Path
from typing import Union

import numpy as np
import torch


def prep_image(image: torch.Tensor) -> np.ndarray:
    """[3|4, H, W] / [1, H, W] / [H, W] float in [0, 1] -> uint8 [H, W, C] (image_io.py:42-58: truncation, not rounding)"""
    if image.dim() == 2:
        image = image[None]
    if image.shape[0] == 1:
        image = image.expand(3, -1, -1)
    assert image.dim() == 3 and image.shape[0] in (3, 4), tuple(image.shape)
    image = (image.detach().float().clip(min=0, max=1) * 255).to(torch.uint8)
    return image.permute(1, 2, 0).contiguous().cpu().numpy()


def encode_png(pixels: np.ndarray) -> bytes:
    h, w, c = pixels.shape
    assert pixels.dtype == np.uint8 and c in (3, 4)
    color_type = 2 if c == 3 else 6

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    raw = np.concatenate([np.zeros((h, 1), np.uint8), pixels.reshape(h, w * c)], axis=1).tobytes()   # filter 0 per row
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color_type, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def save_image(image: torch.Tensor, path: Union[Path, str]) -> None:
    """Save an image assumed to be in range 0-1 (image_io.py:61-73)."""
    path = Path(path)
    path.parent.mkdir(exist_ok=True, parents=True)
    path.write_bytes(encode_png(prep_image(image)))


def decode_png(data: bytes) -> np.ndarray:
    """inverse of `encode_png` for its own output (filter-0 rows only); used by the tests and for round trips"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == (zlib.crc32(tag + body) & 0xFFFFFFFF), "bad CRC"
        if tag == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            assert depth == 8 and ctype in (2, 6)
            c = 3 if ctype == 2 else 4
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * c)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, c).copy()


def load_image(path: Union[Path, str]) -> torch.Tensor:
    """a PNG written by `save_image` -> float32 [3, H, W] in [0, 1] (k / 255; an alpha channel is dropped): the inverse the metric
    tool scores PNG trees with (src/evaluation/metric_computer.py reads the same files through torchvision)"""
    pixels = decode_png(Path(path).read_bytes())
    return torch.from_numpy(pixels[..., :3]).permute(2, 0, 1).float() / 255


def image_size(path: Union[Path, str]) -> tuple:
    """(h, w) of an image file without decoding it: a PNG's IHDR, anything else through Pillow's lazy open"""
    from .ops import png_probe
    with open(path, "rb") as f:
        info = png_probe(f.read(33))
    if info.h and info.w:
        return info.h, info.w
    from PIL import Image
    with Image.open(path) as im:
        return im.height, im.width


def group_by_size(paths) -> dict:
    """{(h, w): [positions in `paths`]}, sizes in order of first appearance, positions ascending"""
    groups: dict = {}
    for i, p in enumerate(paths):
        groups.setdefault(image_size(p), []).append(i)
    return groups


def load_images(paths, device="cuda", pool=None, out: str = "float", info=None, inflate: str = "host") -> torch.Tensor:
    """any PNG files of ONE size -> float32 `[n, 3, h, w]` in [0, 1] on `device`, in the order of `paths`: `Image.open(p).convert("RGB")`
    as k / 255 (for RGB and RGBA files the reference's `ToTensor()(Image.open(p))[:3]`), whichever filter the writer chose per row and
    whether the file is RGB, RGBA, grey, grey + alpha or palette.  The host inflates (on `pool`, a `concurrent.futures` executor, when
    one is given), one upload, and the device unfilters, expands and writes the layout (`ops.png_decode`); what that refuses goes through
    Pillow into the same slot.  `out="uint8"`: the decoded bytes, uint8 `[n, h, w, 3]`.  Files of several sizes: `group_by_size` first.
    `info`: see `ops.png_decode`.  `inflate="device"`: IDAT is inflated on the device too (`ops.png_decode`; opt-in, the same pixels)."""
    from .ops import _map, png_decode
    paths = list(paths)
    if not paths:
        raise ValueError("load_images: no files")
    sizes = group_by_size(paths)
    if len(sizes) > 1:
        raise ValueError(f"load_images: files of one size, got {sorted(sizes)} (group_by_size splits a list)")
    return png_decode(_map(pool, lambda p: Path(p).read_bytes(), paths), pool=pool, device=device, out=out, info=info, inflate=inflate)
