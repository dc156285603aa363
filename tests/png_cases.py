"""The frames of the PNG reader's tests (tests/test_png_cpu.py, tests/test_hip_png.py): a test-side PNG writer that takes, per row, the
filter to apply -- Pillow picks its own and cannot be told -- plus the colour type, bit depth, palette, an optional tRNS, how to split
IDAT, the zlib level and Adam7 interlace.  Seeded content; the expectation is always the pixels a case was made from AND Pillow's own
decode of the same bytes.  A helper module like tests/jpeg_cases.py."""
import hashlib
import struct
import zlib
from io import BytesIO

import numpy as np

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# (colour type, bit depth) the device path takes
SUPPORTED = [(2, 8), (6, 8), (0, 8), (4, 8), (3, 8), (3, 4), (3, 2), (3, 1)]
FILTERS = (0, 1, 2, 3, 4)


def _seed(*key) -> int:
    return int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:4], "little")


def palette(entries: int, key=0) -> np.ndarray:
    """uint8 [entries, 3], seeded, no two entries alike in the first 256"""
    rng = np.random.default_rng(_seed("palette", entries, key))
    p = rng.integers(0, 256, (entries, 3)).astype(np.uint8)
    p[:, 0] = (np.arange(entries) * 37 + 11) % 256
    return p


def samples(h: int, w: int, ctype: int, depth: int = 8, content: str = "noise", entries: int = None, key=0) -> np.ndarray:
    """the samples of a frame: [h, w, channels] (channels squeezed for grey and palette), values below 2^depth -- for a palette frame below
    `entries`.  noise: uniform; flat: one value; smooth: wrapping ramps plus +-3 of noise; photo: ramps across the frame plus +-12 of noise (what
    makes Pillow's encoder choose Sub, Up and Paeth rows in one file)"""
    rng = np.random.default_rng(_seed(h, w, ctype, depth, content, entries, key))
    c = CHANNELS[ctype]
    top = (entries if ctype == 3 and entries else 1 << depth)
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "noise":
        a = rng.integers(0, top, (h, w, c))
    elif content == "flat":
        a = np.broadcast_to(rng.integers(0, top, (1, 1, c)), (h, w, c))
    elif content == "photo":
        ramps = [yy * (top - 1) // max(h - 1, 1), xx * (top - 1) // max(w - 1, 1), (yy + xx) * (top - 1) // max(h + w - 2, 1), (top - 1) - yy * (top - 1) // max(h - 1, 1)]
        a = np.clip(np.stack(ramps[:c], axis=-1) + rng.integers(-12, 13, (h, w, c)), 0, top - 1)
    else:
        a = (np.stack([(yy * (3 + k) + xx * (5 - k)) for k in range(c)], axis=-1) + rng.integers(-3, 4, (h, w, c))) % top
    a = np.ascontiguousarray(a).astype(np.uint16 if depth == 16 else np.uint8)
    return a[..., 0] if c == 1 else a


def expected(a: np.ndarray, ctype: int, depth: int = 8, pal: np.ndarray = None) -> np.ndarray:
    """uint8 [h, w, 3]: what the samples mean as RGB -- alpha dropped, grey replicated (scaled up from below 8 bits, the high byte of 16),
    palette entries looked up"""
    if ctype == 3:
        return pal[a]
    if depth == 16:
        a = (a >> 8).astype(np.uint8)
    elif depth < 8:
        a = (a.astype(np.uint32) * 255 // ((1 << depth) - 1)).astype(np.uint8)
    if ctype in (0, 4):
        g = a if ctype == 0 else a[..., 0]
        return np.ascontiguousarray(np.stack([g, g, g], axis=-1))
    return np.ascontiguousarray(a[..., :3])


def pack_rows(a: np.ndarray, ctype: int, depth: int) -> np.ndarray:
    """samples -> uint8 [h, stride]: the unfiltered rows"""
    h, w = a.shape[:2]
    flat = a.reshape(h, w * CHANNELS[ctype])
    if depth == 8:
        return flat.astype(np.uint8)
    if depth == 16:
        return flat.astype(">u2").view(np.uint8).reshape(h, -1)
    bits = ((flat[:, :, None].astype(np.uint8) >> np.arange(depth - 1, -1, -1)) & 1).reshape(h, -1)     # leftmost pixel in the high bits
    return np.packbits(bits, axis=1)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(raw: np.ndarray, bpp: int, filters) -> bytes:
    """the forward filters of the PNG specification: row r of `raw` (uint8 [h, stride]) with filter filters[r] -> the stream IDAT deflates.
    A filter above 4 is written as its byte in front of the raw row."""
    h, stride = raw.shape
    cur = raw.astype(np.int32)
    up = np.concatenate([np.zeros((1, stride), np.int32), cur[:-1]], axis=0)
    left = np.concatenate([np.zeros((h, bpp), np.int32), cur[:, :-bpp]], axis=1)[:, :stride] if stride > bpp else np.zeros_like(cur)
    upleft = np.concatenate([np.zeros((1, stride), np.int32), left[:-1]], axis=0)
    pred = {0: np.zeros_like(cur), 1: left, 2: up, 3: (left + up) >> 1, 4: _paeth(left, up, upleft)}
    out = np.empty((h, 1 + stride), np.uint8)
    for r in range(h):
        f = int(filters[r])
        out[r, 0] = f
        out[r, 1:] = (cur[r] - pred.get(f, pred[0])[r]) & 255
    return out.tobytes()


def row_filters(h: int, spec) -> list:
    """an int: that filter on every row; "cycle": 0 1 2 3 4 0 ...; "cycle+k": the same, starting at k; a list: as given"""
    if isinstance(spec, int):
        return [spec] * h
    if isinstance(spec, str):
        k = int(spec.split("+")[1]) if "+" in spec else 0
        return [(r + k) % 5 for r in range(h)]
    assert len(spec) == h
    return list(spec)


def chunk(tag: bytes, data: bytes, flip_crc: bool = False) -> bytes:
    crc = zlib.crc32(tag + data) & 0xFFFFFFFF
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", crc ^ (1 if flip_crc else 0))


ADAM7 = ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1))       # y0, x0, dy, dx


def write_png(a: np.ndarray, ctype: int, depth: int = 8, filters=0, pal: np.ndarray = None, trns: bytes = None, idat_split: int = None,
              level: int = 6, interlace: bool = False, stream_edit=None, flip_crc: str = None, plte: bool = True) -> bytes:
    """samples (see `samples`) -> the bytes of a PNG file.  `filters`: see `row_filters` (interlaced: every pass takes filter 0).
    `idat_split`: bytes per IDAT chunk.  `stream_edit`: a function from the stream to the stream, applied before deflate (a short stream,
    trailing bytes).  `flip_crc`: the tag of the chunk whose CRC is wrong.  `plte=False`: leave the palette out."""
    h, w = a.shape[:2]
    bpp = max(1, CHANNELS[ctype] * depth // 8)
    if interlace:
        stream = b""
        for y0, x0, dy, dx in ADAM7:
            sub = a[y0::dy, x0::dx]
            if sub.size:
                stream += filter_rows(pack_rows(sub, ctype, depth), bpp, [0] * sub.shape[0])
    else:
        stream = filter_rows(pack_rows(a, ctype, depth), bpp, row_filters(h, filters))
    if stream_edit is not None:
        stream = stream_edit(stream)
    z = zlib.compress(stream, level)
    parts = [z] if not idat_split else [z[i:i + idat_split] for i in range(0, len(z), idat_split)]
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, int(interlace)), flip_crc == "IHDR")
    if ctype == 3 and plte:
        out += chunk(b"PLTE", np.ascontiguousarray(pal, dtype=np.uint8).tobytes(), flip_crc == "PLTE")
    if trns is not None:
        out += chunk(b"tRNS", trns)
    for k, part in enumerate(parts):
        out += chunk(b"IDAT", part, flip_crc == "IDAT" and k == len(parts) - 1)
    return out + chunk(b"IEND", b"", flip_crc == "IEND")


def pillow(blob: bytes) -> np.ndarray:
    """what the library has to reproduce"""
    from PIL import Image
    return np.array(Image.open(BytesIO(blob)).convert("RGB"))        # a copy: writable


def pillow_file(a: np.ndarray, mode: str, pal: np.ndarray = None) -> bytes:
    """a PNG Pillow wrote (it picks a filter per row): `a` as an image of `mode` (RGB, RGBA, L, LA or P with `pal`)"""
    from PIL import Image
    im = Image.fromarray(a, mode=mode) if mode != "P" else Image.fromarray(a, mode="P")
    if mode == "P":
        im.putpalette(np.ascontiguousarray(pal, dtype=np.uint8).tobytes())
    buf = BytesIO()
    im.save(buf, format="PNG")
    return buf.getvalue()


def filter_types(blob: bytes) -> set:
    """the filter bytes a (non-interlaced, 8-bit) PNG file uses, by reading it with the standard library only"""
    pos, idat, ihdr = 8, b"", None
    while pos < len(blob):
        n, tag = struct.unpack(">I", blob[pos:pos + 4])[0], blob[pos + 4:pos + 8]
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", blob[pos + 8:pos + 21])
        elif tag == b"IDAT":
            idat += blob[pos + 8:pos + 8 + n]
        pos += 12 + n
    w, h, depth, ctype = ihdr[:4]
    stride = (w * CHANNELS[ctype] * depth + 7) // 8
    return set(zlib.decompress(idat)[::1 + stride])


def case(h: int, w: int, ctype: int, depth: int = 8, filters=0, content: str = "noise", entries: int = None, key=0, **kw):
    """(blob, expected RGB) of one seeded frame"""
    pal = None
    if ctype == 3:
        entries = entries or (1 << depth)
        pal = palette(entries, key)
    a = samples(h, w, ctype, depth, content, entries, key)
    return write_png(a, ctype, depth, filters, pal=pal, **kw), expected(a, ctype, depth, pal)
