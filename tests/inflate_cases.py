"""The zlib streams of the device inflate's tests (tests/test_inflate_cpu.py, tests/test_hip_inflate.py): seeded byte strings compressed
with the standard library at the levels, strategies, window sizes and flushes that make zlib write every kind of block, a small
fixed-Huffman WRITER for the matches zlib never emits (distance 32768; distances a little below it, where the window wraps onto the
match), the corruptions of one 4 KB stream, and PNG files whose IDAT was edited with the chunk CRCs kept right.  The expectation is
always `zlib.decompress` of the same bytes.  A helper module like tests/png_cases.py.

A payload is the inflated stream of a frame, so it has a frame's shape: the library takes h, w per call and the colour type and bit
depth per frame, need = h * (1 + stride).  With h = 1 and w = 8400 the eight formats give 1051 .. 33601 bytes behind one filter byte
(`SIZES`); the 70 000 byte payload is 7 rows of RGB at w = 3333.  The filter bytes (one per row) are stamped below 5.
No frame has fewer than 2 bytes: the 1-byte and the empty payload are valid streams that no frame geometry accepts, `tiny_cases`."""
import struct
import zlib

import numpy as np

import png_cases as PC

W = 8400                                        # h = 1: need = 1 + stride
FORMATS = {1051: (3, 1), 2101: (3, 2), 4201: (3, 4), 8401: (3, 8), 16801: (4, 8), 25201: (2, 8), 33601: (6, 8)}     # need -> colour type, depth
SIZES = sorted(FORMATS)
WORDS = [b"frame", b"scene", b"color", b"target", b"context", b"view", b"pose", b"the", b"of", b"and", b"index", b"png", b"0000", b"camera", b"near", b"far"]


def _rng(*key):
    return np.random.default_rng(PC._seed("inflate", *key))


def stamp(payload: bytes, row: int) -> bytes:
    """the payload with its filter bytes (every `row`-th) taken modulo 5"""
    a = np.frombuffer(payload, dtype=np.uint8).copy()
    a[::row] %= 5
    return a.tobytes()


def text(n: int, key=0) -> bytes:
    rng = _rng("text", n, key)
    out = b" ".join(WORDS[i] for i in rng.integers(0, len(WORDS), n // 3 + 8))
    return out[:n]


def content(kind: str, n: int, key=0) -> bytes:
    if kind == "noise":
        return _rng("noise", n, key).integers(0, 256, n).astype(np.uint8).tobytes()
    if kind == "zeros":
        return bytes(n)
    if kind == "period3":
        return (b"\x01\xfe\x37" * (n // 3 + 1))[:n]
    if kind == "text":
        return text(n, key)
    if kind == "far":       # 2000 bytes, 30 000 more that match nothing, the first 2000 again 32 000 bytes later: zlib codes them as far matches
        head = content("noise", 2000, "head")
        return (head + content("noise", 30000, "far") + head + text(n, "tail"))[:n]
    raise ValueError(kind)


def deflate(payload: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush=None, mem=8) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    if flush is None:
        return c.compress(payload) + c.flush()
    half = len(payload) // 2
    return c.compress(payload[:half]) + c.flush(flush) + c.compress(payload[half:]) + c.flush()


CONFIGS = {
    "level0": dict(level=0), "level1": dict(level=1), "level6": dict(level=6), "level9": dict(level=9),
    "fixed": dict(strategy=zlib.Z_FIXED), "rle": dict(strategy=zlib.Z_RLE), "huffman": dict(strategy=zlib.Z_HUFFMAN_ONLY),
    "wbits9": dict(wbits=9), "wbits15": dict(wbits=15, level=9),
    "full_flush": dict(flush=zlib.Z_FULL_FLUSH), "sync_flush": dict(flush=zlib.Z_SYNC_FLUSH),
    "stored_flush": dict(level=0, flush=zlib.Z_FULL_FLUSH),     # a stored block, the flush's empty one, a stored block
}


def first_block_type(z: bytes) -> int:
    """BTYPE of the first block behind the 2-byte header: 0 stored, 1 fixed, 2 dynamic"""
    return (z[2] >> 1) & 3


# ---- a fixed-Huffman writer: the streams zlib does not write ----------------------------------------------------------------------------
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value: int, bits: int):       # LSB first: extra bits and headers
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, bits: int):       # a Huffman code: its first bit first
        self.put(int(format(code, f"0{bits}b")[::-1], 2), bits)

    def done(self) -> bytes:
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


def _fixed_symbol(b: _Bits, s: int):
    if s < 144:
        b.code(0x30 + s, 8)
    elif s < 256:
        b.code(0x190 + s - 144, 9)
    elif s < 280:
        b.code(s - 256, 7)
    else:
        b.code(0xC0 + s - 280, 8)


def fixed_stream(tokens) -> tuple:
    """tokens: a byte value, or (length, distance) -> (zlib stream of one fixed-Huffman block, the payload it means)"""
    b, out = _Bits(), bytearray()
    b.put(1, 1)
    b.put(1, 2)
    for t in tokens:
        if isinstance(t, tuple):
            length, dist = t
            assert 3 <= length <= 258 and 1 <= dist <= 32768 and dist <= len(out)
            ls = max(i for i in range(29) if LBASE[i] <= length)
            ls = 28 if length == 258 else ls
            _fixed_symbol(b, 257 + ls)
            b.put(length - LBASE[ls], LEXT[ls])
            ds = max(i for i in range(30) if DBASE[i] <= dist)
            b.code(ds, 5)
            b.put(dist - DBASE[ds], DEXT[ds])
            for _ in range(length):
                out.append(out[-dist])
        else:
            _fixed_symbol(b, t)
            out.append(t)
    _fixed_symbol(b, 256)
    payload = bytes(out)
    return b"\x78\x01" + b.done() + struct.pack(">I", zlib.adler32(payload)), payload


def handmade(need: int, matches, key=0) -> tuple:
    """`need` bytes: a filter byte, noise literals, then the (length, distance) matches with a literal between them, noise to the end"""
    rng = _rng("handmade", need, key)
    first = max(d for _, d in matches)
    tokens = [0] + [int(v) for v in rng.integers(0, 256, first - 1)]
    count = first
    for length, dist in matches:
        tokens += [(length, dist), int(rng.integers(0, 256))]
        count += length + 1
    assert count <= need
    tokens += [int(v) for v in rng.integers(0, 256, need - count)]
    z, payload = fixed_stream(tokens)
    assert len(payload) == need
    return z, payload


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, z, payload, h, w, ctype, depth):
        self.name, self.z, self.payload, self.h, self.w, self.ctype, self.depth = name, z, payload, h, w, ctype, depth
        self.need = len(payload)
        assert self.need == h * (1 + (w * PC.CHANNELS[ctype] * depth + 7) // 8), name


_CASES = None


def cases() -> list:
    """every stream the decoder has to accept, made once"""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    k = 0
    for kind in ("noise", "zeros", "period3", "text"):
        for name, cfg in CONFIGS.items():
            need = SIZES[k % 4]                 # 1051 .. 8401: only the far matches below need 33 KB
            k += 1
            payload = stamp(content(kind, need, name), need)
            out.append(Case(f"{kind}/{name}", deflate(payload, **cfg), payload, 1, W, *FORMATS[need]))
    far = stamp(content("far", 33601), 33601)
    out.append(Case("far/level9", deflate(far, level=9), far, 1, W, 6, 8))
    for name, need, matches in (("dist32768", 33601, [(258, 32768), (3, 32768), (258, 1)]), ("window_wrap", 33601, [(258, 32758), (258, 32700), (200, 32767)]),
                                ("overlap", 2101, [(258, 1), (258, 2), (258, 3), (7, 5), (3, 1), (258, 257), (100, 64), (130, 63), (129, 65)])):
        z, payload = handmade(need, matches, name)
        out.append(Case(f"handmade/{name}", z, payload, 1, W, *FORMATS[need]))
    z, payload = fixed_stream([0, 7])           # two literals in a fixed block: a distance code that is never used
    out.append(Case("handmade/two_bytes", z, payload, 1, 1, 0, 8))
    rows = stamp(content("text", 70000, "rows"), 10000)
    out.append(Case("stored/70000", deflate(rows, level=0), rows, 7, 3333, 2, 8))
    _CASES = out
    return out


def tiny_cases() -> list:
    """(name, zlib stream): valid streams of 1 and 0 bytes.  No frame is that short (need >= 2), so the library has to report the length."""
    return [("one_byte", zlib.compress(b"\x00", 6)), ("empty", zlib.compress(b"", 6)), ("empty_stored", zlib.compress(b"", 0))]


def self_check():
    """what the cases are meant to contain, checked with the standard library alone"""
    by = {c.name: c for c in cases()}
    for c in cases():
        assert zlib.decompress(c.z) == c.payload, c.name
    assert first_block_type(by["text/level0"].z) == 0 and first_block_type(by["noise/level0"].z) == 0
    assert first_block_type(by["text/level6"].z) == 2 and first_block_type(by["text/level9"].z) == 2 and first_block_type(by["text/huffman"].z) == 2
    assert first_block_type(by["text/fixed"].z) == 1 and first_block_type(by["zeros/fixed"].z) == 1
    assert by["text/wbits9"].z[0] >> 4 == 1 and by["text/wbits15"].z[0] >> 4 == 7
    # zeros under Z_FIXED: two literals (zlib's lazy matcher), then distance-1 matches of 258 -- the very tokens, rebuilt with the writer above
    n = by["zeros/fixed"].need - 2
    z, _ = fixed_stream([0, 0] + [(258, 1)] * (n // 258) + ([(n % 258, 1)] if n % 258 >= 3 else [0] * (n % 258)))
    assert z[2:-4] == by["zeros/fixed"].z[2:-4], "zlib wrote the zeros some other way"
    # 70 000 bytes at level 0: more than one stored block (a block holds at most 65535)
    s = by["stored/70000"].z
    length = struct.unpack("<H", s[3:5])[0]
    assert s[2] == 0 and length < 70000 and s[2 + 5 + length] in (0, 1)
    assert len(by["text/stored_flush"].z) >= by["text/stored_flush"].need + 2 + 3 * 5 + 4, "three stored blocks, one of them empty"
    # the far case: the second copy of the 2000 (here 1601) noise bytes costs a fraction of them, so it went out as matches 32 000 bytes back
    far = by["far/level9"].payload
    assert len(far) == 33601 and len(deflate(far, level=9)) - len(deflate(far[:32000], level=9)) < 400
    for f in (zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH):
        assert b"\x00\x00\xff\xff" in deflate(by["text/level6"].payload, flush=f)       # the empty stored block of a flush


# ---- corruptions of one 4 KB stream --------------------------------------------------------------------------------------------------------
def corruptions() -> list:
    """(name, zlib stream, payload or None, reasons allowed) at need 4201: `None` where the stream must be refused"""
    from mv_ldm_amd import _lib as L
    need = 4201
    payload = stamp(content("text", need, "corrupt"), need)
    z = deflate(payload, level=6)
    assert first_block_type(z) == 2 and zlib.decompress(z) == payload
    flip = lambda at, bit: z[:at] + bytes([z[at] ^ (1 << bit)]) + z[at + 1:]
    inflate, length = (L.PNG_INFLATE,), (L.PNG_LENGTH,)
    longer, shorter = stamp(content("text", need + 1, "corrupt"), need), stamp(content("text", need - 1, "corrupt"), need)
    return [
        ("clean", z, payload, (0,)),
        ("header bit", flip(0, 0), None, inflate),                  # CM = 9
        ("block header bit", flip(2, 1), None, inflate),            # BTYPE 2 -> 3, the reserved type
        ("mid-stream bit", flip(len(z) // 2, 3), None, (L.PNG_INFLATE, L.PNG_LENGTH)),   # a wrong symbol: the check sum, or the length if the end moved
        ("trailer bit", flip(len(z) - 1, 0), None, inflate),
        ("truncated by 1", z[:-1], None, inflate),
        ("truncated by 5", z[:-5], None, inflate),
        ("one byte appended", z + b"\x00", None, inflate),
        ("need one short", deflate(longer, level=6), None, length),  # a valid stream of need + 1 bytes
        ("need one long", deflate(shorter, level=6), None, length),  # a valid stream of need - 1 bytes
        ("filter byte 5", deflate(b"\x05" + payload[1:], level=6), None, (L.PNG_FILTER,)),
        ("clean again", z, payload, (0,)),
    ]


def pack(streams, infos, guard: int = 64):
    """z buffer, zdesc, desc, slot offsets for streams [(z, colour type, depth, need)]: each zlib stream at a multiple of 16 with zeros up
    to its room, each output slot with `guard` bytes on either side"""
    zoffs, soffs, zend, send = [], [], 0, guard
    for z, (ctype, depth, need) in zip(streams, infos):
        zoffs.append(zend)
        zend += ((len(z) + 15) & ~15) + 16
        soffs.append(send)
        send += need + guard
    zbuf = np.zeros(zend, dtype=np.uint8)
    zdesc = np.zeros((len(streams), 4), dtype=np.int32)
    desc = np.zeros((len(streams), 8), dtype=np.int32)
    for i, (z, (ctype, depth, need)) in enumerate(zip(streams, infos)):
        zbuf[zoffs[i]:zoffs[i] + len(z)] = np.frombuffer(z, dtype=np.uint8)
        zdesc[i] = (zoffs[i], len(z), 0, 0)
        desc[i] = (soffs[i], ctype, depth, 0, 1 if ctype == 3 else 0, 0, 0, 0)
    return zbuf, zdesc, desc, soffs, send


def guards_intact(streams_out: np.ndarray, soffs, needs, guard: int = 64, fill: int = 0xA5) -> bool:
    """every byte outside the slots still holds the fill"""
    mask = np.ones(streams_out.size, dtype=bool)
    for off, need in zip(soffs, needs):
        mask[off:off + need] = False
    return bool((streams_out[mask] == fill).all())


def edit_idat(blob: bytes, edit) -> bytes:
    """a PNG file with its IDAT bodies joined, passed through `edit` and written back as one chunk with a right CRC"""
    pos, idat, pre, post = 8, b"", [], []
    while pos < len(blob):
        n, tag = struct.unpack(">I", blob[pos:pos + 4])[0], blob[pos + 4:pos + 8]
        body = blob[pos + 8:pos + 8 + n]
        if tag == b"IDAT":
            idat += body
        else:
            (post if idat else pre).append(PC.chunk(tag, body))
        pos += 12 + n
    return blob[:8] + b"".join(pre) + PC.chunk(b"IDAT", edit(idat)) + b"".join(post)


def refusal_frames(h, w, palette_index=True):
    """one frame per refusal reason that Pillow still reads (the fallback has to give pixels): (blobs, reason names)"""
    rgb = PC.samples(h, w, 2, 8, "photo")
    base = PC.write_png(rgb, 2, 8, "cycle")
    beyond = PC.samples(h, w, 3, 8, "noise", entries=256)
    beyond[0, 0] = 200
    blobs = [PC.write_png(rgb, 2, 8, interlace=True), PC.write_png(PC.samples(h, w, 2, 16), 2, 16), PC.write_png(PC.samples(h, w, 0, 2), 0, 2),
             PC.write_png(rgb, 2, 8, "cycle", stream_edit=lambda s: s + b"\0"), edit_idat(base, lambda z: z + b"\0"), edit_idat(base, lambda z: z[:-4]),
             PC.write_png(beyond, 3, 8, "cycle", pal=PC.palette(12))]
    names = ["interlaced", "16-bit samples", "grey below 8 bits", "inflated length", "inflate", "inflate", "palette index"]
    return (blobs, names) if palette_index else (blobs[:-1], names[:-1])
