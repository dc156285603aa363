"""CPU: the device entropy decoder's host side -- `ops.jpeg_scan_prepare` (csrc/jpeg_host.cpp) and `ops.jpeg_entropy_emul`, the emulation
that runs the kernels' own step function (csrc/jpeg_huff_common.h) with loops for threads -- against the host's Huffman decoder
`ops.jpeg_entropy`, `np.array_equal` everywhere.  Both host buffers carry canaries.  Frames: tests/jpeg_cases.py."""
import numpy as np
import pytest

import jpeg_cases as J

CANARY16, CANARY8 = 0x5A5A, 0xA5
PAD = 64
BITS = [32, 64, 96, 128, 1024]
CHUNKS = [4, 64, 1024]
DAMAGE_SEED = 20240607              # tests/test_hip_jpeg_entropy.py draws its 16 damaged streams from the same seed


@pytest.fixture(scope="module")
def ops():
    from mv_ldm_amd import _build, _lib, ops
    _build.build()
    _lib.load()
    return ops


def host(ops, blob):
    """`jpeg_entropy`: (reason, max_s, coef, qt, info)"""
    info = ops.jpeg_probe(blob)
    count = ops.jpeg_coef_count(info.h, info.w, info.sampling) if info.supported else 64
    coef, qt = np.zeros(count, dtype=np.int16), np.zeros(192, dtype=np.uint16)
    reason, max_s = ops.jpeg_entropy(blob, coef, qt)
    return reason, max_s, coef, qt, info


def prepare(ops, blob):
    """`jpeg_scan_prepare` at a non-zero offset of a canaried buffer -> JpegScan; nothing outside the frame's ranges is written"""
    from mv_ldm_amd import _lib as L
    off = 48
    room = ops.jpeg_scan_room(len(blob))
    assert room % 16 == 0 and room >= len(blob) + 16
    scan = np.full(off + room + PAD, CANARY8, dtype=np.uint8)
    desc = np.full(4 + 2 * PAD, 0x5A5A5A5A, dtype=np.int32)
    tables = np.full(L.JPEG_TABLE_BYTES + 2 * PAD, CANARY8, dtype=np.uint8)
    got = ops.jpeg_scan_prepare(blob, scan[:off + room], off, desc[PAD:PAD + 4], tables[PAD:PAD + L.JPEG_TABLE_BYTES])
    assert (scan[:off] == CANARY8).all() and (scan[off + room:] == CANARY8).all(), "scan: a write outside the frame's room"
    assert (desc[:PAD] == 0x5A5A5A5A).all() and (desc[PAD + 4:] == 0x5A5A5A5A).all()
    assert (tables[:PAD] == CANARY8).all() and (tables[PAD + L.JPEG_TABLE_BYTES:] == CANARY8).all()
    if got.reason == 0:
        d = got.desc
        assert d[0] == off and d[1] % 8 == 0 and d[2] == ops.jpeg_scan_room(d[1] // 8) and d[2] <= room and d[3] == 0
        assert not scan[off + d[1] // 8:off + d[2]].any(), "the padding behind the scan is zero"
    return got


def emulate(ops, p, info, subseq_bits=0, chunk=0):
    """`jpeg_entropy_emul` of one prepared frame into canaried buffers -> (reason, max_s, rounds, coef, qt)"""
    count = ops.jpeg_coef_count(info.h, info.w, info.sampling)
    coef = np.full(count + 2 * PAD, CANARY16, dtype=np.int16)
    qt = np.full(192 + 2 * PAD, CANARY16, dtype=np.uint16)
    status = np.full(4 + 2 * PAD, 0x5A5A5A5A, dtype=np.int32)
    ops.jpeg_entropy_emul(p.scan, p.desc, p.tables, info.h, info.w, info.sampling, coef[PAD:PAD + count], qt[PAD:PAD + 192], status[PAD:PAD + 4],
                          subseq_bits, chunk)
    for buf, c in ((coef, CANARY16), (qt, CANARY16), (status, 0x5A5A5A5A)):
        assert (buf[:PAD] == c).all() and (buf[-PAD:] == c).all(), "a write outside the caller's buffer"
    st = status[PAD:PAD + 4]
    assert st[3] == 0
    return int(st[0]), int(st[1]), int(st[2]), coef[PAD:PAD + count].copy(), qt[PAD:PAD + 192].copy()


def check_frame(ops, blob, name, combos):
    reason, max_s, coef, qt, info = host(ops, blob)
    p = prepare(ops, blob)
    assert p.reason == 0 and p.info == info, name
    bits = int(p.desc[1])
    for sb, chunk in combos:
        got = emulate(ops, p, info, sb, chunk)
        assert (got[0], got[1]) == (reason, max_s), (name, sb, chunk, got[:3])
        assert np.array_equal(got[3], coef) and np.array_equal(got[4], qt), (name, sb, chunk)
        nsub = -(-bits // (sb or 512))                 # 0: the default, 512 bits
        assert 1 <= got[2] <= min(chunk or ops.jpeg_entropy_chunk_subseqs(), nsub), (name, sb, chunk, got[2])
        assert emulate(ops, p, info, sb, chunk)[2] == got[2], "rounds are reproducible"


ALL = [(sb, chunk) for sb in BITS for chunk in CHUNKS]


@pytest.mark.parametrize("h,w", J.SIZES, ids=lambda v: str(v))
def test_small_cases(ops, h, w):
    """every subsampling x quality x content at this size, every subsequence length and chunk size, and the default"""
    for name, blob in J.small_cases(h, w):
        check_frame(ops, blob, name, ALL + [(0, 0)])


def test_single_subsequence_end(ops):
    """the 1 x 1 frames: a scan of a few bytes is one subsequence of one chunk at 1024 bits"""
    for name, blob in J.small_cases(1, 1):
        p = prepare(ops, blob)
        assert p.reason == 0 and 0 < p.desc[1] <= 1024, (name, p.desc)
        assert emulate(ops, p, p.info, 1024, 4)[2] == 1
    assert 7 in {len(blob) - J.scan_start(blob) - 2 for _, blob in J.small_cases(1, 1)}


def test_gray_optimized_and_big(ops):
    check_frame(ops, J.gray_case(), "gray", ALL + [(0, 0)])
    check_frame(ops, J.encode(J.pixels(45, 81, "photo"), quality=90, subsampling=2, optimize=True), "optimize", ALL + [(0, 0)])
    check_frame(ops, J.big_case(), "big", [(32, 64), (128, 1024), (1024, 4), (0, 0)])


def test_multi_chunk_stuffing_heavy_end(ops):
    """45 x 81 noise at quality 100, 4:4:4: a 16,081-byte scan with 142 stuffed pairs, three chunks and more at 32 bits"""
    blob = J.encode(J.pixels(45, 81, "noise"), quality=100, subsampling=0)
    raw = blob[J.scan_start(blob):-2]
    assert len(raw) == 16081 and raw.count(b"\xff\x00") == 142
    p = prepare(ops, blob)
    assert p.reason == 0 and p.desc[1] == 8 * (16081 - 142)
    assert bytes(p.scan[48:48 + p.desc[1] // 8]) == raw.replace(b"\xff\x00", b"\xff")
    assert -(-int(p.desc[1]) // 32) >= 3 * ops.jpeg_entropy_chunk_subseqs()


def test_range_guard(ops):
    from mv_ldm_amd import _lib as L
    blob = J.with_dqt(J.encode(J.pixels(45, 81, "noise"), quality=50, subsampling=2), 255)
    reason, max_s, coef, qt, info = host(ops, blob)
    assert reason == L.JPEG_RANGE and max_s > 5905
    p = prepare(ops, blob)
    assert p.reason == 0
    for sb, chunk in [(32, 4), (128, 64), (0, 0)]:
        got = emulate(ops, p, info, sb, chunk)
        assert (got[0], got[1]) == (L.JPEG_RANGE, max_s) and np.array_equal(got[3], coef)


def test_restart_is_refused_by_prepare(ops):
    from mv_ldm_amd import _lib as L
    blob = J.restart_case()
    assert ops.jpeg_probe(blob).supported
    p = prepare(ops, blob)
    assert p.reason == L.JPEG_RESTART == 13 and L.JPEG_REASONS[13] == "restart intervals" and p.info.supported


def test_refusals_are_the_parsers(ops):
    from mv_ldm_amd.image_io import encode_png
    for blob in (J.encode(J.pixels(16, 16, "photo"), quality=90, progressive=True), encode_png(J.pixels(8, 8, "smooth")), b"", b"\xff\xd8"):
        info = ops.jpeg_probe(blob)
        p = prepare(ops, blob)
        assert not info.supported and p.reason == info.reason and p.info == info


def test_arguments(ops):
    from mv_ldm_amd import _lib as L
    blob = J.encode(J.pixels(8, 8, "noise"), quality=90)
    with pytest.raises(RuntimeError):
        ops.jpeg_scan_prepare(blob, np.zeros(ops.jpeg_scan_room(len(blob)) + 8, dtype=np.uint8), 8)         # offset not a multiple of 16
    with pytest.raises(RuntimeError):
        ops.jpeg_scan_prepare(blob, np.zeros(ops.jpeg_scan_room(len(blob)) - 16, dtype=np.uint8), 0)        # short room
    p = prepare(ops, blob)
    for bad in (16, 48, -32, 1 << 17):
        with pytest.raises(RuntimeError):
            ops.jpeg_entropy_emul(p.scan, p.desc, p.tables, 8, 8, 1, subseq_bits=bad)
    # a descriptor that does not fit the buffer is refused without a read
    for bad in ([8, 64, 0, 0], [0, 8 * p.scan.size, 0, 0], [-16, 64, 0, 0], [p.scan.size + 16, 0, 0, 0]):
        st = ops.jpeg_entropy_emul(p.scan, np.array(bad, dtype=np.int32), p.tables, 8, 8, 1)[2]
        assert st[0, 0] == 3 and st[0, 1] == 0


NOISE8 = dict(quality=100, subsampling=0)


def damaged_stream():
    blob = J.encode(J.pixels(8, 8, "noise"), **NOISE8)
    start = J.scan_start(blob)
    assert len(blob) - start - 2 == 268
    return blob, start


def parity_on_damage(ops, blob, combos=((32, 4), (0, 0))):
    """acceptance parity with the host decoder on a damaged stream; where both accept, the same coefficients -> accepted"""
    reason, max_s, coef, qt, info = host(ops, blob)
    p = prepare(ops, blob)
    if not info.supported:
        assert p.reason == info.reason
        return False
    if p.reason != 0:
        assert reason != 0, (p.reason, reason)
        return False
    for sb, chunk in combos:
        got = emulate(ops, p, info, sb, chunk)
        assert (got[0] == 0) == (reason == 0), (got[:3], reason, sb, chunk)
        if reason == 0:
            assert got[1] == max_s and np.array_equal(got[3], coef) and np.array_equal(got[4], qt)
    return reason == 0


def test_every_truncation(ops):
    blob, start = damaged_stream()
    accepted = [cut for cut in range(len(blob) + 1) if parity_on_damage(ops, blob[:cut])]
    assert accepted == [len(blob)]
    for cut in range(start):                    # in front of the scan: the parser's refusals, code for code
        assert prepare(ops, blob[:cut]).reason == ops.jpeg_probe(blob[:cut]).reason != 0


def test_tail_reasons_are_the_host_decoders(ops):
    """what follows the scan -- fill bytes, then EOI: prepare and the host decoder refuse a bad tail with the same code, TRUNCATED where
    the data runs off the end and CORRUPT where another marker stands"""
    from mv_ldm_amd import _lib as L
    truncated, corrupt = L.JPEG_REASONS.index("truncated"), L.JPEG_REASONS.index("corrupt")
    blob, _ = damaged_stream()
    body = blob[:-2]
    assert blob[-2:] == b"\xff\xd9"
    for tail, want in ((b"", truncated), (b"\xff", truncated), (b"\xff\xff", truncated), (b"\xff\xff\xff", truncated), (b"\xff\xd9", 0),
                       (b"\xff\xff\xd9", 0), (b"\xff\xff\xff\xd9\x00", 0), (b"\xff\xc4", corrupt), (b"\xff\xff\xd8", corrupt), (b"\xff\xda\xff\xd9", corrupt)):
        assert prepare(ops, body + tail).reason == host(ops, body + tail)[0] == want, tail


def test_flipped_bytes(ops):
    blob, start = damaged_stream()
    outcomes = set()
    for at in range(start, len(blob) - 2):
        for mask in (0x01, 0xFF):
            bad = bytearray(blob)
            bad[at] ^= mask
            outcomes.add(parity_on_damage(ops, bytes(bad)))
    assert outcomes == {True, False}


def damaged_sixteen():
    """the 16 flipped-byte streams the GPU test sends to the device"""
    blob, start = damaged_stream()
    rng = np.random.default_rng(DAMAGE_SEED)
    out = []
    for at, mask in zip(rng.integers(start, len(blob) - 2, 16), [0x01, 0xFF] * 8):
        bad = bytearray(blob)
        bad[int(at)] ^= mask
        out.append(bytes(bad))
    return out


def test_the_seeded_sixteen_hold_both_outcomes(ops):
    outcomes = [parity_on_damage(ops, b) for b in damaged_sixteen()]
    assert True in outcomes and False in outcomes, outcomes
