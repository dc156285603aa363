"""CPU: the restart-interval path of the device entropy decoder on the host -- `ops.jpeg_rst_prepare` (csrc/jpeg_host.cpp) and
`ops.jpeg_rst_entropy_emul`, the emulation that runs jpeg_huff.hip's own inline functions (csrc/jpeg_huff_common.h) with loops for
threads -- against the host's Huffman decoder `ops.jpeg_entropy`, `np.array_equal` everywhere, canaries around every buffer.
Frames: tests/jpeg_restart_cases.py."""
import numpy as np
import pytest

import jpeg_cases as J
import jpeg_restart_cases as R

CANARY16, CANARY8, CANARY32 = 0x5A5A, 0xA5, 0x5A5A5A5A
PAD = 64
BITS = [32, 96, 1024, 0]
CHUNKS = [4, 64, 1024]
ALL = [(sb, chunk) for sb in BITS for chunk in CHUNKS]


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
    """`jpeg_rst_prepare` at a non-zero offset of a canaried buffer of exactly the frame's need -> JpegScan"""
    from mv_ldm_amd import _lib as L
    off = 48
    need, room = ops.jpeg_rst_need(blob), ops.jpeg_rst_room(len(blob))
    assert room % 16 == 0 and need % 16 == 0 and need <= room
    scan = np.full(off + need + PAD, CANARY8, dtype=np.uint8)
    desc = np.full(4 + 2 * PAD, CANARY32, dtype=np.int32)
    tables = np.full(L.JPEG_TABLE_BYTES + 2 * PAD, CANARY8, dtype=np.uint8)
    got = ops.jpeg_rst_prepare(blob, scan[:off + need], off, desc[PAD:PAD + 4], tables[PAD:PAD + L.JPEG_TABLE_BYTES])
    assert (scan[:off] == CANARY8).all() and (scan[off + need:] == CANARY8).all(), "scan: a write outside the frame's room"
    assert (desc[:PAD] == CANARY32).all() and (desc[PAD + 4:] == CANARY32).all()
    assert (tables[:PAD] == CANARY8).all() and (tables[PAD + L.JPEG_TABLE_BYTES:] == CANARY8).all()
    assert got.reason != L.JPEG_RESTART
    if got.reason == 0:
        assert need > 0
        d = got.desc
        n = int(d[1])
        assert d[0] == off and n >= 1 and d[2] % 16 == 0 and d[2] <= need and d[3] >= 1
        table = scan[off:off + 8 * n].view(np.int32).reshape(n, 2)
        tb = (8 * n + 15) // 16 * 16
        assert not scan[off + 8 * n:off + tb].any()
        at = tb
        for o, bits in table:                           # 4-byte aligned, in order, zeros in the gaps, 16 bytes and more of zeros behind the last
            assert o % 4 == 0 and bits % 8 == 0 and at <= o < at + 4 and not scan[off + at:off + o].any(), (o, bits, at)
            at = o + bits // 8
        assert d[2] - at >= 16 and not scan[off + at:off + d[2]].any(), "the padding behind the last interval is zero"
    else:
        assert (got.desc[1:] == 0).all()
    return got


def emulate(ops, p, info, subseq_bits=0, chunk=0):
    """`jpeg_rst_entropy_emul` of one prepared frame into canaried buffers -> (reason, max_s, rounds, intervals, coef, qt)"""
    count = ops.jpeg_coef_count(info.h, info.w, info.sampling)
    coef = np.full(count + 2 * PAD, CANARY16, dtype=np.int16)
    qt = np.full(192 + 2 * PAD, CANARY16, dtype=np.uint16)
    status = np.full(4 + 2 * PAD, CANARY32, dtype=np.int32)
    ops.jpeg_rst_entropy_emul(p.scan, p.desc, p.tables, info.h, info.w, info.sampling, coef[PAD:PAD + count], qt[PAD:PAD + 192], status[PAD:PAD + 4],
                              subseq_bits, chunk)
    for buf, c in ((coef, CANARY16), (qt, CANARY16), (status, CANARY32)):
        assert (buf[:PAD] == c).all() and (buf[-PAD:] == c).all(), "a write outside the caller's buffer"
    st = status[PAD:PAD + 4]
    return int(st[0]), int(st[1]), int(st[2]), int(st[3]), coef[PAD:PAD + count].copy(), qt[PAD:PAD + 192].copy()


def check_frame(ops, blob, name, intervals, combos=ALL):
    reason, max_s, coef, qt, info = host(ops, blob)
    assert reason == 0, name
    p = prepare(ops, blob)
    assert p.reason == 0 and p.info == info and p.desc[1] == intervals, (name, p.reason, p.desc)
    n = intervals
    table = p.scan[48:48 + 8 * n].view(np.int32).reshape(n, 2)
    for sb, chunk in combos:
        got = emulate(ops, p, info, sb, chunk)
        assert got[:2] == (reason, max_s) and got[3] == intervals, (name, sb, chunk, got[:4])
        assert np.array_equal(got[4], coef) and np.array_equal(got[5], qt), (name, sb, chunk)
        # subsequence s of an interval is right after s rounds and the round after the last change sees none: the rounds of a chunk are
        # bounded by the subsequences of ONE interval (and by the chunk, where an interval is longer than one)
        longest = max(-(-int(bits) // (sb or 512)) for _, bits in table)
        assert 1 <= got[2] <= min(chunk or ops.jpeg_entropy_chunk_subseqs(), longest), (name, sb, chunk, got[2], longest)
    return p, table


FRAMES = {name: (blob, n) for name, blob, n in R.frames()}


@pytest.mark.parametrize("name", list(FRAMES))
def test_frames(ops, name):
    blob, n = FRAMES[name]
    assert len([m for m in R.markers(blob) if 0xD0 <= m[1] <= 0xD7]) == n - 1
    check_frame(ops, blob, name, n)


def test_markers_wrap_and_a_batch_boundary_falls_between_intervals(ops):
    """45 x 81 noise, quality 100, 4:2:0, Ri = 1: 17 markers (RSTn wraps twice), 7,854 scan bytes with 82 stuffed pairs; at 32 bits about
    2,000 subsequences, so a batch of 1024 ends between two intervals"""
    blob, n = FRAMES["noise-q100-420-ri1"]
    raw = blob[J.scan_start(blob):-2]
    assert R.dri(blob) == 1 and [c for _, c in R.markers(blob)] == [0xD0 + k % 8 for k in range(17)] + [0xD9]
    assert len(raw) == 7854 and raw.count(b"\xff\x00") == 82
    p = prepare(ops, blob)
    table = p.scan[48:48 + 8 * n].view(np.int32).reshape(n, 2)
    assert int(table[:, 1].sum()) == 8 * (7854 - 82 - 2 * 17)
    counts = [-(-int(bits) // 32) for bits in table[:, 1]]
    assert sum(counts) > 1024 and max(counts) < 1024
    # at 1024 bits an interval is four subsequences: four rounds at the most, where a cold decoder needs about nine
    assert max(-(-int(bits) // 1024) for bits in table[:, 1]) == 4 and emulate(ops, p, p.info, 1024, 1024)[2] <= 4


def test_long_intervals_take_chunks_with_a_carry(ops):
    """48 x 640 noise, quality 100, 4:4:4, one interval per MCU row: Ri = 80, six intervals of about 21 KB -- more than five chunks of 1024
    per interval at 32 bits, three intervals per batch at 512"""
    blob, n = FRAMES["noise-48x640-q100-444-rows1"]
    assert R.dri(blob) == 80
    p = prepare(ops, blob)
    bits = p.scan[48:48 + 8 * n].view(np.int32).reshape(n, 2)[:, 1]
    assert all(int(b) // 32 > 5 * 1024 for b in bits)
    per = [-(-int(b) // 512) for b in bits]
    assert sum(per[:3]) <= 1024 < sum(per[:4])


def test_a_frame_without_dri_equals_the_existing_emulation(ops):
    blob, _ = FRAMES["noise-q90-420-plain"]
    assert R.dri(blob) == 0
    old = ops.jpeg_scan_prepare(blob)
    info = old.info
    p = prepare(ops, blob)
    assert p.reason == old.reason == 0 and p.desc[1] == 1 and p.desc[3] == info.mcu_cols * info.mcu_rows
    for sb, chunk in [(32, 4), (96, 64), (0, 0)]:
        want = ops.jpeg_entropy_emul(old.scan, old.desc, old.tables, info.h, info.w, info.sampling, subseq_bits=sb, chunk_subseqs=chunk)
        got = emulate(ops, p, info, sb, chunk)
        assert got[:3] == tuple(int(v) for v in want[2][0, :3])              # reason, S and rounds: one interval is the frame's walk
        assert np.array_equal(got[4], want[0][0]) and np.array_equal(got[5], want[1][0])


def test_the_two_emulations_agree_on_a_frame_of_several_chunks(ops):
    """`R.seam_case()`: the host decoder accepts it under the guard, and both emulations give its values at chunks of 4 and of 1024 --
    more than one chunk of the scan and a carry in the DC pass"""
    blob = R.seam_case()
    reason, max_s, coef, qt, info = host(ops, blob)
    assert R.dri(blob) == 0 and reason == 0 and 0 < max_s <= 5905 and (info.h, info.w, info.sampling) == (264, 264, 1)
    assert info.mcu_cols * info.mcu_rows == 1089 > 1024
    old, p = ops.jpeg_scan_prepare(blob), prepare(ops, blob)
    assert old.reason == p.reason == 0 and p.desc[1] == 1 and p.desc[3] == 1089
    assert old.desc[1] > 4 * 1024 * 32                                          # bits: more than four chunks of 1024 at 32 bits
    for sb, chunk in [(32, 4), (32, 1024), (0, 4), (0, 1024)]:
        want = ops.jpeg_entropy_emul(old.scan, old.desc, old.tables, info.h, info.w, info.sampling, subseq_bits=sb, chunk_subseqs=chunk)
        got = emulate(ops, p, info, sb, chunk)
        assert tuple(int(v) for v in want[2][0]) == (0, max_s, got[2], 0) and got[:2] == (0, max_s) and got[3] == 1, (sb, chunk, want[2], got[:4])
        for c, q in ((want[0][0], want[1][0]), (got[4], got[5])):
            assert np.array_equal(c, coef) and np.array_equal(q, qt), (sb, chunk)


def test_fill_byte_in_front_of_a_marker(ops):
    blob = J.restart_case()
    at = [a for a, c in R.markers(blob) if 0xD0 <= c <= 0xD7][1]
    filled = blob[:at] + b"\xff" + blob[at:]
    want, got = host(ops, blob), host(ops, filled)
    assert got[0] == 0 and np.array_equal(got[2], want[2])
    p = prepare(ops, filled)
    assert p.reason == 0
    for sb, chunk in [(32, 4), (0, 0)]:
        e = emulate(ops, p, p.info, sb, chunk)
        assert e[:2] == (0, want[1]) and np.array_equal(e[4], want[2]) and np.array_equal(e[5], want[3])


def parity_on_damage(ops, blob, combos=((32, 4), (0, 0)), prepare_refuses=None):
    """acceptance parity with the host decoder; prepare's reason is the host's wherever prepare itself refuses; where both accept, the
    same values -> (accepted, prepare passed)"""
    reason, max_s, coef, qt, info = host(ops, blob)
    p = prepare(ops, blob)
    if prepare_refuses is not None:
        assert (p.reason != 0) == prepare_refuses
    if p.reason != 0:
        assert p.reason == reason, (p.reason, reason)
        return False, False
    for sb, chunk in combos:
        got = emulate(ops, p, info, sb, chunk)
        assert (got[0] == 0) == (reason == 0), (got[:4], reason, sb, chunk)
        if reason == 0:
            assert got[1] == max_s and np.array_equal(got[4], coef) and np.array_equal(got[5], qt)
    return reason == 0, True


def test_damaged_marker_structure(ops):
    blob = J.restart_case()
    assert R.dri(blob) == 6 and parity_on_damage(ops, blob) == (True, True)
    damage = R.marker_damage(blob)
    assert len(damage) == 5
    for name, bad in damage:
        assert parity_on_damage(ops, bad, prepare_refuses=True) == (False, False), name
    # one too many and one too few at the END of the stream
    rst = [a for a, c in R.markers(blob) if 0xD0 <= c <= 0xD7]
    assert parity_on_damage(ops, blob[:-2] + b"\xff\xd2\xff\xd9", prepare_refuses=True)[0] is False
    assert parity_on_damage(ops, blob[:rst[-1]] + b"\xff\xd9", prepare_refuses=True)[0] is False


def test_every_truncation(ops):
    blob = J.restart_case()
    start = J.scan_start(blob)
    accepted = [cut for cut in range(start, len(blob) + 1) if parity_on_damage(ops, blob[:cut], combos=((0, 0),), prepare_refuses=cut < len(blob))[0]]
    assert accepted == [len(blob)]
    for cut in range(0, start, 7):                      # in front of the scan: the parser's refusals, code for code
        assert prepare(ops, blob[:cut]).reason == ops.jpeg_probe(blob[:cut]).reason != 0


def test_sixteen_flips_inside_interval_data(ops):
    flips = R.flipped_sixteen()
    accepted = [host(ops, b)[0] == 0 for b in flips]
    assert True in accepted and False in accepted, accepted
    assert sum(prepare(ops, b).reason == 0 for b in flips) >= 8
    assert [parity_on_damage(ops, b)[0] for b in flips] == accepted


def test_range_guard_and_refusals(ops):
    from mv_ldm_amd import _lib as L
    from mv_ldm_amd.image_io import encode_png
    blob = J.with_dqt(J.encode(J.pixels(45, 81, "noise"), quality=50, subsampling=2, restart_marker_blocks=2), 255)
    reason, max_s, coef, qt, info = host(ops, blob)
    assert reason == L.JPEG_RANGE and max_s > 5905
    p = prepare(ops, blob)
    assert p.reason == 0
    for sb, chunk in [(32, 4), (0, 0)]:
        got = emulate(ops, p, info, sb, chunk)
        assert got[:2] == (L.JPEG_RANGE, max_s) and np.array_equal(got[4], coef)
    for bad in (J.encode(J.pixels(16, 16, "photo"), quality=90, progressive=True), encode_png(J.pixels(8, 8, "smooth")), b"", b"\xff\xd8"):
        info = ops.jpeg_probe(bad)
        q = prepare(ops, bad)
        assert not info.supported and q.reason == info.reason and q.info == info and ops.jpeg_rst_need(bad) == 0


def test_arguments(ops):
    from mv_ldm_amd import _lib as L
    lib = L.load()
    blob = J.restart_case()
    need = ops.jpeg_rst_need(blob)
    with pytest.raises(RuntimeError):
        ops.jpeg_rst_prepare(blob, np.zeros(need + 8, dtype=np.uint8), 8)               # offset not a multiple of 16
    with pytest.raises(RuntimeError):
        ops.jpeg_rst_prepare(blob, np.zeros(need - 16, dtype=np.uint8), 0)              # short room
    with pytest.raises(RuntimeError):
        ops.jpeg_rst_prepare(blob, np.zeros(need, dtype=np.uint8), need + 16)           # offset behind the buffer
    scan, desc, tables = np.zeros(need, dtype=np.uint8), np.zeros(4, dtype=np.int32), np.zeros(L.JPEG_TABLE_BYTES, dtype=np.uint8)
    args = [blob, len(blob), scan.ctypes.data, 0, need, desc.ctypes.data, tables.ctypes.data, None]
    assert lib.mvldm_jpeg_rst_prepare(*args) == 0
    for k in (0, 2, 5, 6):                              # null pointers
        broken = list(args)
        broken[k] = None
        assert lib.mvldm_jpeg_rst_prepare(*broken) == -1
    p = prepare(ops, blob)
    info = p.info
    for bad in (16, 48, -32, 1 << 17):
        with pytest.raises(RuntimeError):
            ops.jpeg_rst_entropy_emul(p.scan, p.desc, p.tables, info.h, info.w, info.sampling, subseq_bits=bad)
    coef, qt, st = np.zeros(ops.jpeg_coef_count(info.h, info.w, info.sampling), np.int16), np.zeros(192, np.uint16), np.zeros(4, np.int32)
    eargs = [p.scan.ctypes.data, p.scan.size, p.desc.ctypes.data, p.tables.ctypes.data, 1, info.h, info.w, info.sampling, coef.ctypes.data, qt.ctypes.data,
             st.ctypes.data, 0, 0]
    assert lib.mvldm_jpeg_rst_entropy_emul_host(*eargs) == 0 and st[0] == 0
    for k in (0, 2, 3, 8, 9, 10):
        broken = list(eargs)
        broken[k] = None
        assert lib.mvldm_jpeg_rst_entropy_emul_host(*broken) == -1
    # a descriptor that does not fit the buffer or the frame is refused without a read
    off, n, occupied, ri = (int(v) for v in p.desc)
    for bad in ([off + 8, n, occupied, ri], [off, n, p.scan.size, ri], [-16, n, occupied, ri], [p.scan.size + 16, n, occupied, ri], [off, n + 1, occupied, ri],
                [off, n, occupied, ri + 3], [off, 0, occupied, ri], [off, n, 8 * n, ri], [off, n, occupied, 0]):
        st = ops.jpeg_rst_entropy_emul(p.scan, np.array(bad, dtype=np.int32), p.tables, info.h, info.w, info.sampling)[2]
        assert st[0, 0] == 3 and st[0, 1] == 0 and st[0, 3] == 0, bad
    # a table entry that points outside the region (far outside the buffer: a read would leave the process's memory), is misaligned,
    # empty, or lies inside the table: CORRUPT, and nothing of the scan is read
    for g, change in ((1, lambda o, bits: (1 << 30, 64)), (0, lambda o, bits: (-4, 64)), (2, lambda o, bits: (o, 1 << 30)), (1, lambda o, bits: (o, 0)),
                      (0, lambda o, bits: (8, 64)), (2, lambda o, bits: (o + 2, bits))):
        scan = p.scan.copy()
        table = scan[off:off + 8 * n].view(np.int32).reshape(n, 2)
        table[g] = change(int(table[g, 0]), int(table[g, 1]))
        st = ops.jpeg_rst_entropy_emul(scan, p.desc, p.tables, info.h, info.w, info.sampling)[2]
        assert tuple(st[0]) == (3, 0, 0, n), (g, table[g], st)
