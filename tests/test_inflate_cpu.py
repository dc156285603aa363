"""CPU: the device inflate's host twin (csrc/inflate_host.cpp: the kernel's step functions with loops in place of lanes) against
`zlib.decompress`, byte for byte, over every stream of tests/inflate_cases.py; the refusals of a corrupted stream with their reasons; 500
single-bit flips (the twin may refuse more than zlib, never accept what zlib refuses or give other bytes); writes confined to the slot;
`png_decode(device="cpu", inflate="device")` against Pillow.

Two cases the issue lists cannot be accepted by the interface it specifies: the 1-byte and the empty payload.  The output of a frame is
need = h * (1 + stride) >= 2 bytes by `png_desc_ok`, so these valid streams are inflated, their check sums verified, and reported as
MVLDM_PNG_LENGTH (test_streams_shorter_than_any_frame)."""
import zlib

import numpy as np
import pytest

import inflate_cases as IC
import png_cases as PC


@pytest.fixture(scope="module")
def ops():
    from mv_ldm_amd import _build
    _build.build()
    from mv_ldm_amd import ops
    return ops


def twin(ops, streams, infos, h, w, guard=64):
    """(status, output buffer, slot offsets) of one twin call over streams [(z)] with infos [(colour type, depth, need)]"""
    zbuf, zdesc, desc, soffs, send = IC.pack(streams, infos, guard)
    out = np.full(send, 0xA5, dtype=np.uint8)
    status = ops.png_inflate_host(zbuf, zdesc, out, desc, h, w)
    assert IC.guards_intact(out, soffs, [n for _, _, n in infos], guard), "the twin wrote outside a slot"
    return status, out, soffs


def test_room_is_round_up_16_plus_16():
    from mv_ldm_amd import _lib as L
    lib = L.load()
    assert [lib.mvldm_png_inflate_room(b) for b in (0, 1, 15, 16, 17, 910)] == [16, 32, 32, 32, 48, 912 + 16]


def test_twin_equals_zlib_on_every_case(ops):
    IC.self_check()                                         # the streams hold the blocks, matches and distances they are meant to
    groups = {}
    for c in IC.cases():
        groups.setdefault((c.h, c.w), []).append(c)
    assert len(groups) == 3
    seen = 0
    for (h, w), group in groups.items():
        status, out, soffs = twin(ops, [c.z for c in group], [(c.ctype, c.depth, c.need) for c in group], h, w)
        for i, c in enumerate(group):
            assert status[i] == 0, (c.name, int(status[i]))
            assert out[soffs[i]:soffs[i] + c.need].tobytes() == zlib.decompress(c.z), c.name
            seen += 1
    assert seen == len(IC.cases()) == 54


def test_streams_shorter_than_any_frame(ops):
    from mv_ldm_amd import _lib as L
    tiny = IC.tiny_cases()
    status, out, soffs = twin(ops, [z for _, z in tiny], [(0, 8, 2)] * len(tiny), 1, 1)
    assert status.tolist() == [L.PNG_LENGTH] * len(tiny)
    bad = [zlib.compress(b"\x00", 6)[:-1] + b"\x07", zlib.compress(b"", 6)[:-1] + b"\x07"]         # the same with a wrong check sum: not a length matter
    status, out, soffs = twin(ops, bad, [(0, 8, 2)] * 2, 1, 1)
    assert status.tolist() == [L.PNG_INFLATE] * 2


def test_corruptions_are_refused_with_their_reason(ops):
    from mv_ldm_amd import _lib as L
    rows = IC.corruptions()
    status, out, soffs = twin(ops, [z for _, z, _, _ in rows], [(3, 4, 4201)] * len(rows), 1, IC.W)
    for i, (name, z, payload, allowed) in enumerate(rows):
        assert status[i] in allowed, (name, int(status[i]))
        if payload is not None:
            assert out[soffs[i]:soffs[i] + 4201].tobytes() == payload, name
        else:
            try:                                            # what the reference says of the same bytes: an error, no end, bytes behind it, or another length
                d = zlib.decompressobj()
                raw = d.decompress(z)
                assert len(raw) != 4201 or not d.eof or d.unused_data or name == "filter byte 5", name
            except zlib.error:
                pass
    assert [s for s in status.tolist() if s == 0] == [0, 0] and len(rows) == 12


def test_500_bit_flips_never_accept_what_zlib_refuses(ops):
    rows = IC.corruptions()
    z, payload = rows[0][1], rows[0][2]
    rng = np.random.default_rng(PC._seed("flips"))
    flipped = []
    for bit in rng.integers(0, 8 * len(z), 500):
        b = bytearray(z)
        b[bit >> 3] ^= 1 << (bit & 7)
        flipped.append(bytes(b))
    status, out, soffs = twin(ops, flipped, [(3, 4, 4201)] * 500, 1, IC.W)
    accepted = 0
    for i, f in enumerate(flipped):
        if status[i] == 0:
            assert out[soffs[i]:soffs[i] + 4201].tobytes() == zlib.decompress(f), i      # raises where zlib refuses
            accepted += 1
    assert accepted <= 10, accepted                         # zlib ignores only the up to 7 padding bits between the last block and the trailer


def test_bad_descriptors_are_skipped(ops):
    from mv_ldm_amd import _lib as L
    c = IC.cases()[0]
    zbuf, zdesc, desc, soffs, send = IC.pack([c.z] * 5, [(c.ctype, c.depth, c.need)] * 5)
    desc[1] = (0, -1, 0, 0, 0, 0, 0, 0)                     # the no-frame descriptor of a frame the host refused
    zdesc[2, 0] += 8                                        # an offset that is no multiple of 16
    zdesc[3, 1] = zbuf.size                                 # a stream that runs past the buffer
    desc[4, 0] = send - c.need + 1                          # a slot that runs past the buffer
    out = np.full(send, 0xA5, dtype=np.uint8)
    status = ops.png_inflate_host(zbuf, zdesc, out, desc, c.h, c.w)
    assert status.tolist() == [0, L.PNG_DESC, L.PNG_DESC, L.PNG_DESC, L.PNG_DESC]
    assert out[soffs[0]:soffs[0] + c.need].tobytes() == c.payload and IC.guards_intact(out, soffs[:1], [c.need])


def test_png_decode_with_the_twin_equals_pillow():
    PIL = pytest.importorskip("PIL")
    from mv_ldm_amd import _build
    _build.build()
    from mv_ldm_amd import ops
    blobs, want = [], []
    for ctype, depth in PC.SUPPORTED:                       # all eight formats at 5 x 7, IDAT in 1-byte chunks
        blob, exp = PC.case(5, 7, ctype, depth, "cycle", idat_split=1)
        blobs.append(blob)
        want.append(exp)
    modes = {(2, 8): "RGB", (6, 8): "RGBA", (0, 8): "L", (4, 8): "LA", (3, 8): "P"}
    for (ctype, depth), mode in modes.items():              # and as Pillow writes them
        pal = PC.palette(256) if ctype == 3 else None
        blobs.append(PC.pillow_file(PC.samples(5, 7, ctype, depth, "photo"), mode, pal))
        want.append(PC.pillow(blobs[-1]))
    for out in ("uint8", "float"):
        info = {}
        got = ops.png_decode(blobs, device="cpu", out=out, info=info, inflate="device")
        assert info["fallback"] == [], info
        same = ops.png_decode(blobs, device="cpu", out=out)
        assert got.dtype == same.dtype and np.array_equal(got.numpy(), same.numpy())
        if out == "uint8":
            for i, blob in enumerate(blobs):
                assert np.array_equal(got[i].numpy(), want[i]) and np.array_equal(got[i].numpy(), PC.pillow(blob)), i
    with pytest.raises(ValueError, match="inflate"):
        ops.png_decode(blobs, device="cpu", inflate="gpu")


def test_png_decode_names_the_same_fallbacks_on_either_path():
    PIL = pytest.importorskip("PIL")
    from mv_ldm_amd import ops
    blobs, names = IC.refusal_frames(9, 11, palette_index=False)      # the host path with device="cpu" does not act on the twin's palette flag
    fine, exp = PC.case(9, 11, 2, 8, "cycle")
    mixed = [fine] + blobs + [fine]
    a, b = {}, {}
    got = ops.png_decode(mixed, device="cpu", info=a, inflate="device")
    ref = ops.png_decode(mixed, device="cpu", info=b)
    assert a["fallback"] == b["fallback"] == [(i + 1, n) for i, n in enumerate(names)]
    assert np.array_equal(got.numpy(), ref.numpy()) and np.array_equal(got[0].numpy(), exp)
    for i, blob in enumerate(mixed):
        assert np.array_equal(got[i].numpy(), PC.pillow(blob)), i
