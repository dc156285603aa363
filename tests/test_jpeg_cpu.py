"""CPU: the JPEG decoder's host side (csrc/jpeg_host.cpp through `ops.jpeg_probe` / `jpeg_entropy` / `jpeg_idct_host`) against Pillow's own
decode of the same bytes, `np.array_equal` everywhere: the marker parser, the Huffman decoder, the range guard, the refusals, and the
plain C++ restatement of the device half (the same inline arithmetic the kernels run: csrc/jpeg_common.h).  Frames: tests/jpeg_cases.py."""
import ctypes as C
import json
from io import BytesIO
from pathlib import Path

import numpy as np
import pytest

import jpeg_cases as J

CANARY = 0x5A5A
GUARD = 5905                        # csrc/jpeg_common.h kJpegGuard


@pytest.fixture(scope="module")
def ops():
    from mv_ldm_amd import _build, _lib, ops
    _build.build()
    _lib.load()
    return ops


def decode(ops, blob, expect_reason=0):
    """probe + entropy + host IDCT with canaries around both host buffers -> (pixels or None, reason, largest S)"""
    info = ops.jpeg_probe(blob)
    count = ops.jpeg_coef_count(info.h, info.w, info.sampling) if info.supported else 4096
    coef = np.full(count + 128, CANARY, dtype=np.int16)
    qt = np.full(192 + 128, CANARY, dtype=np.uint16)
    reason, max_s = ops.jpeg_entropy(blob, coef[64:64 + count], qt[64:64 + 192])
    for buf in (coef, qt):
        assert (buf[:64] == CANARY).all() and (buf[-64:] == CANARY).all(), "a write outside the caller's buffer"
    if not info.supported:
        assert reason == info.reason
    assert reason == expect_reason, (reason, expect_reason)
    if reason != 0:
        return None, reason, max_s
    return ops.jpeg_idct_host(coef[64:64 + count].copy(), qt[64:64 + 192].copy(), info.h, info.w, info.sampling), reason, max_s


@pytest.mark.parametrize("h,w", J.SIZES, ids=lambda v: str(v))
def test_parity_with_pillow(ops, h, w):
    """every subsampling x quality x content at this size: the guard accepts the frame (nothing passes by falling back), and the bytes are
    Pillow's"""
    for name, blob in J.small_cases(h, w):
        got, reason, max_s = decode(ops, blob)
        assert reason == 0 and max_s <= GUARD, (name, reason, max_s)
        assert np.array_equal(got, J.pillow(blob)), name


@pytest.mark.parametrize("h,w", J.SIZES, ids=lambda v: str(v))
def test_probe_agrees_with_pillow(ops, h, w):
    from PIL import Image
    for name, blob in J.small_cases(h, w):
        im = Image.open(BytesIO(blob))
        info = ops.jpeg_probe(blob)
        assert info.supported and (info.w, info.h) == im.size, name
        hs, vs = im.layer[0][1], im.layer[0][2]
        assert all(tuple(layer[1:3]) == (1, 1) for layer in im.layer[1:])
        assert info.sampling == {(1, 1): 1, (2, 1): 2, (2, 2): 3}[(hs, vs)], name
        mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
        assert (info.mcu_cols, info.mcu_rows, info.luma_blocks, info.chroma_blocks) == (mcux, mcuy, mcux * mcuy * hs * vs, mcux * mcuy), name
        assert ops.jpeg_coef_count(h, w, info.sampling) == 64 * (info.luma_blocks + 2 * info.chroma_blocks)
    gray = ops.jpeg_probe(J.gray_case())
    assert gray.supported and (gray.h, gray.w, gray.sampling, gray.chroma_blocks) == (45, 81, 0, 0) and gray.luma_blocks == 6 * 11
    assert ops.jpeg_coef_count(0, 8, 1) == 0 and ops.jpeg_coef_count(8, 8, 4) == 0 and ops.jpeg_coef_count(8, 16385, 1) == 0


def test_grayscale(ops):
    blob = J.gray_case()
    got, reason, _ = decode(ops, blob)
    assert np.array_equal(got, J.pillow(blob)) and (got[..., 0] == got[..., 1]).all()


def test_restart_markers(ops):
    blob = J.restart_case()
    assert b"\xff\xdd" in blob and b"\xff\xd0" in blob and b"\xff\xd1" in blob      # DRI and RSTn are really there
    got, reason, _ = decode(ops, blob)
    assert np.array_equal(got, J.pillow(blob))
    # a restart marker out of sequence is corrupt, not decoded
    at = blob.index(b"\xff\xd1")
    assert decode(ops, blob[:at] + b"\xff\xd3" + blob[at + 2:], expect_reason=3)[1] == 3


def test_range_guard(ops):
    """a noise frame with its quantisation tables overwritten in the stream: a small value keeps every block within the guard and the
    bytes are Pillow's; 255 takes blocks far outside it and the frame is refused (Pillow's SIMD path saturates there, libjpeg's C path
    masks: no one answer to reproduce)"""
    blob = J.encode(J.pixels(45, 81, "noise"), quality=50, subsampling=2)
    small = J.with_dqt(blob, 8)
    got, reason, max_s = decode(ops, small)
    assert reason == 0 and 0 < max_s <= GUARD
    assert np.array_equal(got, J.pillow(small))
    wide = J.with_dqt(blob, 255)
    _, reason, max_s = decode(ops, wide, expect_reason=12)
    assert max_s > GUARD
    assert ops.jpeg_probe(wide).supported          # the markers are fine: only the scan tells


def test_refusals(ops):
    a = J.pixels(24, 40, "smooth")
    from PIL import Image
    progressive = J.encode(a, quality=90, progressive=True)
    assert decode(ops, progressive, expect_reason=4)[1] == 4 and (ops.jpeg_probe(progressive).h, ops.jpeg_probe(progressive).w) == (24, 40)
    buf = BytesIO()
    Image.fromarray(a).convert("CMYK").save(buf, format="JPEG", quality=90)
    assert decode(ops, buf.getvalue(), expect_reason=7)[1] == 7
    assert decode(ops, J.encode(a, quality=90, subsampling=0, optimize=True))[1] == 0           # optimised Huffman tables are still baseline
    assert decode(ops, b"\x89PNG\r\n\x1a\n" + bytes(64), expect_reason=1)[1] == 1
    assert decode(ops, b"", expect_reason=1)[1] == 1
    rgb = J.encode(a, quality=90, subsampling=0)
    adobe = rgb[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + rgb[2 + 2 + int.from_bytes(rgb[4:6], "big"):]       # APP14 instead of JFIF
    assert decode(ops, adobe, expect_reason=9)[1] == 9


def test_truncated_streams(ops):
    """a stream cut anywhere -- inside every header segment, inside the scan, in front of EOI -- is reported truncated, and nothing is
    written outside the caller's buffers (the canaries of `decode`)"""
    blob = J.encode(J.pixels(17, 33, "noise"), quality=90, subsampling=2)
    start = J.scan_start(blob)
    assert 100 < start < len(blob) - 100
    cuts = sorted(set(range(2, len(blob))))
    for cut in cuts:
        assert decode(ops, blob[:cut], expect_reason=2)[1] == 2, cut
    assert decode(ops, blob[:1], expect_reason=1)[1] == 1
    restart = J.restart_case()
    for cut in (J.scan_start(restart) + 1, restart.index(b"\xff\xd0") + 1, restart.index(b"\xff\xd1"), len(restart) // 2, len(restart) - 2, len(restart) - 1):
        assert decode(ops, restart[:cut], expect_reason=2)[1] == 2, cut
    # a byte of the scan replaced by a marker that cannot stand there
    assert decode(ops, blob[:start + 40] + b"\xff\xc0" + blob[start + 42:], expect_reason=3)[1] == 3


def test_argument_checks(ops):
    from mv_ldm_amd import _lib as L
    lib = L.load()
    blob = J.encode(J.pixels(24, 40, "smooth"), quality=90, subsampling=2)
    count = ops.jpeg_coef_count(24, 40, 3)
    coef = np.full(count + 64, CANARY, dtype=np.int16)
    qt = np.zeros(192, dtype=np.uint16)
    assert lib.mvldm_jpeg_entropy(blob, len(blob), coef.ctypes.data, count - 1, qt.ctypes.data, None) == -1      # short: refused before any write
    assert (coef == CANARY).all()
    assert lib.mvldm_jpeg_entropy(blob, len(blob), None, count, qt.ctypes.data, None) == -1
    assert lib.mvldm_jpeg_probe(None, 0, (C.c_int32 * 8)()) == -1
    assert lib.mvldm_jpeg_idct_host(coef.ctypes.data, qt.ctypes.data, None, 24, 40, 3) == -1
    assert lib.mvldm_jpeg_idct_host(coef.ctypes.data, qt.ctypes.data, coef.ctypes.data, 24, 40, 7) == -1
    ws = lib.mvldm_jpeg_workspace_bytes
    assert ws(5, 360, 640, 3) == 5 * 64 * (23 * 40 * 6) and ws(1, 8, 8, 0) == 64 and ws(0, 8, 8, 0) == 0 and ws(1, 8, 8, 9) == 0
    # the device entry checks its arguments before it touches a device
    p = 1 << 20
    call = lambda coef=p, qt=p, dst=p, n=2, h=24, w=40, s=3, wsp=p, wsb=1 << 20: lib.mvldm_jpeg_decode(coef, qt, dst, n, h, w, s, wsp, wsb, None)
    assert call(coef=None) == -1 and call(qt=p + 2) == -1 and call(dst=p + 1) == -1 and call(wsp=None) == -1
    assert call(wsb=2 * count - 1) == -1 and call(s=4) == -1 and call(h=0) == -1 and call(w=16385) == -1 and call(n=-1) == -1
    assert lib.mvldm_jpeg_decode(None, None, None, 0, 24, 40, 3, None, 0, None) == 0                              # nothing to do


def test_golden_frame(ops):
    """360 x 640, 4:2:0, quality 90: the dataset's frame size, by SHA-256 (tests/golden/jpeg.json from tests/golden/make_jpeg_golden.py)"""
    gold = json.loads((Path(__file__).parent / "golden" / "jpeg.json").read_text())
    assert J.sha256(J.pixels(*J.BIG, "photo")) == gold["pixels_sha256"]
    blob = J.big_case()
    assert J.sha256(blob) == gold["stream_sha256"], "this Pillow encodes the frame differently: regenerate tests/golden/jpeg.json"
    got, reason, max_s = decode(ops, blob)
    assert reason == 0 and max_s <= GUARD
    assert J.sha256(got) == gold["decoded_sha256"] == J.sha256(J.pillow(blob))


def test_dataset_frame_size_through_the_probe(ops):
    from mv_ldm_amd import dataset as D
    for blob in (J.big_case(), J.gray_case(), J.encode(J.pixels(24, 40, "smooth"), quality=90, progressive=True)):
        assert D._frame_size(blob, probe=True) == D._frame_size(blob)


def test_kernels_use_no_scratch(ops):
    """both kernels are in the build's resource report, with no scratch and no spills (a runtime index into the layout struct, or the
    8-value row demoted from registers, would show here and nowhere else)"""
    from mv_ldm_amd import _build
    res = json.loads(_build.RES.read_text())
    mine = {k: v for k, v in res.items() if "jpeg_idct_kernel" in k or "jpeg_color_kernel" in k}
    assert sum("jpeg_idct_kernel" in k for k in mine) == 2 and sum("jpeg_color_kernel" in k for k in mine) == 1, sorted(mine)
    assert all(v["scratch"] == 0 and v.get("vgpr_spill", 0) == 0 for v in mine.values()), mine
