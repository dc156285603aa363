"""The frames of the restart-interval tests (tests/test_jpeg_restart_cpu.py, tests/test_hip_jpeg_restart.py): tests/jpeg_cases.py's seeded
pixels encoded by Pillow with restart markers (`restart_marker_blocks` counts MCUs, `restart_marker_rows` MCU rows), a proper walk of a
scan's markers, and the damaged streams both files draw from one seed.  A helper module like tests/jpeg_cases.py."""
import numpy as np

import jpeg_cases as J

DAMAGE_SEED = 20240611


def frames():
    """(name, blob, intervals)"""
    noise = J.pixels(45, 81, "noise")
    return [
        ("noise-q100-420-ri1", J.encode(noise, quality=100, subsampling=2, restart_marker_blocks=1), 18),
        ("noise-q90-420-ri7", J.encode(noise, quality=90, subsampling=2, restart_marker_blocks=7), 3),           # a short last interval, a boundary mid-row
        ("noise-q90-420-ri100", J.encode(noise, quality=90, subsampling=2, restart_marker_blocks=100), 1),       # DRI above the MCUs: no marker
        ("photo-q90-422-ri4", J.encode(J.pixels(45, 81, "photo"), quality=90, subsampling=1, restart_marker_blocks=4), 9),
        ("gray-17x33-ri1", J.encode(J.pixels(17, 33, "noise", channels=1), quality=90, restart_marker_blocks=1), 15),
        ("noise-48x640-q100-444-rows1", J.encode(J.pixels(48, 640, "noise"), quality=100, subsampling=0, restart_marker_rows=1), 6),
        ("noise-q90-420-plain", J.encode(noise, quality=90, subsampling=2), 1),                                   # no DRI
    ]


def seam_case() -> bytes:
    """264 x 264 noise, quality 50, 4:4:4, no DRI: the frame both device entropy paths take.  33 x 33 = 1089 blocks a component, so the
    DC pass of either form runs a second pass of 1024 with a carry; about 4,700 subsequences of 32 bits, so the scan takes several chunks"""
    return J.encode(J.pixels(264, 264, "noise"), quality=50, subsampling=0)


def dri(blob: bytes) -> int:
    """the restart interval of the stream's DRI segment, 0 without one"""
    pos = 2
    while blob[pos + 1] != 0xDA:
        if blob[pos + 1] == 0xDD:
            return int.from_bytes(blob[pos + 4:pos + 6], "big")
        pos += 2 + int.from_bytes(blob[pos + 2:pos + 4], "big")
    return 0


def markers(blob: bytes):
    """a walk of the entropy-coded data: [(index of the marker's FF, its code)] of every marker from the scan's first byte on, EOI included;
    a stuffed pair FF 00 is data"""
    out, i = [], J.scan_start(blob)
    while i + 1 < len(blob):
        if blob[i] == 0xFF and blob[i + 1] != 0x00:
            at = i
            while i < len(blob) and blob[i] == 0xFF:
                i += 1
            out.append((at, blob[i]))
            if blob[i] == 0xD9:
                break
            i += 1
        else:
            i += 2 if blob[i] == 0xFF else 1
    return out


def marker_damage(blob: bytes):
    """(name, stream): two markers swapped, each marker removed, each marker doubled"""
    rst = [(at, code) for at, code in markers(blob) if 0xD0 <= code <= 0xD7]
    assert len(rst) >= 2
    out = []
    a, b = rst[0][0], rst[1][0]
    swapped = bytearray(blob)
    swapped[a + 1], swapped[b + 1] = blob[b + 1], blob[a + 1]
    out.append(("swapped", bytes(swapped)))
    for k, (at, code) in enumerate(rst):
        out.append((f"removed-{k}", blob[:at] + blob[at + 2:]))
        out.append((f"doubled-{k}", blob[:at] + blob[at:at + 2] + blob[at:]))
    return out


def flipped_sixteen():
    """sixteen seeded single-byte flips inside the interval data (never a marker's two bytes) of `J.restart_case()`"""
    blob = J.restart_case()
    taken = {at + d for at, _ in markers(blob) for d in (0, 1)}
    data = np.array([i for i in range(J.scan_start(blob), len(blob)) if i not in taken])
    rng = np.random.default_rng(DAMAGE_SEED)
    out = []
    for at, mask in zip(rng.choice(data, 16, replace=False), [0x01, 0xFF] * 8):
        bad = bytearray(blob)
        bad[int(at)] ^= mask
        out.append(bytes(bad))
    return out
