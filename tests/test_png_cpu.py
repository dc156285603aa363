"""CPU: the PNG reader's host half and the kernel's host twin (`mvldm_png_unfilter_host`: the kernel's arithmetic, csrc/png_common.h) against
Pillow and against the pixels each case was made from, byte for byte.  The frames come from tests/png_cases.py, a writer that is told which
filter every row takes; the files Pillow writes itself are the last section.  The kernel is pinned to the twin in tests/test_hip_png.py."""
import numpy as np
import pytest
import torch

import png_cases as PC

PIL = pytest.importorskip("PIL")


@pytest.fixture(scope="module")
def ops():
    from mv_ldm_amd import _build
    _build.build()
    from mv_ldm_amd import ops
    return ops


def check(ops, blob, want, what=""):
    """the frame takes the library's path, and gives the pixels it was made from, which are Pillow's"""
    assert np.array_equal(PC.pillow(blob), want), f"{what}: the writer and Pillow disagree"
    reason, got = ops.png_decode_host(blob)
    assert reason == 0, (what, reason)
    assert got.dtype == np.uint8 and np.array_equal(got, want), what


# ---- filters and sizes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype,depth", PC.SUPPORTED)
def test_every_filter_on_every_row_and_cycling(ops, ctype, depth):
    for f in (*PC.FILTERS, "cycle", "cycle+3", "cycle+4"):          # cycle+3 / +4: Average / Paeth on the first row (zero row above)
        blob, want = PC.case(13, 21, ctype, depth, f)
        check(ops, blob, want, (ctype, depth, f))


@pytest.mark.parametrize("content", ["noise", "flat", "smooth"])
def test_contents(ops, content):
    for ctype, depth in PC.SUPPORTED:
        blob, want = PC.case(20, 19, ctype, depth, "cycle", content=content)
        check(ops, blob, want, (ctype, depth, content))


@pytest.mark.parametrize("h", [1, 2, 63, 64, 65, 129])              # the kernel's band edges; the twin walks the same rows
def test_heights_and_widths(ops, h):
    for w in (1, 2, 3, 17):
        for ctype, depth in ((2, 8), (6, 8), (4, 8), (3, 2)):
            for f in ("cycle", 4, 3):
                blob, want = PC.case(h, w, ctype, depth, f)
                check(ops, blob, want, (h, w, ctype, depth, f))


def test_strides_of_every_residue(ops):
    seen = set()
    for ctype, depth, w in ((0, 8, 4), (0, 8, 5), (0, 8, 6), (0, 8, 7), (2, 8, 3), (2, 8, 4), (4, 8, 5), (6, 8, 3), (3, 4, 9), (3, 1, 17)):
        stride = (w * PC.CHANNELS[ctype] * depth + 7) // 8
        seen.add(stride % 4)
        blob, want = PC.case(9, w, ctype, depth, "cycle+1")
        check(ops, blob, want, (ctype, depth, w))
    assert seen == {0, 1, 2, 3}


# ---- formats ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,w", [(1, 13), (2, 7), (4, 5), (8, 9), (1, 8), (2, 4), (4, 2)])     # partial and whole last bytes
def test_palette_depths(ops, depth, w):
    blob, want = PC.case(11, w, 3, depth, "cycle")
    check(ops, blob, want, (depth, w))


def test_short_palette_trns_and_split_idat(ops):
    blob, want = PC.case(10, 12, 3, 8, "cycle", entries=37)                                  # fewer than 256 entries, every index inside
    check(ops, blob, want, "short palette")
    blob, want = PC.case(10, 12, 3, 4, 4, entries=5, trns=bytes([0, 128, 255]))             # tRNS plays no part in convert("RGB")
    check(ops, blob, want, "palette + tRNS")
    blob, want = PC.case(10, 12, 2, 8, "cycle", trns=bytes([0, 1, 0, 2, 0, 3]))
    check(ops, blob, want, "RGB + tRNS")
    blob, want = PC.case(40, 33, 6, 8, "cycle", idat_split=7, level=9)                       # many small IDAT chunks
    assert blob.count(b"IDAT") > 20
    check(ops, blob, want, "split IDAT")
    blob, want = PC.case(40, 33, 2, 8, "cycle", level=0)                                     # stored blocks
    check(ops, blob, want, "level 0")


def test_palette_index_beyond_plte_is_flagged(ops):
    """Pillow 12 gives black for such a pixel; the library does not lean on that: the frame is flagged (and `png_decode` sends it to Pillow)"""
    from mv_ldm_amd import _lib as L
    a = PC.samples(6, 9, 3, 8, "noise", entries=256)
    a[0, 0] = 12                                                                             # one index past the 12 entries, at the very least
    blob = PC.write_png(a, 3, 8, "cycle", pal=PC.palette(12))
    reason, got = ops.png_decode_host(blob)
    assert reason == L.PNG_PALETTE_INDEX
    inside = a < 12
    assert np.array_equal(got[inside], PC.palette(12)[a[inside]]) and not got[~inside].any()


# ---- Paeth: the tie order and the signed arithmetic -----------------------------------------------------------------------------------
def test_paeth_triples(ops):
    edge = (0, 1, 127, 128, 254, 255)
    tri = np.array([(a, b, c) for a in edge for b in edge for c in edge], dtype=np.uint8)
    tri = np.concatenate([tri, np.random.default_rng(7).integers(0, 256, (4096, 3)).astype(np.uint8)])
    n = len(tri)
    img = np.zeros((2, 2 * n), dtype=np.uint8)                      # pixel (1, 2i + 1): left a, above b, above-left c
    img[0, 0::2], img[0, 1::2], img[1, 0::2] = tri[:, 2], tri[:, 1], tri[:, 0]
    img[1, 1::2] = np.random.default_rng(8).integers(0, 256, n)
    for ctype in (0, 3):
        blob = PC.write_png(img, ctype, 8, [0, 4], pal=PC.palette(256))
        check(ops, blob, PC.expected(img, ctype, 8, PC.palette(256)), f"paeth triples, colour type {ctype}")


# ---- both output kinds ----------------------------------------------------------------------------------------------------------------
def test_float_output_is_k_over_255_for_every_k(ops):
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    blob = PC.write_png(img, 0, 8, "cycle")
    reason, got = ops.png_decode_host(blob, out="float")
    want = torch.from_numpy(PC.pillow(blob)).permute(2, 0, 1).float() / 255
    assert reason == 0 and got.dtype == np.float32 and torch.equal(torch.from_numpy(got), want)
    assert sorted(set(got[0].ravel().view(np.uint32))) == sorted(set((torch.arange(256).float() / 255).numpy().view(np.uint32)))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _refusals():
    from mv_ldm_amd import _lib as L
    rgb = PC.samples(9, 11, 2, 8)
    yield "interlaced", PC.write_png(rgb, 2, 8, interlace=True), L.PNG_INTERLACE
    yield "16-bit", PC.write_png(PC.samples(9, 11, 2, 16), 2, 16), L.PNG_DEPTH16
    yield "2-bit grey", PC.write_png(PC.samples(9, 11, 0, 2), 0, 2), L.PNG_GREY_BITS
    five = bytearray(PC.filter_rows(PC.pack_rows(rgb, 2, 8), 3, [0] * 9))
    five[4 * 34] = 5
    yield "filter byte 5", PC.write_png(rgb, 2, 8, stream_edit=lambda s: bytes(five)), L.PNG_FILTER
    yield "short stream", PC.write_png(rgb, 2, 8, "cycle", stream_edit=lambda s: s[:-1]), L.PNG_LENGTH
    yield "trailing bytes", PC.write_png(rgb, 2, 8, "cycle", stream_edit=lambda s: s + b"\0"), L.PNG_LENGTH
    yield "flipped CRC", PC.write_png(rgb, 2, 8, "cycle", flip_crc="IDAT"), L.PNG_CRC
    yield "flipped header CRC", PC.write_png(rgb, 2, 8, "cycle", flip_crc="IHDR"), L.PNG_CRC
    yield "no PLTE", PC.write_png(PC.samples(9, 11, 3, 8), 3, 8, plte=False), L.PNG_NO_PLTE
    yield "not a PNG", b"\xff\xd8\xff\xe0" + bytes(40), L.PNG_NOT_PNG


def test_refusals_name_their_reason_and_leave_dst_alone(ops):
    seen = []
    for name, blob, reason in _refusals():
        for out, dtype, shape in (("uint8", np.uint8, (9, 11, 3)), ("float", np.float32, (3, 9, 11))):
            count = int(np.prod(shape))
            room = np.full(count + 128, 0xA5, dtype=np.uint8).view(dtype) if dtype == np.uint8 else np.full(count + 128, -7.0, dtype=np.float32)
            before = room.copy()
            got_reason, got = ops.png_decode_host(blob, dst=room[64:64 + count].reshape(shape), out=out)
            assert got_reason == reason and got is None, (name, got_reason, reason)
            assert np.array_equal(room, before), f"{name}: dst or its guards were written"
        assert ops.png_probe(blob).supported == (name not in ("interlaced", "16-bit", "2-bit grey", "flipped header CRC", "not a PNG")), name
        seen.append(name)
    assert len(seen) == 10


def test_a_supported_frame_writes_dst_and_only_dst(ops):
    blob, want = PC.case(9, 11, 6, 8, "cycle")
    room = np.full(9 * 11 * 3 + 128, 0xA5, dtype=np.uint8)
    reason, got = ops.png_decode_host(blob, dst=room[64:-64].reshape(9, 11, 3))
    assert reason == 0 and np.array_equal(room[64:-64].reshape(9, 11, 3), want) and (room[:64] == 0xA5).all() and (room[-64:] == 0xA5).all()


def test_twin_refuses_descriptors_that_do_not_fit(ops):
    """the check the kernel applies (png_desc_ok), on the host: an offset, a length, a palette or a format that does not fit leaves the
    frame alone; the frames around it are decoded"""
    from mv_ldm_amd import _lib as L
    h, w = 5, 7
    rgb = PC.samples(h, w, 2, 8)
    stream = np.frombuffer(PC.filter_rows(PC.pack_rows(rgb, 2, 8), 3, PC.row_filters(h, "cycle")), dtype=np.uint8)
    need = stream.size
    streams = np.concatenate([stream, stream])
    pal = np.zeros(30, dtype=np.uint8)
    good = (0, 2, 8, 0, 0, 0, 0, 0)
    rows = [good, (need + 1, 2, 8, 0, 0, 0, 0, 0), (-1, 2, 8, 0, 0, 0, 0, 0), (need, 6, 8, 0, 0, 0, 0, 0), (0, 2, 16, 0, 0, 0, 0, 0), (0, 0, 4, 0, 0, 0, 0, 0),
            (0, 3, 8, 0, 11, 0, 0, 0), (0, 3, 8, 29, 1, 0, 0, 0), (0, 3, 8, 0, 0, 0, 0, 0), (0, 3, 8, 0, 257, 0, 0, 0), (0, 5, 8, 0, 0, 0, 0, 0),
            (2 ** 31 - 1, 2, 8, 0, 0, 0, 0, 0), (need, 2, 8, 0, 0, 0, 0, 0)]
    desc = np.array(rows, dtype=np.int32)
    dst = np.full((len(rows), h, w, 3), 0xA5, dtype=np.uint8)
    status = ops.png_unfilter_host(streams, desc, pal, h, w, dst)
    assert status.tolist() == [0] + [L.PNG_DESC] * (len(rows) - 2) + [0]
    assert np.array_equal(dst[0], rgb) and np.array_equal(dst[-1], rgb) and (dst[1:-1] == 0xA5).all()


# ---- files Pillow wrote -----------------------------------------------------------------------------------------------------------------
def _pillow_files():
    h, w = 48, 64
    rgba = PC.samples(h, w, 6, 8, "photo")
    idx = PC.samples(h, w, 3, 8, "photo", entries=200)
    return {"RGB": PC.pillow_file(rgba[..., :3].copy(), "RGB"), "RGBA": PC.pillow_file(rgba, "RGBA"), "L": PC.pillow_file(rgba[..., 0].copy(), "L"),
            "LA": PC.pillow_file(rgba[..., ::3].copy(), "LA"), "P": PC.pillow_file(idx, "P", PC.palette(200))}


def test_files_pillow_wrote(ops, tmp_path):
    from mv_ldm_amd.image_io import decode_png
    files = _pillow_files()
    assert len(PC.filter_types(files["RGB"])) >= 3, "Pillow chose fewer than three filter types: the case went soft"
    for mode, blob in files.items():
        info = ops.png_probe(blob)
        assert info.supported and (info.h, info.w) == (48, 64) and info.color_type == {"RGB": 2, "RGBA": 6, "L": 0, "LA": 4, "P": 3}[mode]
        reason, got = ops.png_decode_host(blob)
        assert reason == 0 and np.array_equal(got, PC.pillow(blob)), mode
    with pytest.raises(AssertionError):                             # what every tool met before: `decode_png` reads its own writer's files only
        decode_png(files["RGB"])


def test_load_images_reads_what_pillow_wrote(ops, tmp_path):
    """`image_io.load_images` (here through the host twin: no device) on a Pillow-written tree, mixed with `save_image`'s own files, in the
    order of the paths; every frame took the library's path"""
    from mv_ldm_amd.image_io import group_by_size, load_image, load_images, save_image
    files = _pillow_files()
    paths = []
    for mode, blob in files.items():
        paths.append(tmp_path / f"{mode}.png")
        paths[-1].write_bytes(blob)
    own = torch.rand(3, 48, 64)
    paths.insert(2, tmp_path / "own.png")
    save_image(own, paths[2])
    info = {}
    got = load_images(paths, "cpu", info=info)
    want = torch.stack([torch.from_numpy(PC.pillow(p.read_bytes())).permute(2, 0, 1).float() / 255 for p in paths])
    assert got.dtype == torch.float32 and tuple(got.shape) == (6, 3, 48, 64) and torch.equal(got, want)
    assert torch.equal(got[2], load_image(paths[2])) and info["fallback"] == []
    as_bytes = load_images(paths, "cpu", out="uint8")
    assert as_bytes.dtype == torch.uint8 and torch.equal(as_bytes.permute(0, 3, 1, 2).float() / 255, want)
    save_image(torch.rand(3, 5, 4), tmp_path / "small.png")
    assert group_by_size(paths + [tmp_path / "small.png"]) == {(48, 64): [0, 1, 2, 3, 4, 5], (5, 4): [6]}
    with pytest.raises(ValueError, match="one size"):
        load_images(paths + [tmp_path / "small.png"], "cpu")


def test_png_decode_on_the_host_mixes_paths_and_counts_fallbacks(ops):
    """the batch driver without a device: refused frames go through Pillow into their slots, the others through the twin"""
    blobs, want = [], []
    for ctype, depth in PC.SUPPORTED:
        blob, exp = PC.case(9, 11, ctype, depth, "cycle")
        blobs.append(blob)
        want.append(exp)
    rgb = PC.samples(9, 11, 2, 8)
    blobs += [PC.write_png(rgb, 2, 8, interlace=True), PC.write_png(PC.samples(9, 11, 2, 16), 2, 16)]
    info = {}
    got = ops.png_decode(blobs, device="cpu", info=info)
    assert [i for i, _ in info["fallback"]] == [8, 9] and [r for _, r in info["fallback"]] == ["interlaced", "16-bit samples"]
    for i, blob in enumerate(blobs):
        assert np.array_equal(got[i].numpy(), PC.pillow(blob)), i
    for i, exp in enumerate(want):
        assert np.array_equal(got[i].numpy(), exp), i
    with pytest.raises(ValueError, match="one size"):
        ops.png_decode([blobs[0], PC.case(9, 12, 2, 8)[0]], device="cpu")
    broken = PC.write_png(rgb, 2, 8, "cycle", stream_edit=lambda s: s[:40])
    with pytest.raises(Exception) as e:                             # Pillow's own error for a broken file is the caller's
        ops.png_decode([broken], device="cpu")
    with pytest.raises(type(e.value)):
        PC.pillow(broken)
