"""GPU: the PNG row-unfiltering kernel (csrc/png.hip) against its host twin and Pillow, bit for bit, at the shapes that exercise its lanes
and bands; both output kinds; writes confined to dst; `ops.png_decode` end to end with its fallback count; `metrics.score_trees` and
`cleanfid.iter_batches` on trees Pillow wrote.  Frames: tests/png_cases.py.  No test launches a descriptor meant to run past its buffers:
malformed inputs are refused on the host (tests/test_png_cpu.py pins the descriptor check itself on the twin)."""
import numpy as np
import pytest
import torch

import png_cases as PC

pytestmark = pytest.mark.gpu
PIL = pytest.importorskip("PIL")


@pytest.fixture(scope="module")
def ops():
    from mv_ldm_amd import _build
    _build.build()
    from mv_ldm_amd import ops
    return ops


def as_float(pixels: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(pixels.copy()).permute(2, 0, 1).float() / 255


def device_path(ops, blobs, out="uint8"):
    """`png_decode` of frames that must all take the device path"""
    info = {}
    got = ops.png_decode(blobs, out=out, info=info)
    assert info["fallback"] == [], info
    return got.cpu()


def all_formats(h, w, filters=("cycle", 4)):
    blobs, want = [], []
    for ctype, depth in PC.SUPPORTED:
        for f in filters:
            blob, exp = PC.case(h, w, ctype, depth, f)
            blobs.append(blob)
            want.append(exp)
    return blobs, want


# ---- the kernel against the twin and Pillow ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [1, 63, 64, 65, 129])         # one lane; a band less one row; a whole band; a band and one row (LDS hand-over); two and a row
def test_lanes_and_bands(ops, h):
    for w in (1, 3, 17, 64):
        blobs, want = all_formats(h, w)                     # every colour type x (cycling filters, all-Paeth): one launch of 16 frames
        got = device_path(ops, blobs).numpy()
        for i, blob in enumerate(blobs):
            reason, twin = ops.png_decode_host(blob)
            assert reason == 0
            assert np.array_equal(got[i], twin), (h, w, i, "kernel != host twin")
            assert np.array_equal(got[i], want[i]) and np.array_equal(got[i], PC.pillow(blob)), (h, w, i, "kernel != Pillow")


def test_every_filter_alone_and_first_rows(ops):
    blobs, want = all_formats(70, 33, filters=(0, 1, 2, 3, "cycle+3", "cycle+4"))       # Average / Paeth on the first row: the zero row above
    got = device_path(ops, blobs).numpy()
    for i in range(len(blobs)):
        assert np.array_equal(got[i], want[i]), i


def test_batch_of_70_mixed_frames(ops):
    blobs, want = [], []
    for i in range(70):                                     # more frames than one round of anything; colour types and filters mixed in one launch
        ctype, depth = PC.SUPPORTED[i % len(PC.SUPPORTED)]
        blob, exp = PC.case(32, 40, ctype, depth, f"cycle+{i % 5}", content=("noise", "photo", "flat")[i % 3], key=i)
        blobs.append(blob)
        want.append(exp)
    got = device_path(ops, blobs).numpy()
    assert np.array_equal(got, np.stack(want))
    assert np.array_equal(got[::9], np.stack([PC.pillow(b) for b in blobs[::9]]))


def test_one_256_square_rgb_frame(ops):
    a = PC.samples(256, 256, 2, 8, "photo")
    for blob in (PC.write_png(a, 2, 8, "cycle"), PC.write_png(a, 2, 8, 4), PC.pillow_file(a, "RGB")):
        got = device_path(ops, [blob]).numpy()
        assert np.array_equal(got[0], a) and np.array_equal(got[0], PC.pillow(blob))


# ---- both output kinds, confined writes ---------------------------------------------------------------------------------------------------
def test_float_output_is_torch_k_over_255(ops):
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)   # all 256 values of k
    blobs = [PC.write_png(ramp, 0, 8, "cycle"), PC.write_png(np.stack([ramp, ramp.T, ramp[::-1]], axis=-1), 2, 8, 4),
             PC.write_png(ramp, 3, 8, 3, pal=PC.palette(256))]
    got = device_path(ops, blobs, out="float")
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3, 16, 16)
    for i, blob in enumerate(blobs):
        assert torch.equal(got[i], as_float(PC.pillow(blob))), i
    assert torch.equal(got[0, 0].reshape(-1), torch.arange(256).float() / 255)
    blobs, want = all_formats(65, 17)
    got = device_path(ops, blobs, out="float")
    assert torch.equal(got, torch.stack([as_float(x) for x in want]))


def staged(ops, blobs):
    """the staging buffer `png_decode` uploads, made by its own helpers: every frame accepted on the host"""
    infos = [ops.png_probe(b) for b in blobs]
    assert all(p.supported for p in infos)
    offs, end, desc0, total = ops._png_layout(infos)
    host = np.zeros(total, dtype=np.uint8)
    desc = host[desc0:].view(np.int32).reshape(len(blobs), -1)
    for i, b in enumerate(blobs):
        assert ops._png_stage(b, infos[i], host, offs[i], end, 768 * i, desc[i]) == 0
    return torch.from_numpy(host).cuda(), end, desc0


@pytest.mark.parametrize("out", ["uint8", "float"])
def test_writes_stay_inside_dst(ops, out):
    h, w = 65, 19
    blobs, want = all_formats(h, w)
    n = len(blobs)
    buf, end, desc0 = staged(ops, blobs)
    guard, count = 4096, n * h * w * 3
    if out == "uint8":
        room = torch.full((count + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
        dst, fill = room[guard:guard + count].view(n, h, w, 3), 0xA5
    else:
        room = torch.full((count + 2 * guard,), -7.0, dtype=torch.float32, device="cuda")
        dst, fill = room[guard:guard + count].view(n, 3, h, w), -7.0
    status = ops.png_unfilter(buf, end, desc0, n, h, w, dst)
    assert status.cpu().tolist() == [0] * n
    assert bool((room[:guard] == fill).all()) and bool((room[guard + count:] == fill).all()), "the kernel wrote outside dst"
    ref = np.stack(want)
    if out == "uint8":
        assert np.array_equal(dst.cpu().numpy(), ref)
    else:
        assert torch.equal(dst.cpu(), torch.from_numpy(ref).permute(0, 3, 1, 2).float() / 255)


# ---- png_decode end to end --------------------------------------------------------------------------------------------------------------
def test_png_decode_mixes_paths_and_counts_the_fallbacks(ops):
    blobs, want = all_formats(40, 24)
    device_path(ops, blobs)                                 # what keeps the count below honest: the supported frames alone take 0 fallbacks
    rgb = PC.samples(40, 24, 2, 8, "photo")
    mixed = blobs[:5] + [PC.write_png(rgb, 2, 8, interlace=True)] + blobs[5:] + [PC.write_png(PC.samples(40, 24, 2, 16), 2, 16)]
    for out in ("uint8", "float"):
        info = {}
        got = ops.png_decode(mixed, out=out, info=info).cpu()
        assert info["fallback"] == [(5, "interlaced"), (len(mixed) - 1, "16-bit samples")] and len(info["fallback"]) == 2
        for i, blob in enumerate(mixed):
            ref = PC.pillow(blob)
            assert torch.equal(got[i], torch.from_numpy(ref) if out == "uint8" else as_float(ref)), (out, i)


def test_palette_index_beyond_plte_goes_to_pillow(ops):
    a = PC.samples(20, 24, 3, 8, "noise", entries=256)
    a[3, 5] = 200
    flagged = PC.write_png(a, 3, 8, "cycle", pal=PC.palette(12))
    fine, exp = PC.case(20, 24, 3, 8, "cycle", entries=12)
    info = {}
    got = ops.png_decode([fine, flagged, fine], info=info).cpu().numpy()
    assert info["fallback"] == [(1, "palette index")]
    assert np.array_equal(got[1], PC.pillow(flagged)) and np.array_equal(got[0], exp) and np.array_equal(got[2], exp)


# ---- the tools on trees Pillow wrote ------------------------------------------------------------------------------------------------------
def pillow_trees(root):
    """2 scenes x 3 frames of 32 x 32 under root/pred and root/gt, written by Pillow (filtered rows); returns {side: {scene: [pixels]}}"""
    made = {}
    for side in ("pred", "gt"):
        for s, scene in enumerate(("scene_a", "scene_b")):
            (root / side / scene / "color").mkdir(parents=True)
            for f in range(3):
                a = PC.samples(32, 32, 2, 8, "photo", key=(s, f))
                if side == "pred":                          # the ground truth, off by up to 4
                    a = np.clip(a.astype(np.int32) + (PC.samples(32, 32, 2, 8, "noise", key=("d", s, f)) % 9).astype(np.int32) - 4, 0, 255).astype(np.uint8)
                blob = PC.pillow_file(a, "RGB")
                (root / side / scene / "color" / f"{f:0>6}.png").write_bytes(blob)
                made.setdefault(side, {}).setdefault(scene, []).append(PC.pillow(blob))
    return made


def test_score_trees_on_pillow_written_trees(ops, tmp_path):
    from mv_ldm_amd import metrics as M
    from mv_ldm_amd.image_io import save_image
    made = pillow_trees(tmp_path)
    kinds = set()
    for p in sorted((tmp_path / "gt").rglob("*.png")):
        kinds |= PC.filter_types(p.read_bytes())
    assert kinds - {0}, "Pillow wrote filter 0 only: the case went soft"
    rep = M.score_trees(tmp_path / "pred", tmp_path / "gt")
    assert rep["overall"]["frames"] == 6 and rep["missing"] == []
    for scene in ("scene_a", "scene_b"):
        p = torch.stack([as_float(x) for x in made["pred"][scene]]).cuda()
        g = torch.stack([as_float(x) for x in made["gt"][scene]]).cuda()
        psnr, ssim = M.image_metrics(g, p)
        assert rep["scenes"][scene]["per_frame"] == {i: [a, b] for i, (a, b) in enumerate(zip(psnr.tolist(), ssim.tolist()))}
    for side in ("pred", "gt"):                             # the same trees as `save_image` writes them (filter 0 on every row): the same report
        for scene, frames in made[side].items():
            for f, x in enumerate(frames):
                save_image(as_float(x), tmp_path / "own" / side / scene / "color" / f"{f:0>6}.png")
    assert M.score_trees(tmp_path / "own" / "pred", tmp_path / "own" / "gt") == rep


def test_cleanfid_folder_reader_on_the_device(ops, tmp_path):
    from mv_ldm_amd import cleanfid
    made = pillow_trees(tmp_path)
    grey = PC.samples(20, 24, 0, 8, "photo")
    (tmp_path / "gt" / "z.png").write_bytes(PC.pillow_file(grey, "L"))
    batches = list(cleanfid.iter_batches(tmp_path / "gt", batch=4, device="cuda"))
    assert [tuple(b.shape) for b in batches] == [(4, 3, 32, 32), (2, 3, 32, 32), (1, 3, 20, 24)] and all(b.is_cuda and b.dtype == torch.uint8 for b in batches)
    want = torch.stack([torch.from_numpy(x.copy()).permute(2, 0, 1) for scene in ("scene_a", "scene_b") for x in made["gt"][scene]])
    assert torch.equal(torch.cat(batches[:2]).cpu(), want)
    assert torch.equal(batches[2][0].cpu(), torch.from_numpy(grey)[None].expand(3, -1, -1))
