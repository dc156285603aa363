"""GPU: the inflate kernel (csrc/inflate.hip) against `zlib.decompress` over the streams of tests/inflate_cases.py in one mixed batch with
guard bytes around every slot; kernel and host twin agreeing in bytes and status on the corruption set (one launch: every one of those
streams is refused by bounded, guarded code, none is meant to fault); `png_decode(inflate="device")` against Pillow and against
`inflate="host"`, fallbacks included; `cleanfid.score_folders` and `metrics.score_trees` giving the same numbers on either path.
The 1-byte and the empty payload: see tests/test_inflate_cpu.py."""
import zlib

import numpy as np
import pytest
import torch

import inflate_cases as IC
import png_cases as PC

pytestmark = pytest.mark.gpu
PIL = pytest.importorskip("PIL")


@pytest.fixture(scope="module")
def ops():
    from mv_ldm_amd import _build
    _build.build()
    from mv_ldm_amd import ops
    return ops


def kernel(ops, streams, infos, h, w, guard=64):
    """(status, output buffer, slot offsets, the packed host arrays) of one launch"""
    packed = IC.pack(streams, infos, guard)
    zbuf, zdesc, desc, soffs, send = packed
    out = torch.full((send,), 0xA5, dtype=torch.uint8, device="cuda")
    status = ops.png_inflate(torch.from_numpy(zbuf).cuda(), torch.from_numpy(zdesc).cuda(), out, torch.from_numpy(desc).cuda(), h, w)
    status, out = status.cpu().numpy(), out.cpu().numpy()
    assert IC.guards_intact(out, soffs, [n for _, _, n in infos], guard), "the kernel wrote outside a slot"
    return status, out, soffs, packed


def test_kernel_equals_zlib_on_every_case_in_one_mixed_batch(ops):
    from mv_ldm_amd import _lib as L
    group = [c for c in IC.cases() if (c.h, c.w) == (1, IC.W)]
    assert len(group) == 52 and {c.need for c in group} >= {1051, 2101, 4201, 8401, 33601}
    status, out, soffs, _ = kernel(ops, [c.z for c in group], [(c.ctype, c.depth, c.need) for c in group], 1, IC.W)
    for i, c in enumerate(group):
        assert status[i] == 0, (c.name, int(status[i]))
        assert out[soffs[i]:soffs[i] + c.need].tobytes() == zlib.decompress(c.z), c.name
    for c in (c for c in IC.cases() if (c.h, c.w) != (1, IC.W)):   # the two other geometries: 7 rows of stored blocks, a 2-byte frame
        status, out, soffs, _ = kernel(ops, [c.z], [(c.ctype, c.depth, c.need)], c.h, c.w)
        assert status[0] == 0 and out[soffs[0]:soffs[0] + c.need].tobytes() == zlib.decompress(c.z), c.name
    tiny = IC.tiny_cases()
    status, out, soffs, _ = kernel(ops, [z for _, z in tiny], [(0, 8, 2)] * len(tiny), 1, 1)
    assert status.tolist() == [L.PNG_LENGTH] * len(tiny)


def test_kernel_and_twin_agree_on_the_corruption_set(ops):
    rows = IC.corruptions()
    infos = [(3, 4, 4201)] * len(rows)
    status, out, soffs, (zbuf, zdesc, desc, _, send) = kernel(ops, [z for _, z, _, _ in rows], infos, 1, IC.W)
    host = np.full(send, 0xA5, dtype=np.uint8)
    twin = ops.png_inflate_host(zbuf, zdesc, host, desc, 1, IC.W)
    assert status.tolist() == twin.tolist()
    for i, (name, z, payload, allowed) in enumerate(rows):
        assert status[i] in allowed, (name, int(status[i]))
        if payload is not None:                             # after a refusal the slot is unspecified: bytes are compared where both accepted
            assert out[soffs[i]:soffs[i] + 4201].tobytes() == host[soffs[i]:soffs[i] + 4201].tobytes() == payload, name


def test_a_captured_call_replays(ops):
    c = next(c for c in IC.cases() if c.name == "handmade/overlap")
    zbuf, zdesc, desc, soffs, send = IC.pack([c.z], [(c.ctype, c.depth, c.need)])
    z, zd, d = torch.from_numpy(zbuf).cuda(), torch.from_numpy(zdesc).cuda(), torch.from_numpy(desc).cuda()
    out = torch.zeros(send, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ops.png_inflate(z, zd, out, d, c.h, c.w, status)        # warm: nothing is allocated inside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.png_inflate(z, zd, out, d, c.h, c.w, status)
    out.zero_()
    status.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert status.tolist() == [0] and out[soffs[0]:soffs[0] + c.need].cpu().numpy().tobytes() == c.payload


# ---- png_decode end to end ----------------------------------------------------------------------------------------------------------------
def both_paths(ops, blobs, out="uint8"):
    a, b = {}, {}
    dev = ops.png_decode(blobs, out=out, info=a, inflate="device").cpu()
    host = ops.png_decode(blobs, out=out, info=b).cpu()
    assert torch.equal(dev, host) and a["fallback"] == b["fallback"]
    return dev, a


def test_one_row_frames(ops):
    blobs, want = [], []
    for ctype, depth in PC.SUPPORTED:
        blob, exp = PC.case(1, 37, ctype, depth, 4)
        blobs.append(blob)
        want.append(exp)
    got, info = both_paths(ops, blobs)
    assert info["fallback"] == [] and np.array_equal(got.numpy(), np.stack(want))


def test_64_square_rgb_as_pillow_writes_it(ops):
    a = PC.samples(64, 64, 2, 8, "photo")
    blob = PC.pillow_file(a, "RGB")
    assert PC.filter_types(blob) - {0}, "Pillow wrote filter 0 only: the case went soft"
    for out in ("uint8", "float"):
        blobs = [blob, PC.write_png(a, 2, 8, "cycle", level=9), PC.write_png(a, 2, 8, 0, level=0)]
        got, info = both_paths(ops, blobs, out)
        assert info["fallback"] == [] and info["upload_bytes"] < ops._png_layout([ops.png_probe(b) for b in blobs])[3]      # the files, not the inflated streams
        ref = torch.from_numpy(a)
        for i in range(3):
            assert torch.equal(got[i], ref if out == "uint8" else ref.permute(2, 0, 1).float() / 255), (out, i)
    assert np.array_equal(PC.pillow(blob), a)


def test_batch_of_70_mixed_frames_with_every_fallback(ops):
    refused, names = IC.refusal_frames(32, 40)
    blobs, want, at = [], [], {}
    for i in range(70):
        if i % 9 == 4 and len(at) < len(refused):           # the frames Pillow has to read, spread through the batch
            at[i] = names[len(at)]
            blobs.append(refused[len(at) - 1])
            want.append(PC.pillow(blobs[-1]))
            continue
        ctype, depth = PC.SUPPORTED[i % len(PC.SUPPORTED)]
        blob, exp = PC.case(32, 40, ctype, depth, f"cycle+{i % 5}", content=("noise", "photo", "flat")[i % 3], key=i, level=(0, 1, 6, 9)[i % 4],
                            idat_split=(None, 1, 100)[i % 3])
        blobs.append(blob)
        want.append(exp)
    assert len(at) == len(refused) == 7
    got, info = both_paths(ops, blobs)
    assert info["fallback"] == sorted(at.items())
    assert np.array_equal(got.numpy(), np.stack(want))
    assert np.array_equal(got[::9].numpy(), np.stack([PC.pillow(b) for b in blobs[::9]]))


# ---- the tools ---------------------------------------------------------------------------------------------------------------------------
def pillow_trees(root):
    """2 scenes x 3 frames of 32 x 32 under root/pred and root/gt, written by Pillow (filtered rows)"""
    for side in ("pred", "gt"):
        for s, scene in enumerate(("scene_a", "scene_b")):
            (root / side / scene / "color").mkdir(parents=True)
            for f in range(3):
                a = PC.samples(32, 32, 2, 8, "photo", key=(s, f))
                if side == "pred":
                    a = np.clip(a.astype(np.int32) + (PC.samples(32, 32, 2, 8, "noise", key=("d", s, f)) % 9).astype(np.int32) - 4, 0, 255).astype(np.uint8)
                (root / side / scene / "color" / f"{f:0>6}.png").write_bytes(PC.pillow_file(a, "RGB"))


def test_score_trees_gives_the_same_report_on_either_path(ops, tmp_path):
    from mv_ldm_amd import metrics as M
    from mv_ldm_amd.image_io import load_images
    pillow_trees(tmp_path)
    host = M.score_trees(tmp_path / "pred", tmp_path / "gt")
    dev = M.score_trees(tmp_path / "pred", tmp_path / "gt", inflate="device")
    assert dev == host and dev["overall"]["frames"] == 6
    info = {}
    load_images(sorted((tmp_path / "gt").rglob("*.png")), "cuda", info=info, inflate="device")
    assert info["fallback"] == []


def test_score_folders_gives_the_same_numbers_on_either_path(ops, tmp_path):
    from mv_ldm_amd import cleanfid
    pillow_trees(tmp_path)
    host = list(cleanfid.iter_batches(tmp_path / "gt", batch=4, device="cuda"))
    dev = list(cleanfid.iter_batches(tmp_path / "gt", batch=4, device="cuda", inflate="device"))
    assert [tuple(b.shape) for b in dev] == [(4, 3, 32, 32), (2, 3, 32, 32)] and all(torch.equal(a, b) for a, b in zip(dev, host))

    class Counting:                                         # score_folders' reader, without an Inception network: what it feeds is what is compared
        keep_features, real_state, info = False, torch.zeros(1, device="cuda"), torch.zeros(8, device="cuda")

        def __init__(self):
            self.seen = []

        def reset(self):
            pass

        def update(self, imgs, real, dtype=None):
            self.seen.append((real, imgs.clone()))

        def compute(self):
            return torch.stack([x.double().mean() for _, x in self.seen]).sum()

    a, b = Counting(), Counting()
    ra = cleanfid.score_folders(tmp_path / "pred", tmp_path / "gt", a, batch=4)
    rb = cleanfid.score_folders(tmp_path / "pred", tmp_path / "gt", b, batch=4, inflate="device")
    assert ra == rb and ra["n1"] == ra["n2"] == 6
    assert len(a.seen) == len(b.seen) == 4 and all(x[0] == y[0] and torch.equal(x[1], y[1]) for x, y in zip(a.seen, b.seen))
