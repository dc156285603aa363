"""GPU: the Huffman scan decoded on the device (csrc/jpeg_huff.hip through `ops.jpeg_entropy_device`) against its host emulation and the
host's Huffman decoder, `torch.equal` everywhere, then `ops.jpeg_decode(entropy="device")` and the readers end to end against Pillow.
The frames are those of tests/test_jpeg_entropy_cpu.py, which pins the emulation (the kernels' own step function) to the host decoder
without a device: run this file after that one passes."""
import numpy as np
import pytest
import torch

import jpeg_cases as J
import re10k_fixture
import test_jpeg_entropy_cpu as E
import train_fixture as F

pytestmark = pytest.mark.gpu

CANARY = 0x5A


@pytest.fixture(scope="module")
def ops():
    from mv_ldm_amd import ops
    return ops


def _expect(blobs):
    return torch.from_numpy(np.stack([J.pillow(b) for b in blobs]))


def _pack(ops, blobs):
    """prepare a batch of one layout into one host buffer -> (scan, desc [n, 4], tables [n, TB], info)"""
    from mv_ldm_amd import _lib as L
    offs = [0]
    for b in blobs:
        offs.append(offs[-1] + ops.jpeg_scan_room(len(b)))
    scan = np.zeros(offs[-1], dtype=np.uint8)
    desc, tables = np.zeros((len(blobs), 4), dtype=np.int32), np.zeros((len(blobs), L.JPEG_TABLE_BYTES), dtype=np.uint8)
    infos = []
    for j, b in enumerate(blobs):
        p = ops.jpeg_scan_prepare(b, scan, offs[j], desc[j], tables[j])
        assert p.reason == 0
        infos.append(p.info)
    assert len({(i.h, i.w, i.sampling) for i in infos}) == 1
    return scan, desc, tables, infos[0]


def _device(ops, scan, desc, tables, info, subseq_bits=0):
    """`jpeg_entropy_device` with canaries around coef, qt and status -> host tensors"""
    n, count, pad = desc.shape[0], ops.jpeg_coef_count(info.h, info.w, info.sampling), 64
    bufs = [torch.full((n * k * size + 2 * pad,), CANARY, dtype=torch.uint8, device="cuda") for k, size in ((count, 2), (192, 2), (4, 4))]
    views = [b[pad:b.numel() - pad].view(dt).view(n, k) for b, dt, k in zip(bufs, (torch.int16, torch.int16, torch.int32), (count, 192, 4))]
    ops.jpeg_entropy_device(torch.from_numpy(scan).cuda(), torch.from_numpy(desc).cuda(), torch.from_numpy(tables).cuda(), info.h, info.w, info.sampling,
                            *views, subseq_bits=subseq_bits)
    torch.cuda.synchronize()
    for b in bufs:
        assert (b[:pad] == CANARY).all() and (b[-pad:] == CANARY).all(), "a write outside coef, qt or status"
    return [v.cpu() for v in views]


def _check(ops, blobs, name, bits=(32, 0), acceptance_only=False):
    scan, desc, tables, info = _pack(ops, blobs)
    for sb in bits:
        coef, qt, status = _device(ops, scan, desc, tables, info, sb)
        ecoef, eqt, estatus = ops.jpeg_entropy_emul(scan, desc, tables, info.h, info.w, info.sampling, subseq_bits=sb)
        if acceptance_only:
            assert torch.equal(status[:, 0] == 0, torch.from_numpy(estatus[:, 0] == 0)), (name, sb, status, estatus)
            for j, b in enumerate(blobs):
                assert (E.host(ops, b)[0] == 0) == (int(status[j, 0]) == 0), (name, sb, j)
            continue
        assert torch.equal(status, torch.from_numpy(estatus)), (name, sb, status, estatus)
        assert torch.equal(coef, torch.from_numpy(ecoef)) and torch.equal(qt, torch.from_numpy(eqt.view(np.int16))), (name, sb)
        for j, b in enumerate(blobs):
            reason, max_s, hcoef, hqt, _ = E.host(ops, b)
            assert (int(status[j, 0]), int(status[j, 1])) == (reason, max_s), (name, sb, j)
            assert torch.equal(coef[j], torch.from_numpy(hcoef)) and torch.equal(qt[j], torch.from_numpy(hqt.view(np.int16))), (name, sb, j)


@pytest.mark.parametrize("h,w", J.SIZES, ids=lambda v: str(v))
def test_device_against_emulation_and_host(ops, h, w):
    """every small case at 32-bit subsequences and the default; 45 x 81 holds the multi-chunk frame, 1 x 1 the single subsequence"""
    for name, blob in J.small_cases(h, w):
        _check(ops, [blob], name)


def test_gray_and_optimized(ops):
    _check(ops, [J.gray_case()], "gray")
    _check(ops, [J.encode(J.pixels(45, 81, "photo"), quality=90, subsampling=2, optimize=True)], "optimize")


def test_batch_of_three(ops):
    """three scan lengths and three sets of optimised tables in one call"""
    blobs = [J.encode(J.pixels(45, 81, c), quality=q, subsampling=2, optimize=True) for c, q in (("noise", 100), ("smooth", 50), ("photo", 90))]
    assert len({len(b) for b in blobs}) == 3
    _check(ops, blobs, "three")


def test_range_guard(ops):
    from mv_ldm_amd import _lib as L
    blob = J.with_dqt(J.encode(J.pixels(45, 81, "noise"), quality=50, subsampling=2), 255)
    assert E.host(ops, blob)[0] == L.JPEG_RANGE
    _check(ops, [blob], "range")


def test_damaged_streams(ops):
    """the 16 seeded flipped-byte streams of the CPU file (both outcomes occur: checked here again, on the CPU): acceptance parity with
    the host decoder and the emulation, and nothing written outside the three outputs"""
    streams = [b for b in E.damaged_sixteen() if ops.jpeg_scan_prepare(b).reason == 0]
    outcomes = {E.host(ops, b)[0] == 0 for b in E.damaged_sixteen()}
    assert outcomes == {True, False} and len(streams) >= 8
    _check(ops, streams, f"seed {E.DAMAGE_SEED}", acceptance_only=True)


def test_arguments(ops):
    scan, desc, tables, info = _pack(ops, [J.encode(J.pixels(8, 8, "noise"), quality=90)])
    dev = [torch.from_numpy(a).cuda() for a in (scan, desc, tables)]
    for bad in (16, 48, 1 << 17):
        with pytest.raises(RuntimeError):
            ops.jpeg_entropy_device(*dev, info.h, info.w, info.sampling, subseq_bits=bad)
    with pytest.raises(RuntimeError):
        ops.jpeg_entropy_device(torch.zeros(scan.size + 16, dtype=torch.uint8, device="cuda")[4:4 + scan.size], dev[1], dev[2], info.h, info.w, info.sampling)
    # a descriptor that does not fit the scan buffer: refused, nothing read
    wild = torch.tensor([[0, 8 * scan.size, 0, 0]], dtype=torch.int32, device="cuda")
    status = ops.jpeg_entropy_device(dev[0], wild, dev[2], info.h, info.w, info.sampling)[2]
    assert status.cpu().tolist() == [[3, 0, 0, 0]]


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _counted(ops, monkeypatch):
    calls = {"status": 0, "entropy": [], "decode": []}
    real_s, real_e, real_d = ops.jpeg_status_download, ops.jpeg_entropy_device, ops.jpeg_decode_coefs
    monkeypatch.setattr(ops, "jpeg_status_download", lambda s: (calls.__setitem__("status", calls["status"] + 1), real_s(s))[1])
    monkeypatch.setattr(ops, "jpeg_entropy_device", lambda *a, **k: (calls["entropy"].append((a[5], a[1].shape[0])), real_e(*a, **k))[1])
    monkeypatch.setattr(ops, "jpeg_decode_coefs", lambda *a, **k: (calls["decode"].append((a[4], a[0].shape[0])), real_d(*a, **k))[1])
    return calls


@pytest.mark.parametrize("h,w", J.SIZES, ids=lambda v: str(v))
def test_decode_small_cases(ops, h, w, monkeypatch):
    from mv_ldm_amd import dataset as D
    fell = []
    real = D.decode_image
    monkeypatch.setattr(D, "decode_image", lambda b: (fell.append(1), real(b))[1])
    for name, blob in J.small_cases(h, w):
        assert torch.equal(ops.jpeg_decode([blob], entropy="device").cpu(), _expect([blob])), name
    assert not fell, "a frame took the Pillow path"


def test_decode_mixed_layouts(ops, monkeypatch):
    """4:2:0, 4:4:4, grayscale and 4:2:2 interleaved: per layout one entropy call, one decode call and one status download"""
    kinds = [2, 0, None, 2, 1, 0, None]
    blobs = [J.encode(J.pixels(24, 40, "noise", channels=1), quality=90) if s is None else J.encode(J.pixels(24, 40, "photo" if i % 2 else "noise"), quality=90, subsampling=s)
             for i, s in enumerate(kinds)]
    calls = _counted(ops, monkeypatch)
    out = ops.jpeg_decode(blobs, entropy="device")
    assert sorted(calls["entropy"]) == sorted(calls["decode"]) == [(0, 2), (1, 2), (2, 1), (3, 2)] and calls["status"] == 4
    assert torch.equal(out.cpu(), _expect(blobs))
    assert torch.equal(out, ops.jpeg_decode(blobs))
    with pytest.raises(ValueError):
        ops.jpeg_decode([blobs[0], J.encode(J.pixels(24, 48, "noise"), quality=90)], entropy="device")
    with pytest.raises(ValueError):
        ops.jpeg_decode(blobs, entropy="pillow")


def test_decode_fallbacks_inside_a_batch(ops, monkeypatch):
    """a restart frame (host entropy pass, same device call, not Pillow), a progressive frame, a PNG and a frame outside the guard"""
    from mv_ldm_amd import dataset as D
    from mv_ldm_amd.image_io import encode_png
    base = J.encode(J.pixels(45, 81, "noise"), quality=50, subsampling=2)
    wide = J.with_dqt(base, 255)
    progressive = J.encode(J.pixels(45, 81, "photo"), quality=90, progressive=True)
    png = encode_png(J.pixels(45, 81, "smooth"))
    blobs = [base, wide, J.restart_case(), progressive, png, J.encode(J.pixels(45, 81, "smooth"), quality=90, subsampling=2)]
    fell = []
    real = D.decode_image
    monkeypatch.setattr(D, "decode_image", lambda b: (fell.append(blobs.index(b)), real(b))[1])
    calls = _counted(ops, monkeypatch)
    out = ops.jpeg_decode(blobs, entropy="device")
    assert sorted(fell) == [1, 3, 4] and calls["status"] == 1 and calls["entropy"] == calls["decode"] == [(3, 4)]
    want = torch.from_numpy(np.stack([J.pillow(b) for b in blobs[:4]] + [J.pixels(45, 81, "smooth"), J.pillow(blobs[5])]))
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("entropy", ["host", "device"])
def test_decode_every_frame_refused(ops, entropy, monkeypatch):
    """two PNGs and a progressive frame: no layout, so nothing is launched or read back; all three come from `decode_image`"""
    from mv_ldm_amd import dataset as D
    from mv_ldm_amd.image_io import encode_png
    blobs = [encode_png(J.pixels(45, 81, "smooth")), encode_png(J.pixels(45, 81, "noise")), J.encode(J.pixels(45, 81, "photo"), quality=90, progressive=True)]
    fell = []
    real = D.decode_image
    monkeypatch.setattr(D, "decode_image", lambda b: (fell.append(blobs.index(b)), real(b))[1])
    calls = _counted(ops, monkeypatch)
    out = ops.jpeg_decode(blobs, entropy=entropy)
    assert sorted(fell) == [0, 1, 2] and calls == {"status": 0, "entropy": [], "decode": []}
    want = torch.from_numpy(np.stack([J.pixels(45, 81, "smooth"), J.pixels(45, 81, "noise"), J.pillow(blobs[2])]))
    assert out.is_cuda and torch.equal(out.cpu(), want)


@pytest.mark.parametrize("entropy", ["host", "device"])
def test_decode_layout_of_restart_frames(ops, entropy, monkeypatch):
    """a layout made only of restart frames: the host's entropy pass for both, one decode call, never Pillow; with device entropy the
    layout still makes its one (empty) entropy call and its one status download"""
    from mv_ldm_amd import dataset as D
    blobs = [J.restart_case(), J.restart_case()]
    info = ops.jpeg_probe(blobs[0])
    assert info.supported and (info.h, info.w) == (45, 81)
    fell = []
    real = D.decode_image
    monkeypatch.setattr(D, "decode_image", lambda b: (fell.append(1), real(b))[1])
    calls = _counted(ops, monkeypatch)
    out = ops.jpeg_decode(blobs, entropy=entropy)
    assert not fell and calls["decode"] == [(info.sampling, 2)]
    assert (calls["entropy"], calls["status"]) == (([(info.sampling, 2)], 1) if entropy == "device" else ([], 0))
    assert torch.equal(out.cpu(), _expect(blobs))


def test_decode_big_case(ops, monkeypatch):
    blob = J.big_case()
    calls = _counted(ops, monkeypatch)
    out = ops.jpeg_decode([blob, blob], entropy="device")
    assert calls["status"] == 1 and torch.equal(out[0], out[1]) and torch.equal(out[0].cpu(), _expect([blob])[0])


def test_graph_capture(ops):
    """`jpeg_entropy_device` + `jpeg_decode_coefs` on caller-given buffers, captured; the replay decodes new scan bytes"""
    first = [J.encode(J.pixels(45, 81, c), quality=90, subsampling=2) for c in ("noise", "photo")]
    other = [J.encode(J.pixels(45, 81, c), quality=50, subsampling=2, optimize=True) for c in ("smooth", "noise")]
    room = max(sum(ops.jpeg_scan_room(len(b)) for b in bs) for bs in (first, other))
    packed = []
    for bs in (first, other):
        scan, desc, tables, info = _pack(ops, bs)
        packed.append((np.concatenate([scan, np.zeros(room - scan.size, dtype=np.uint8)]), desc, tables))
    h, w, sampling = info.h, info.w, info.sampling
    scan, desc, tables = (torch.from_numpy(a).cuda() for a in packed[0])
    count = ops.jpeg_coef_count(h, w, sampling)
    coef, qt = torch.empty(2, count, dtype=torch.int16, device="cuda"), torch.empty(2, 192, dtype=torch.int16, device="cuda")
    status = torch.empty(2, 4, dtype=torch.int32, device="cuda")
    dst = torch.zeros(2, h, w, 3, dtype=torch.uint8, device="cuda")
    ws = torch.empty(ops.jpeg_workspace_bytes(2, h, w, sampling), dtype=torch.uint8, device="cuda")

    def run():
        ops.jpeg_entropy_device(scan, desc, tables, h, w, sampling, coef, qt, status)
        ops.jpeg_decode_coefs(coef, qt, h, w, sampling, dst, ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
        eager = dst.clone()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for t, a in zip((scan, desc, tables), packed[1]):
        t.copy_(torch.from_numpy(a))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager.cpu(), _expect(first)) and torch.equal(dst.cpu(), _expect(other))
    assert status.cpu()[:, 0].tolist() == [0, 0]


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k])
        elif isinstance(a[k], torch.Tensor):
            assert a[k].device == b[k].device and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_scene_reader_device_entropy(ops, tmp_path, monkeypatch):
    from mv_ldm_amd import dataset as D
    index = re10k_fixture.build(tmp_path / "re10k", jpeg_scenes=("a_one", "c_two"))
    host = list(D.RE10KScenes(tmp_path / "re10k", index=index, image_shape=(32, 32)))
    calls = _counted(ops, monkeypatch)
    device = list(D.RE10KScenes(tmp_path / "re10k", index=index, image_shape=(32, 32), device_entropy=True))
    assert calls["status"] >= 1 and len(host) == len(device) >= 4
    for a, b in zip(host, device):
        _same(a, b)


@pytest.mark.parametrize("workers", [0, 3])
def test_train_loader_device_entropy(ops, tmp_path, workers, monkeypatch):
    """the batches of `device_entropy=True` are those of `False` under one seed, the draws too, and no frame goes through Pillow"""
    from mv_ldm_amd import dataset as D
    root = F.build(tmp_path / "train", jpeg=True)
    kw = dict(view_sampler=D.get_view_sampler("bounded", **F.SAMPLER), image_shape=F.SHAPE, batch_size=2, augment=True, drop_last=False)
    torch.manual_seed(7)
    host = list(D.RE10KTrainLoader(root, decode_workers=workers, **kw))
    after_host = torch.rand(())
    fell = []
    real = D.decode_image
    monkeypatch.setattr(D, "decode_image", lambda b: (fell.append(1), real(b))[1])
    calls = _counted(ops, monkeypatch)
    torch.manual_seed(7)
    device = list(D.RE10KTrainLoader(root, decode_workers=workers, device_entropy=True, **kw))
    assert torch.equal(after_host, torch.rand(())) and not fell and calls["status"] >= 1
    assert len(host) == len(device) >= 2
    for a, b in zip(host, device):
        _same(a, b)
