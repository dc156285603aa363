"""GPU: `ops.jpeg_decode` (csrc/jpeg_host.cpp's entropy decoder, csrc/jpeg.hip's two kernels) against Pillow's own decode of the same
bytes, `torch.equal` everywhere; the frames are those of tests/test_jpeg_cpu.py (tests/jpeg_cases.py), which pins the host restatement of
the same arithmetic to Pillow without a device.  Then the readers end to end: `device_decode=True` gives the batches of `False`."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import jpeg_cases as J
import re10k_fixture
import train_fixture as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from mv_ldm_amd import ops
    return ops


def _expect(blobs):
    return torch.from_numpy(np.stack([J.pillow(b) for b in blobs]))


def _coefs(ops, blobs, sampling):
    """the host half by hand: int16 [n, count] and [n, 192] on the device; every frame must be inside the guard"""
    info = ops.jpeg_probe(blobs[0])
    assert info.sampling == sampling
    count = ops.jpeg_coef_count(info.h, info.w, sampling)
    coef, qt = np.zeros((len(blobs), count), dtype=np.int16), np.zeros((len(blobs), 192), dtype=np.int16)
    for i, b in enumerate(blobs):
        assert ops.jpeg_entropy(b, coef[i], qt[i])[0] == 0
    return torch.from_numpy(coef).cuda(), torch.from_numpy(qt).cuda(), info.h, info.w


@pytest.mark.parametrize("h,w", J.SIZES, ids=lambda v: str(v))
def test_small_cases(ops, h, w):
    for name, blob in J.small_cases(h, w):
        coef = np.zeros(ops.jpeg_coef_count(h, w, 3 if "-s2-" in name else 2 if "-s1-" in name else 1), dtype=np.int16)
        assert ops.jpeg_entropy(blob, coef, np.zeros(192, dtype=np.uint16))[0] == 0, f"{name}: not decoded by the library"
        assert torch.equal(ops.jpeg_decode([blob]).cpu(), _expect([blob])), name


def test_grayscale_and_restart_markers(ops):
    for blob in (J.gray_case(), J.restart_case()):
        assert ops.jpeg_probe(blob).supported
        assert torch.equal(ops.jpeg_decode([blob]).cpu(), _expect([blob]))


def test_three_frames_one_call(ops, monkeypatch):
    blobs = [J.encode(J.pixels(45, 81, c), quality=q, subsampling=2) for c, q in (("noise", 90), ("smooth", 50), ("photo", 100))]
    calls = []
    real = ops.jpeg_decode_coefs
    monkeypatch.setattr(ops, "jpeg_decode_coefs", lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])
    out = ops.jpeg_decode(blobs)
    assert calls == [3] and out.shape == (3, 45, 81, 3) and out.dtype == torch.uint8 and out.is_cuda
    assert torch.equal(out.cpu(), _expect(blobs))


def test_mixed_layouts_one_batch(ops, monkeypatch):
    """4:2:0, 4:4:4, grayscale and 4:2:2 frames interleaved: one device call per layout, every frame in its own slot"""
    kinds = [2, 0, None, 2, 1, 0, None]
    blobs = [J.encode(J.pixels(24, 40, "noise", channels=1), quality=90) if s is None else J.encode(J.pixels(24, 40, "photo" if i % 2 else "noise"), quality=90, subsampling=s)
             for i, s in enumerate(kinds)]
    calls = []
    real = ops.jpeg_decode_coefs
    monkeypatch.setattr(ops, "jpeg_decode_coefs", lambda *a, **k: (calls.append((a[4], a[0].shape[0])), real(*a, **k))[1])
    out = ops.jpeg_decode(blobs)
    assert sorted(calls) == [(0, 2), (1, 2), (2, 1), (3, 2)]
    assert torch.equal(out.cpu(), _expect(blobs))
    with pytest.raises(ValueError):
        ops.jpeg_decode([blobs[0], J.encode(J.pixels(24, 48, "noise"), quality=90)])


def test_fallback_frames_inside_a_batch(ops, monkeypatch):
    """a frame outside the range guard, a progressive one and a PNG among decodable ones: they take the Pillow path into their slots"""
    from mv_ldm_amd.image_io import encode_png
    base = J.encode(J.pixels(45, 81, "noise"), quality=50, subsampling=2)
    wide = J.with_dqt(base, 255)
    progressive = J.encode(J.pixels(45, 81, "photo"), quality=90, progressive=True)
    png = encode_png(J.pixels(45, 81, "smooth"))
    blobs = [base, wide, J.encode(J.pixels(45, 81, "smooth"), quality=90, subsampling=2), progressive, png]
    assert ops.jpeg_probe(wide).supported and not ops.jpeg_probe(progressive).supported
    from mv_ldm_amd import dataset as D
    fell = []
    real = D.decode_image
    monkeypatch.setattr(D, "decode_image", lambda b: (fell.append(blobs.index(b)), real(b))[1])
    out = ops.jpeg_decode(blobs)
    assert sorted(fell) == [1, 3, 4]
    want = torch.from_numpy(np.stack([J.pillow(b) for b in blobs[:4]] + [J.pixels(45, 81, "smooth")]))
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("misalign", [0, 4])
def test_confined_writes(ops, misalign):
    """dst and workspace sit inside larger tensors filled with a canary; `misalign` = 4 takes the kernels' dword path (pointers that are
    4- but not 16-byte aligned)"""
    from mv_ldm_amd import _lib as L
    blobs = [J.encode(J.pixels(17, 33, c), quality=90, subsampling=2) for c in ("noise", "photo", "smooth")]
    coef, qt, h, w = _coefs(ops, blobs, 3)
    n = len(blobs)
    pad = 256
    need = ops.jpeg_workspace_bytes(n, h, w, 3)
    nbytes = n * h * w * 3
    dst = torch.full((pad + misalign + (nbytes + 3) // 4 * 4 + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = torch.full((pad + misalign + need + pad,), 0x5A, dtype=torch.uint8, device="cuda")
    cbuf = torch.zeros(coef.numel() + 8, dtype=torch.int16, device="cuda")
    cin = cbuf[misalign // 2:misalign // 2 + coef.numel()]
    cin.copy_(coef.reshape(-1))
    at = pad + misalign
    L.check(L.load().mvldm_jpeg_decode(cin.data_ptr(), qt.data_ptr(), dst[at:].data_ptr(), n, h, w, 3, ws[at:].data_ptr(), need, ops.stream()))
    dst, ws = dst.cpu(), ws.cpu()
    assert (dst[:at] == 0xA5).all() and (dst[at + nbytes:] == 0xA5).all()
    assert (ws[:at] == 0x5A).all() and (ws[at + need:] == 0x5A).all()
    assert torch.equal(dst[at:at + nbytes].reshape(n, h, w, 3), _expect(blobs))


def test_golden_frame(ops):
    gold = json.loads((Path(__file__).parent / "golden" / "jpeg.json").read_text())
    blob = J.big_case()
    assert J.sha256(blob) == gold["stream_sha256"], "this Pillow encodes the frame differently: regenerate tests/golden/jpeg.json"
    out = ops.jpeg_decode([blob, blob])
    assert J.sha256(out[0].cpu().numpy()) == gold["decoded_sha256"] and torch.equal(out[0], out[1])


def test_graph_capture(ops):
    blobs = [J.encode(J.pixels(45, 81, c), quality=90, subsampling=2) for c in ("noise", "photo")]
    other = [J.encode(J.pixels(45, 81, c), quality=50, subsampling=2) for c in ("smooth", "noise")]
    coef, qt, h, w = _coefs(ops, blobs, 3)
    dst = torch.zeros(2, h, w, 3, dtype=torch.uint8, device="cuda")
    ws = torch.empty(ops.jpeg_workspace_bytes(2, h, w, 3), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = ops.jpeg_decode_coefs(coef, qt, h, w, 3, dst, ws).clone()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.jpeg_decode_coefs(coef, qt, h, w, 3, dst, ws)
    coef2, qt2, _, _ = _coefs(ops, other, 3)
    coef.copy_(coef2)
    qt.copy_(qt2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager.cpu(), _expect(blobs)) and torch.equal(dst.cpu(), _expect(other))


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k])
        elif isinstance(a[k], torch.Tensor):
            assert a[k].device == b[k].device and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_scene_reader_device_decode(ops, tmp_path):
    """`RE10KScenes` over a tree that mixes JPEG and PNG scenes: the same examples either way"""
    from mv_ldm_amd import dataset as D
    index = re10k_fixture.build(tmp_path / "re10k", jpeg_scenes=("a_one", "c_two"))
    host = list(D.RE10KScenes(tmp_path / "re10k", index=index, image_shape=(32, 32)))
    device = list(D.RE10KScenes(tmp_path / "re10k", index=index, image_shape=(32, 32), device_decode=True))
    assert len(host) == len(device) >= 4
    for a, b in zip(host, device):
        _same(a, b)


@pytest.mark.parametrize("workers", [0, 3])
def test_train_loader_device_decode(ops, tmp_path, workers, monkeypatch):
    """`RE10KTrainLoader` over the JPEG tree under one seed: the batches of `device_decode=True` are those of `False`, the draws too, and
    no frame is decoded by Pillow on the way"""
    from mv_ldm_amd import dataset as D
    root = F.build(tmp_path / "train", jpeg=True)
    kw = dict(view_sampler=D.get_view_sampler("bounded", **F.SAMPLER), image_shape=F.SHAPE, batch_size=2, augment=True, drop_last=False)
    torch.manual_seed(7)
    host = list(D.RE10KTrainLoader(root, decode_workers=workers, **kw))
    after_host = torch.rand(())
    fell = []
    real = D.decode_image
    monkeypatch.setattr(D, "decode_image", lambda b: (fell.append(1), real(b))[1])
    torch.manual_seed(7)
    device = list(D.RE10KTrainLoader(root, decode_workers=workers, device_decode=True, **kw))
    assert torch.equal(after_host, torch.rand(())) and not fell
    assert len(host) == len(device) >= 2
    for a, b in zip(host, device):
        _same(a, b)
