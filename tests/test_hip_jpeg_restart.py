"""GPU: the Huffman scan of frames with restart intervals decoded on the device (csrc/jpeg_huff.hip through `ops.jpeg_rst_entropy_device`)
against its host emulation and the host's Huffman decoder, `torch.equal` everywhere, then `ops.jpeg_decode(entropy="device",
restarts="device")` and a reader end to end against Pillow.  The frames are those of tests/test_jpeg_restart_cpu.py, which pins the
emulation (the kernels' own inline functions) to the host decoder without a device: run this file after that one passes."""
import numpy as np
import pytest
import torch

import jpeg_cases as J
import jpeg_restart_cases as R
import re10k_fixture

pytestmark = pytest.mark.gpu

CANARY = 0x5A


@pytest.fixture(scope="module")
def ops():
    from mv_ldm_amd import ops
    return ops


def _expect(blobs):
    return torch.from_numpy(np.stack([J.pillow(b) for b in blobs]))


def _host(ops, blob):
    info = ops.jpeg_probe(blob)
    coef, qt = np.zeros(ops.jpeg_coef_count(info.h, info.w, info.sampling), dtype=np.int16), np.zeros(192, dtype=np.uint16)
    reason, max_s = ops.jpeg_entropy(blob, coef, qt)
    return reason, max_s, coef, qt


def _pack(ops, blobs, room=None):
    """prepare a batch of one layout into one host buffer -> (scan, desc [n, 4], tables [n, TB], info)"""
    from mv_ldm_amd import _lib as L
    offs = [0]
    for b in blobs:
        offs.append(offs[-1] + ops.jpeg_rst_need(b))
    scan = np.zeros(max(offs[-1], room or 0), dtype=np.uint8)
    desc, tables = np.zeros((len(blobs), 4), dtype=np.int32), np.zeros((len(blobs), L.JPEG_TABLE_BYTES), dtype=np.uint8)
    infos = []
    for j, b in enumerate(blobs):
        p = ops.jpeg_rst_prepare(b, scan[:offs[j + 1]], offs[j], desc[j], tables[j])
        assert p.reason == 0
        infos.append(p.info)
    assert len({(i.h, i.w, i.sampling) for i in infos}) == 1
    return scan, desc, tables, infos[0]


def _device(ops, scan, desc, tables, info, subseq_bits=0, entry=None):
    """`jpeg_rst_entropy_device` (or `entry`) with canaries around coef, qt and status -> host tensors"""
    n, count, pad = desc.shape[0], ops.jpeg_coef_count(info.h, info.w, info.sampling), 64
    bufs = [torch.full((n * k * size + 2 * pad,), CANARY, dtype=torch.uint8, device="cuda") for k, size in ((count, 2), (192, 2), (4, 4))]
    views = [b[pad:b.numel() - pad].view(dt).view(n, k) for b, dt, k in zip(bufs, (torch.int16, torch.int16, torch.int32), (count, 192, 4))]
    (entry or ops.jpeg_rst_entropy_device)(torch.from_numpy(scan).cuda(), torch.from_numpy(desc).cuda(), torch.from_numpy(tables).cuda(), info.h, info.w,
                                           info.sampling, *views, subseq_bits=subseq_bits)
    torch.cuda.synchronize()
    for b in bufs:
        assert (b[:pad] == CANARY).all() and (b[-pad:] == CANARY).all(), "a write outside coef, qt or status"
    return [v.cpu() for v in views]


def _check(ops, blobs, name, bits=(32, 0), acceptance_only=False):
    scan, desc, tables, info = _pack(ops, blobs)
    for sb in bits:
        coef, qt, status = _device(ops, scan, desc, tables, info, sb)
        ecoef, eqt, estatus = ops.jpeg_rst_entropy_emul(scan, desc, tables, info.h, info.w, info.sampling, subseq_bits=sb)
        if acceptance_only:
            assert torch.equal(status[:, 0] == 0, torch.from_numpy(estatus[:, 0] == 0)), (name, sb, status, estatus)
            for j, b in enumerate(blobs):
                assert (_host(ops, b)[0] == 0) == (int(status[j, 0]) == 0), (name, sb, j)
            continue
        assert torch.equal(status, torch.from_numpy(estatus)), (name, sb, status, estatus)
        assert torch.equal(coef, torch.from_numpy(ecoef)) and torch.equal(qt, torch.from_numpy(eqt.view(np.int16))), (name, sb)
        for j, b in enumerate(blobs):
            reason, max_s, hcoef, hqt = _host(ops, b)
            assert (int(status[j, 0]), int(status[j, 1])) == (reason, max_s), (name, sb, j)
            assert torch.equal(coef[j], torch.from_numpy(hcoef)) and torch.equal(qt[j], torch.from_numpy(hqt.view(np.int16))), (name, sb, j)


FRAMES = {name: (blob, n) for name, blob, n in R.frames()}


@pytest.mark.parametrize("name", list(FRAMES))
def test_device_against_emulation_and_host(ops, name):
    """at 32-bit subsequences and the default: batches that end between intervals, intervals of more than five chunks, one interval"""
    _check(ops, [FRAMES[name][0]], name)


def test_three_frames_three_intervals(ops):
    """one call, one layout: Ri = 1, Ri = 7 and no DRI"""
    noise, photo = J.pixels(45, 81, "noise"), J.pixels(45, 81, "photo")
    blobs = [J.encode(noise, quality=100, subsampling=2, restart_marker_blocks=1), J.encode(photo, quality=90, subsampling=2, restart_marker_blocks=7),
             J.encode(noise, quality=50, subsampling=2, optimize=True)]
    assert [R.dri(b) for b in blobs] == [1, 7, 0]
    _check(ops, blobs, "three")


def test_both_paths_on_a_frame_without_dri(ops):
    """`R.seam_case()` through `jpeg_entropy_device` and `jpeg_rst_entropy_device`, which share their passes: the same coefficients,
    tables, reason, S and rounds, the host decoder's values, and each path's emulation on all four status words.  1089 blocks a
    component: both DC passes carry into a second pass of 1024; at 32 bits the scan takes several chunks"""
    blob = R.seam_case()
    reason, max_s, hcoef, hqt = _host(ops, blob)
    assert R.dri(blob) == 0 and reason == 0
    scan, desc, tables, info = _pack(ops, [blob])
    plain = ops.jpeg_scan_prepare(blob)
    assert plain.reason == 0 and info.mcu_cols * info.mcu_rows == 1089
    pscan, pdesc, ptables = plain.scan, plain.desc.reshape(1, 4), plain.tables.reshape(1, -1)
    for sb in (32, 0):
        got = {"restart": _device(ops, scan, desc, tables, info, sb), "plain": _device(ops, pscan, pdesc, ptables, info, sb, entry=ops.jpeg_entropy_device)}
        emul = {"restart": ops.jpeg_rst_entropy_emul(scan, desc, tables, info.h, info.w, info.sampling, subseq_bits=sb),
                "plain": ops.jpeg_entropy_emul(pscan, pdesc, ptables, info.h, info.w, info.sampling, subseq_bits=sb)}
        (pc, pq, ps), (rc, rq, rs) = got["plain"], got["restart"]
        assert torch.equal(pc, rc) and torch.equal(pq, rq) and torch.equal(ps[:, :3], rs[:, :3]), (sb, ps, rs)
        for path, (coef, qt, status) in got.items():
            assert (int(status[0, 0]), int(status[0, 1])) == (reason, max_s), (path, sb, status)
            assert torch.equal(coef[0], torch.from_numpy(hcoef)) and torch.equal(qt[0], torch.from_numpy(hqt.view(np.int16))), (path, sb)
            assert torch.equal(status, torch.from_numpy(emul[path][2])), (path, sb, status, emul[path][2])
            assert torch.equal(coef, torch.from_numpy(emul[path][0])) and torch.equal(qt, torch.from_numpy(emul[path][1].view(np.int16))), (path, sb)
        assert got["plain"][2][0, 3] == 0 and got["restart"][2][0, 3] == 1


def test_range_guard(ops):
    from mv_ldm_amd import _lib as L
    blob = J.with_dqt(J.encode(J.pixels(45, 81, "noise"), quality=50, subsampling=2, restart_marker_blocks=2), 255)
    assert _host(ops, blob)[0] == L.JPEG_RANGE
    _check(ops, [blob], "range")


def test_damaged_streams(ops):
    """the 16 seeded flipped-byte streams of the CPU file: acceptance parity with the host decoder and the emulation, and nothing written
    outside the three outputs"""
    flips = R.flipped_sixteen()
    streams = [b for b in flips if ops.jpeg_rst_prepare(b).reason == 0]
    assert {_host(ops, b)[0] == 0 for b in flips} == {True, False} and len(streams) >= 8
    _check(ops, streams, f"seed {R.DAMAGE_SEED}", acceptance_only=True)


def test_arguments(ops):
    blob = J.restart_case()
    scan, desc, tables, info = _pack(ops, [blob])
    dev = [torch.from_numpy(a).cuda() for a in (scan, desc, tables)]
    for bad in (16, 48, 1 << 17):
        with pytest.raises(RuntimeError):
            ops.jpeg_rst_entropy_device(*dev, info.h, info.w, info.sampling, subseq_bits=bad)
    with pytest.raises(RuntimeError):
        ops.jpeg_rst_entropy_device(torch.zeros(scan.size + 16, dtype=torch.uint8, device="cuda")[4:4 + scan.size], dev[1], dev[2], info.h, info.w, info.sampling)
    # a descriptor that does not fit the scan buffer, and a table entry that points outside the region: refused, nothing of the scan read
    n, occupied, ri = (int(v) for v in desc[0, 1:])
    wild = torch.tensor([[0, n, scan.size + 16, ri]], dtype=torch.int32, device="cuda")
    assert ops.jpeg_rst_entropy_device(dev[0], wild, dev[2], info.h, info.w, info.sampling)[2].cpu().tolist() == [[3, 0, 0, 0]]
    broken = scan.copy()
    broken[:8 * n].view(np.int32).reshape(n, 2)[1] = (1 << 30, 64)
    status = ops.jpeg_rst_entropy_device(torch.from_numpy(broken).cuda(), dev[1], dev[2], info.h, info.w, info.sampling)[2]
    assert status.cpu().tolist() == [[3, 0, 0, n]]


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _counted(ops, monkeypatch):
    calls = {"status": 0, "entropy": [], "decode": [], "host": 0, "plain": 0}
    real_s, real_e, real_d, real_h, real_p = ops.jpeg_status_download, ops.jpeg_rst_entropy_device, ops.jpeg_decode_coefs, ops.jpeg_entropy, ops.jpeg_entropy_device
    monkeypatch.setattr(ops, "jpeg_status_download", lambda s: (calls.__setitem__("status", calls["status"] + 1), real_s(s))[1])
    monkeypatch.setattr(ops, "jpeg_rst_entropy_device", lambda *a, **k: (calls["entropy"].append((a[5], a[1].shape[0])), real_e(*a, **k))[1])
    monkeypatch.setattr(ops, "jpeg_decode_coefs", lambda *a, **k: (calls["decode"].append((a[4], a[0].shape[0])), real_d(*a, **k))[1])
    monkeypatch.setattr(ops, "jpeg_entropy", lambda *a, **k: (calls.__setitem__("host", calls["host"] + 1), real_h(*a, **k))[1])
    monkeypatch.setattr(ops, "jpeg_entropy_device", lambda *a, **k: (calls.__setitem__("plain", calls["plain"] + 1), real_p(*a, **k))[1])
    return calls


def test_decode_restart_and_plain_frames_of_two_layouts(ops, monkeypatch):
    """restart and plain frames of 4:2:0 and 4:4:4 plus one progressive frame: per layout ONE entropy call, one decode call and one status
    download; the host's Huffman decoder is never called and only the progressive frame goes through `decode_image`"""
    from mv_ldm_amd import dataset as D
    noise, photo = J.pixels(45, 81, "noise"), J.pixels(45, 81, "photo")
    blobs = [J.restart_case(), J.encode(photo, quality=90, subsampling=0, restart_marker_blocks=5), J.encode(noise, quality=90, subsampling=2),
             J.encode(photo, quality=90, progressive=True), J.encode(noise, quality=50, subsampling=0), J.encode(photo, quality=100, subsampling=2, restart_marker_rows=2)]
    fell = []
    real = D.decode_image
    monkeypatch.setattr(D, "decode_image", lambda b: (fell.append(blobs.index(b)), real(b))[1])
    calls = _counted(ops, monkeypatch)
    out = ops.jpeg_decode(blobs, entropy="device", restarts="device")
    assert fell == [3] and calls["host"] == 0 and calls["plain"] == 0 and calls["status"] == 2
    assert sorted(calls["entropy"]) == sorted(calls["decode"]) == [(1, 2), (3, 3)]
    assert torch.equal(out.cpu(), _expect(blobs))
    monkeypatch.undo()
    assert torch.equal(out, ops.jpeg_decode(blobs)) and torch.equal(out, ops.jpeg_decode(blobs, entropy="device"))


def test_restarts_need_device_entropy(ops):
    blobs = [J.restart_case()]
    with pytest.raises(ValueError):
        ops.jpeg_decode(blobs, entropy="host", restarts="device")
    with pytest.raises(ValueError):
        ops.jpeg_decode(blobs, restarts="device")
    with pytest.raises(ValueError):
        ops.jpeg_decode(blobs, entropy="device", restarts="pillow")


def test_graph_capture(ops):
    """`jpeg_rst_entropy_device` + `jpeg_decode_coefs` on caller-given buffers, captured; the replay decodes new scans with another
    interval count"""
    noise, photo = J.pixels(45, 81, "noise"), J.pixels(45, 81, "photo")
    first = [J.encode(noise, quality=90, subsampling=2, restart_marker_rows=1), J.encode(photo, quality=90, subsampling=2)]
    other = [J.encode(photo, quality=50, subsampling=2, restart_marker_blocks=1, optimize=True), J.encode(noise, quality=90, subsampling=2, restart_marker_blocks=4)]
    room = max(sum(ops.jpeg_rst_need(b) for b in bs) for bs in (first, other))
    packed = []
    for bs in (first, other):
        scan, desc, tables, info = _pack(ops, bs, room)
        packed.append((scan, desc, tables))
    assert packed[0][1][:, 1].tolist() == [3, 1] and packed[1][1][:, 1].tolist() == [18, 5]
    h, w, sampling = info.h, info.w, info.sampling
    scan, desc, tables = (torch.from_numpy(a).cuda() for a in packed[0])
    count = ops.jpeg_coef_count(h, w, sampling)
    coef, qt = torch.empty(2, count, dtype=torch.int16, device="cuda"), torch.empty(2, 192, dtype=torch.int16, device="cuda")
    status = torch.empty(2, 4, dtype=torch.int32, device="cuda")
    dst = torch.zeros(2, h, w, 3, dtype=torch.uint8, device="cuda")
    ws = torch.empty(ops.jpeg_workspace_bytes(2, h, w, sampling), dtype=torch.uint8, device="cuda")

    def run():
        ops.jpeg_rst_entropy_device(scan, desc, tables, h, w, sampling, coef, qt, status)
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
    assert status.cpu()[:, [0, 3]].tolist() == [[0, 18], [0, 5]]


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k])
        elif isinstance(a[k], torch.Tensor):
            assert a[k].device == b[k].device and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_scene_reader_device_restarts(ops, tmp_path, monkeypatch):
    """a fixture scene whose JPEG frames are re-encoded with one restart interval per MCU row: the reader with `device_restarts=True`
    gives what the default reader gives, through the restart path and without the host's Huffman decoder"""
    from io import BytesIO
    from PIL import Image
    from mv_ldm_amd import dataset as D
    index = re10k_fixture.build(tmp_path / "re10k", jpeg_scenes=("a_one", "c_two"))
    marked = 0
    for path in sorted((tmp_path / "re10k" / "test").glob("*.torch")):
        chunk = torch.load(path, weights_only=True)
        for example in chunk:
            for i, frame in enumerate(example["images"]):
                blob = bytes(frame.numpy().tobytes())
                if blob[:2] == b"\xff\xd8":
                    buf = BytesIO()
                    Image.open(BytesIO(blob)).save(buf, format="JPEG", quality="keep", restart_marker_rows=1)
                    assert R.dri(buf.getvalue()) > 0
                    example["images"][i] = torch.frombuffer(bytearray(buf.getvalue()), dtype=torch.uint8)
                    marked += 1
        torch.save(chunk, path)
    assert marked >= 4
    default = list(D.RE10KScenes(tmp_path / "re10k", index=index, image_shape=(32, 32)))
    calls = _counted(ops, monkeypatch)
    device = list(D.RE10KScenes(tmp_path / "re10k", index=index, image_shape=(32, 32), device_restarts=True))
    assert calls["status"] >= 1 and len(calls["entropy"]) >= 1 and calls["host"] == 0 and calls["plain"] == 0 and len(default) == len(device) >= 4
    for a, b in zip(default, device):
        _same(a, b)
