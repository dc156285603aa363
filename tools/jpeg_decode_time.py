"""time the JPEG decoder (mv_ldm_amd/ops.py jpeg_decode: csrc/jpeg_host.cpp on the host, csrc/jpeg.hip on the device) next to Pillow:
    python tools/jpeg_decode_time.py [--entropy] [--restarts] [--json OUT]
Two 360 x 640 4:2:0 quality-90 frames built here: "fixture" (tests/train_fixture.py's kind: 45 x 80 noise repeated 8 x each way, so every
luma block is flat) and "photo" (smooth ramps plus +-12 of noise: every block has AC coefficients).  Per frame:
  * host: `mvldm_jpeg_entropy` (markers + Huffman scan into a reused buffer) on ONE thread, best of 5 passes of 20 calls, ms a frame; and
    Pillow's whole decode of the same bytes (`Image.open(...).convert("RGB")` to a numpy array) on one core of the same box, likewise.
  * device: `mvldm_jpeg_decode` of n = 5 and n = 30 copies, coefficients already on the device, microseconds per frame.  "hot": the median
    of 5 windows of back-to-back calls between device events; "cold": one call per window behind a 640 MB fill that evicts the 256 MiB
    last-level cache, median of 7.
  * `--entropy`: the Huffman scan on the device (`mvldm_jpeg_entropy_device`, csrc/jpeg_huff.hip), prepared scans already on the device: per
    subseq_bits in 128, 256, 512, 1024 and n = 5, 30 the same hot / cold microseconds per frame, the rounds the worst chunk took and the
    bytes uploaded per frame (scan with padding + tables + descriptor); next to it, IN THE SAME RUN, the host's entropy pass spread over a
    pool of 16 threads (wall time of 30 frames / 30) and `mvldm_jpeg_scan_prepare` on one thread.  Coefficients are checked against the
    host's before anything is timed.
  * `--restarts`: the same pixels re-encoded with `restart_marker_rows=1` (one restart interval per MCU row: 23 of 40 MCUs) through
    `mvldm_jpeg_rst_entropy_device` (csrc/jpeg_huff.hip): per subseq_bits in 128, 256, 512, 1024 and n = 5, 30 the hot / cold microseconds
    per frame and the rounds of the worst chunk; next to it, IN THE SAME RUN, `mvldm_jpeg_entropy_device` on the stream without markers,
    the host's entropy pass of the restart stream on one thread and over 16 workers, `mvldm_jpeg_rst_prepare` on one thread and the bytes
    uploaded per frame.  Coefficients are checked against the host's before anything is timed.  The same again under
    "device_restarts_8_mcus" for `restart_marker_blocks=8` (an interval of 8 MCUs, about 3,000 bits: shorter than the ~9,000 bits a cold
    decoder needs to synchronise, which an MCU row of 40 is not).
The device result is checked against Pillow's before anything is timed.  No threshold: the figures go to DESIGN.md and profiles/."""
import json, os, sys, time
from io import BytesIO
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image
from mv_ldm_amd import ops

H, W = 360, 640
rng = np.random.default_rng(0)
yy, xx = np.mgrid[0:H, 0:W]
FRAMES = {
    "fixture": rng.integers(0, 256, (H // 8, W // 8, 3), dtype=np.uint8).repeat(8, axis=0).repeat(8, axis=1),
    "photo": np.clip(np.stack([yy * 255 // (H - 1), xx * 255 // (W - 1), (yy + xx) * 255 // (H + W - 2)], axis=-1) + rng.integers(-12, 13, (H, W, 3)), 0, 255).astype(np.uint8),
}
rec = {"frame": [H, W], "format": "4:2:0, quality 90, Pillow " + __import__("PIL").__version__, "device": torch.cuda.get_device_name(0),
       "arch": torch.cuda.get_device_properties(0).gcnArchName, "host_cpus_visible": len(os.sched_getaffinity(0)),
       "note": "host: ms per frame, one thread, best of 5 passes of 20; device: us per frame, hot = median of 5 windows of back-to-back calls, "
               "cold = one call behind a 640 MB fill, median of 7; one run on one box"}
flush = torch.empty(640 << 20, dtype=torch.uint8, device="cuda")
torch.set_num_threads(1)


def event_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def best_ms(fn):
    best = float("inf")
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(20):
            fn()
        best = min(best, (time.perf_counter() - t0) / 20)
    return best * 1e3


for name, pixels in FRAMES.items():
    buf = BytesIO()
    Image.fromarray(pixels).save(buf, format="JPEG", quality=90, subsampling=2)
    blob = buf.getvalue()
    want = np.asarray(Image.open(BytesIO(blob)).convert("RGB"))
    info = ops.jpeg_probe(blob)
    assert info.supported and info.sampling == 3
    count = ops.jpeg_coef_count(H, W, 3)
    coef, qt = np.zeros(count, dtype=np.int16), np.zeros(192, dtype=np.int16)
    reason, max_s = ops.jpeg_entropy(blob, coef, qt)
    assert reason == 0, reason
    r = rec[name] = {"stream_bytes": len(blob), "largest_block_S": max_s,
                     "host_entropy_ms_per_frame": round(best_ms(lambda: ops.jpeg_entropy(blob, coef, qt)), 4),
                     "pillow_decode_ms_per_frame": round(best_ms(lambda: np.asarray(Image.open(BytesIO(blob)).convert("RGB"))), 4)}
    for n in (5, 30):
        dc = torch.from_numpy(coef).cuda().repeat(n, 1)
        dq = torch.from_numpy(qt).cuda().repeat(n, 1)
        dst = torch.empty(n, H, W, 3, dtype=torch.uint8, device="cuda")
        ws = torch.empty(ops.jpeg_workspace_bytes(n, H, W, 3), dtype=torch.uint8, device="cuda")
        call = lambda: ops.jpeg_decode_coefs(dc, dq, H, W, 3, dst, ws)
        call()
        torch.cuda.synchronize()
        assert all(np.array_equal(dst[i].cpu().numpy(), want) for i in (0, n - 1)), "the device result is not Pillow's"
        hot = sorted(event_us(call, 50 if n == 5 else 20) for _ in range(5))[2]
        cold = []
        for _ in range(7):
            flush.fill_(1)
            cold.append(event_us(call, 1))
        cold = sorted(cold)[3]
        r[f"device_n{n}"] = {"hot_us_per_frame": round(hot / n, 3), "cold_us_per_frame": round(cold / n, 3), "hot_us_per_call": round(hot, 2),
                             "cold_us_per_call": round(cold, 2), "coefficient_bytes_per_frame": count * 2}
    if "--entropy" in sys.argv:
        from concurrent.futures import ThreadPoolExecutor
        from mv_ldm_amd import _lib
        e = r["device_entropy"] = {}
        p = ops.jpeg_scan_prepare(blob)
        assert p.reason == 0
        room = int(p.desc[2])
        e["scan_bytes"] = int(p.desc[1]) // 8
        e["upload_bytes_per_frame"] = room + _lib.JPEG_TABLE_BYTES + 16
        e["prepare_ms_per_frame"] = round(best_ms(lambda: ops.jpeg_scan_prepare(blob, p.scan, 0, p.desc, p.tables)), 4)
        with ThreadPoolExecutor(16) as pool:
            bufs = [(np.zeros(count, dtype=np.int16), np.zeros(192, dtype=np.int16)) for _ in range(30)]
            spread = lambda: list(pool.map(lambda b: ops.jpeg_entropy(blob, b[0], b[1]), bufs))
            e["host_entropy_16_workers_ms_per_frame"] = round(best_ms(spread) / 30, 4)
        for n in (5, 30):
            scan = torch.from_numpy(p.scan[:room]).cuda().repeat(n)
            desc = torch.from_numpy(p.desc).cuda().repeat(n, 1)
            desc[:, 0] = torch.arange(n, device="cuda", dtype=torch.int32) * room
            tables = torch.from_numpy(p.tables).cuda().repeat(n, 1)
            dc, dq = torch.empty(n, count, dtype=torch.int16, device="cuda"), torch.empty(n, 192, dtype=torch.int16, device="cuda")
            st = torch.empty(n, 4, dtype=torch.int32, device="cuda")
            for sb in (128, 256, 512, 1024):
                call = lambda: ops.jpeg_entropy_device(scan, desc, tables, H, W, 3, dc, dq, st, subseq_bits=sb)
                call()
                torch.cuda.synchronize()
                status = st.cpu().numpy()
                assert (status[:, 0] == 0).all() and (status[:, 1] == max_s).all(), status
                assert all(np.array_equal(dc[i].cpu().numpy(), coef) and np.array_equal(dq[i].cpu().numpy(), qt) for i in (0, n - 1)), "not the host's coefficients"
                hot = sorted(event_us(call, 20) for _ in range(5))[2]
                cold = []
                for _ in range(7):
                    flush.fill_(1)
                    cold.append(event_us(call, 1))
                cold = sorted(cold)[3]
                e[f"n{n}_bits{sb}"] = {"hot_us_per_frame": round(hot / n, 3), "cold_us_per_frame": round(cold / n, 3), "hot_us_per_call": round(hot, 2),
                                       "cold_us_per_call": round(cold, 2), "rounds": int(status[:, 2].max())}
    if "--restarts" in sys.argv:
        from concurrent.futures import ThreadPoolExecutor
        from mv_ldm_amd import _lib
        for tag, markers in (("device_restarts", dict(restart_marker_rows=1)), ("device_restarts_8_mcus", dict(restart_marker_blocks=8))):
            e = r[tag] = {}
            buf = BytesIO()
            Image.fromarray(pixels).save(buf, format="JPEG", quality=90, subsampling=2, **markers)
            rblob = buf.getvalue()
            rcoef, rqt = np.zeros(count, dtype=np.int16), np.zeros(192, dtype=np.int16)
            reason, rmax_s = ops.jpeg_entropy(rblob, rcoef, rqt)
            assert reason == 0 and np.array_equal(np.asarray(Image.open(BytesIO(rblob)).convert("RGB")), want), "markers change no pixel"
            plain, marked = ops.jpeg_scan_prepare(blob), ops.jpeg_rst_prepare(rblob)
            assert plain.reason == 0 and marked.reason == 0
            e["stream_bytes"], e["stream_bytes_without_markers"], e["intervals"], e["mcus_per_interval"] = len(rblob), len(blob), int(marked.desc[1]), int(marked.desc[3])
            e["upload_bytes_per_frame"] = int(marked.desc[2]) + _lib.JPEG_TABLE_BYTES + 16
            e["upload_bytes_per_frame_without_markers"] = int(plain.desc[2]) + _lib.JPEG_TABLE_BYTES + 16
            e["coefficient_bytes_per_frame"] = count * 2
            e["prepare_ms_per_frame"] = round(best_ms(lambda: ops.jpeg_rst_prepare(rblob, marked.scan, 0, marked.desc, marked.tables)), 4)
            e["host_entropy_ms_per_frame"] = round(best_ms(lambda: ops.jpeg_entropy(rblob, rcoef, rqt)), 4)
            with ThreadPoolExecutor(16) as pool:
                bufs = [(np.zeros(count, dtype=np.int16), np.zeros(192, dtype=np.int16)) for _ in range(30)]
                spread = lambda: list(pool.map(lambda b: ops.jpeg_entropy(rblob, b[0], b[1]), bufs))
                e["host_entropy_16_workers_ms_per_frame"] = round(best_ms(spread) / 30, 4)
            for n in (5, 30):
                dc, dq = torch.empty(n, count, dtype=torch.int16, device="cuda"), torch.empty(n, 192, dtype=torch.int16, device="cuda")
                st = torch.empty(n, 4, dtype=torch.int32, device="cuda")
                for key, p, fn, hcoef, hmax in (("restarts", marked, ops.jpeg_rst_entropy_device, rcoef, rmax_s), ("no_markers", plain, ops.jpeg_entropy_device, coef, max_s)):
                    room = int(p.desc[2])
                    scan = torch.from_numpy(p.scan[:room]).cuda().repeat(n)
                    desc = torch.from_numpy(p.desc).cuda().repeat(n, 1)
                    desc[:, 0] = torch.arange(n, device="cuda", dtype=torch.int32) * room
                    tables = torch.from_numpy(p.tables).cuda().repeat(n, 1)
                    for sb in (128, 256, 512, 1024):
                        call = lambda: fn(scan, desc, tables, H, W, 3, dc, dq, st, subseq_bits=sb)
                        call()
                        torch.cuda.synchronize()
                        status = st.cpu().numpy()
                        assert (status[:, 0] == 0).all() and (status[:, 1] == hmax).all(), status
                        assert all(np.array_equal(dc[i].cpu().numpy(), hcoef) and np.array_equal(dq[i].cpu().numpy(), rqt) for i in (0, n - 1)), "not the host's coefficients"
                        hot = sorted(event_us(call, 20) for _ in range(5))[2]
                        cold = []
                        for _ in range(7):
                            flush.fill_(1)
                            cold.append(event_us(call, 1))
                        cold = sorted(cold)[3]
                        e[f"{key}_n{n}_bits{sb}"] = {"hot_us_per_frame": round(hot / n, 3), "cold_us_per_frame": round(cold / n, 3), "hot_us_per_call": round(hot, 2),
                                                     "cold_us_per_call": round(cold, 2), "rounds": int(status[:, 2].max())}
    print(name, json.dumps(r), flush=True)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(rec, f, indent=1)
print(json.dumps(rec))
