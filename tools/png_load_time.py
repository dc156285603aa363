"""time the PNG reader (mv_ldm_amd/image_io.py load_images -> ops.png_decode: inflate on the host, csrc/png.hip on the device):
    python tools/png_load_time.py [--json OUT]
64 RGB frames of 256 x 256 ("photo": ramps plus +-12 of noise) in a temporary folder, as two input sets: (a) written by Pillow, which
picks a filter per row, (b) written by `image_io.save_image` (filter 0 on every row).  Per set, warm, medians of 7:
  * `load_images` of the 64 files, wall time per frame, without a pool and with a pool of 16 threads;
  * the parts, each alone: inflate (chunks, CRCs, zlib into the staging buffer; one thread, and the pool), upload (the staging buffer,
    between device events), kernel (`mvldm_png_unfilter` into fp32 [64, 3, 256, 256], between device events);
  * on (b) only -- the one thing the reader before this one could read: `torch.stack([load_image(p) for p in paths]).to(device)`.
The result is checked against Pillow before anything is timed.  No threshold: the figures go to DESIGN.md and profiles/."""
import json, os, statistics, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor
from io import BytesIO
from pathlib import Path
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image
from mv_ldm_amd import ops
from mv_ldm_amd.image_io import load_image, load_images, save_image

N, H, W = 64, 256, 256
yy, xx = np.mgrid[0:H, 0:W]
rec = {"frames": N, "frame": [H, W], "pillow": __import__("PIL").__version__, "device": torch.cuda.get_device_name(0),
       "arch": torch.cuda.get_device_properties(0).gcnArchName, "host_cpus_visible": len(os.sched_getaffinity(0)),
       "note": "warm, medians of 7, one run on one box; per frame = per call / 64"}
torch.set_num_threads(1)


def wall_ms(fn):
    out = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def event_ms(fn):
    out = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=16) as pool:
    sets = {"pillow_written": [], "save_image_written": []}
    for i in range(N):
        rng = np.random.default_rng(i)
        a = np.clip(np.stack([yy * 255 // (H - 1), xx * 255 // (W - 1), (yy + xx) * 255 // (H + W - 2)], axis=-1) + rng.integers(-12, 13, (H, W, 3)), 0, 255).astype(np.uint8)
        p = Path(tmp) / "a" / f"{i:06d}.png"
        p.parent.mkdir(exist_ok=True)
        Image.fromarray(a).save(p)
        sets["pillow_written"].append(p)
        q = Path(tmp) / "b" / f"{i:06d}.png"
        save_image(torch.from_numpy(a).permute(2, 0, 1).float() / 255, q)
        sets["save_image_written"].append(q)
    for name, paths in sets.items():
        blobs = [p.read_bytes() for p in paths]
        want = torch.stack([torch.from_numpy(np.array(Image.open(BytesIO(b)).convert("RGB"))).permute(2, 0, 1).float() / 255 for b in blobs])
        info = {}
        got = load_images(paths, "cuda", pool, info=info)
        assert torch.equal(got.cpu(), want) and info["fallback"] == [], name
        infos = [ops.png_probe(b) for b in blobs]
        offs, end, desc0, total = ops._png_layout(infos)
        buf = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        host = buf.numpy()
        desc = host[desc0:].view(np.int32).reshape(N, -1)
        stage = lambda i: ops._png_stage(blobs[i], infos[i], host, offs[i], end, 768 * i, desc[i])
        filters = sorted({int(v) for i in range(N) if stage(i) == 0 for v in host[offs[i]:offs[i] + infos[i].stream_bytes:1 + infos[i].stride]})
        on_dev = buf.cuda()
        dst = torch.empty(N, 3, H, W, dtype=torch.float32, device="cuda")
        status = torch.empty(N, dtype=torch.int32, device="cuda")
        r = rec[name] = {"file_bytes_per_frame": sum(map(len, blobs)) / N, "staged_bytes_per_frame": total / N, "filter_types": filters}
        r["load_images_ms_per_frame"] = wall_ms(lambda: load_images(paths, "cuda")) / N
        r["load_images_pool16_ms_per_frame"] = wall_ms(lambda: load_images(paths, "cuda", pool)) / N
        r["inflate_ms_per_frame"] = wall_ms(lambda: [stage(i) for i in range(N)]) / N
        r["inflate_pool16_ms_per_frame"] = wall_ms(lambda: list(pool.map(stage, range(N)))) / N
        r["upload_ms_per_frame"] = event_ms(lambda: on_dev.copy_(buf, non_blocking=True)) / N
        r["kernel_ms_per_frame"] = event_ms(lambda: ops.png_unfilter(on_dev, end, desc0, N, H, W, dst, status)) / N
        assert torch.equal(dst.cpu(), want) and status.cpu().tolist() == [0] * N
        if name == "save_image_written":
            r["previous_reader_ms_per_frame"] = wall_ms(lambda: torch.stack([load_image(p) for p in paths]).to("cuda")) / N
        print(name, json.dumps(r))
if "--json" in sys.argv:
    Path(sys.argv[sys.argv.index("--json") + 1]).write_text(json.dumps(rec, indent=1))
