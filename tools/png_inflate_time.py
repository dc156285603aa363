"""time the PNG reader with IDAT inflated on the host (the default) and on the device (`inflate="device"`: csrc/inflate.hip):
    python tools/png_inflate_time.py [--json OUT]
The frames of tools/png_load_time.py: 64 RGB frames of 256 x 256 ("photo": ramps plus +-12 of noise) in a temporary folder, as two input
sets: (a) written by Pillow, which picks a filter per row, (b) written by `image_io.save_image` (filter 0 on every row).  Per set and per
batch size (32: a `cleanfid` batch; 64: the profile's and a `metrics` batch; 256: the 64 files four times), warm, medians of 7:
  * `load_images` with `inflate="host"` -- the path as it was -- without a pool, with 8 workers (what `metrics` and `cleanfid` use) and
    with 16, wall time per frame;
  * `load_images` with `inflate="device"`, without a pool and with 8 workers (the chunk walk and its CRCs are the host's on this path too);
  * the inflate kernel alone (`mvldm_png_inflate`, between device events) and the unfilter kernel behind it;
  * the bytes uploaded per frame on either path.
Both paths are checked against Pillow before anything is timed.  No threshold: the figures go to DESIGN.md, README.md and profiles/."""
import json, os, statistics, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor
from io import BytesIO
from pathlib import Path
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image
from mv_ldm_amd import _lib as L
from mv_ldm_amd import ops
from mv_ldm_amd.image_io import load_images, save_image

N, H, W = 64, 256, 256
yy, xx = np.mgrid[0:H, 0:W]
props = torch.cuda.get_device_properties(0)
rec = {"frames": N, "frame": [H, W], "pillow": __import__("PIL").__version__, "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName,
       "compute_units": props.multi_processor_count, "host": os.uname().nodename, "host_cpus_visible": len(os.sched_getaffinity(0)),
       "note": "warm, medians of 7, one run on one box; per frame = per call / batch; batch 256 reads the 64 files four times"}
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


with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=8) as pool8, ThreadPoolExecutor(max_workers=16) as pool16:
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
    for name, files in sets.items():
        rec[name] = {}
        for batch in (32, 64, 256):
            paths = (files * 4)[:batch]
            blobs = [p.read_bytes() for p in paths]
            want = torch.stack([torch.from_numpy(np.array(Image.open(BytesIO(b)).convert("RGB"))).permute(2, 0, 1).float() / 255 for b in blobs[:N]])
            want = torch.cat([want] * 4)[:batch]
            for mode in ("host", "device"):
                info = {}
                got = load_images(paths, "cuda", pool8, info=info, inflate=mode)
                assert torch.equal(got.cpu(), want) and info["fallback"] == [], (name, batch, mode)
            infos = [ops.png_probe(b) for b in blobs]
            r = rec[name][f"batch_{batch}"] = {"file_bytes_per_frame": sum(map(len, blobs)) / batch, "host_upload_bytes_per_frame": ops._png_layout(infos)[3] / batch,
                                               "device_upload_bytes_per_frame": info["upload_bytes"] / batch}
            r["host_ms_per_frame"] = wall_ms(lambda: load_images(paths, "cuda")) / batch
            r["host_pool8_ms_per_frame"] = wall_ms(lambda: load_images(paths, "cuda", pool8)) / batch
            r["host_pool16_ms_per_frame"] = wall_ms(lambda: load_images(paths, "cuda", pool16)) / batch
            r["device_ms_per_frame"] = wall_ms(lambda: load_images(paths, "cuda", inflate="device")) / batch
            r["device_pool8_ms_per_frame"] = wall_ms(lambda: load_images(paths, "cuda", pool8, inflate="device")) / batch
            buf, keep, zend, send, desc0, zdesc0 = ops._png_zstage(blobs, infos, pool8, {}, pin=True)
            on_dev = buf.cuda()
            base = on_dev.data_ptr()
            streams = torch.empty(send, dtype=torch.uint8, device="cuda")
            dst = torch.empty(batch, 3, H, W, dtype=torch.float32, device="cuda")
            both = torch.empty(2, batch, dtype=torch.int32, device="cuda")
            lib = L.load()
            inflate = lambda: L.check(lib.mvldm_png_inflate(base, zend, base + zdesc0, streams.data_ptr(), send, base + desc0, batch, H, W, both[0].data_ptr(), ops.stream()))
            unfilter = lambda: L.check(lib.mvldm_png_unfilter(streams.data_ptr(), send, base + desc0, base + zend, 768 * batch, dst.data_ptr(), L.PNG_DST_F32, batch, H, W,
                                                              both[1].data_ptr(), ops.stream()))
            r["stage_pool8_ms_per_frame"] = wall_ms(lambda: ops._png_zstage(blobs, infos, pool8, {}, pin=True)) / batch
            r["upload_ms_per_frame"] = event_ms(lambda: on_dev.copy_(buf, non_blocking=True)) / batch
            r["inflate_kernel_ms_per_frame"] = event_ms(inflate) / batch
            r["inflate_kernel_ms_per_call"] = r["inflate_kernel_ms_per_frame"] * batch
            r["unfilter_kernel_ms_per_frame"] = event_ms(unfilter) / batch
            assert torch.equal(dst.cpu(), want) and both.cpu().tolist() == [[0] * batch] * 2
            r["device_ahead_of_host_pool8"] = r["device_pool8_ms_per_frame"] < r["host_pool8_ms_per_frame"]
            print(name, batch, json.dumps(r), flush=True)
if "--json" in sys.argv:
    Path(sys.argv[sys.argv.index("--json") + 1]).write_text(json.dumps(rec, indent=1))
