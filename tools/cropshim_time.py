"""time the crop shim on the device (mv_ldm_amd/ops.py crop_shim, csrc/cropshim.hip) next to PIL on the host:
    python tools/cropshim_time.py [h=360] [w=640] [out=256] [--json OUT]
  * device: microseconds per image at n = 5 (one view group) and n = 320 (a training step's worth), uint8 [n, h, w, 3] in, fp32
    [n, 3, out, out] out, tables warm.  "hot": the median of 5 windows of back-to-back calls between device events on one input set (its
    bytes stay in the caches); "cold": one call per window behind a 640 MB fill that evicts the 256 MiB last-level cache, median of 7.
  * host: the reference's three steps per image -- Image.fromarray(...).resize((w_s, h_s), LANCZOS), the crop, / 255 -- on ONE core
    (torch.set_num_threads(1); Pillow's resize is single-threaded), best of 3 passes over 20 images.
No threshold: the figures go to DESIGN.md and profiles/."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mv_ldm_amd import ops

args = [int(a) for a in sys.argv[1:] if a.isdigit()]
h, w, res = (args + [360, 640, 256][len(args):])[:3]
shape = (res, res)
h_s, w_s, row, col = ops.crop_geometry(h, w, shape)
rec = {"source": [h, w], "shape": list(shape), "scaled": [h_s, w_s], "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
       "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
       "note": "us per image; hot = median of 5 windows of back-to-back calls, cold = one call behind a 640 MB fill, median of 7"}
flush = torch.empty(640 << 20, dtype=torch.uint8, device="cuda")


def event_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


for n in (5, 320):
    src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
    ws = torch.empty(ops.crop_shim_workspace_bytes(n, h, w, shape), dtype=torch.uint8, device="cuda")
    call = lambda: ops.crop_shim(src, shape, ws)
    call()
    torch.cuda.synchronize()
    iters = 50 if n == 5 else 5
    hot = sorted(event_us(call, iters) for _ in range(5))[2]
    cold = []
    for _ in range(7):
        flush.fill_(1)
        cold.append(event_us(call, 1))
    cold = sorted(cold)[3]
    rec[f"n{n}"] = {"hot_us_per_image": hot / n, "cold_us_per_image": cold / n, "hot_us_per_call": hot, "cold_us_per_call": cold,
                    "source_GB_per_s_hot": n * h * w * 3 / (hot * 1e-6) / 1e9}
    print(f"n = {n}: {hot / n:.2f} us / image hot, {cold / n:.2f} us / image cold ({hot:.0f} / {cold:.0f} us a call)")

try:
    from PIL import Image
except ImportError:
    Image = None
    rec["host"] = "Pillow is not installed: not measured"
if Image is not None:
    torch.set_num_threads(1)
    imgs = np.random.default_rng(0).integers(0, 256, (20, h, w, 3), dtype=np.uint8)
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        for im in imgs:
            out = np.array(Image.fromarray(im).resize((w_s, h_s), Image.LANCZOS))[row:row + res, col:col + res] / 255
            torch.tensor(out, dtype=torch.float32)
        best = min(best, (time.perf_counter() - t0) / len(imgs))
    rec["host"] = {"pil_us_per_image_one_core": best * 1e6, "pil_version": __import__("PIL").__version__, "cpu": os.uname().machine}
    print(f"host (PIL {rec['host']['pil_version']}, one core): {best * 1e6:.0f} us / image")
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(rec, f, indent=1)
print(json.dumps(rec))
