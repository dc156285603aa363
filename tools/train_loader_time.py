"""views/s of the training loader (mv_ldm_amd/dataset.py `RE10KTrainLoader`: container decode on the host, one pinned upload and one flagged
crop-shim call per batch) next to what the trainer consumes:
    python tools/train_loader_time.py [--device-decode] [--device-entropy] [--json OUT]
A tree of one chunk of 12 scenes x 8 frames of 360 x 640 (tests/train_fixture.py's frames: 45 x 80 noise repeated 8 x each way -- a PNG of
it inflates fast and a JPEG of it is blocky, so both decode at the cheap end of what real frames cost), PNG (decoded by `image_io`) and
JPEG quality 90 (decoded by Pillow), batches of 6 scenes x (2 + 3) views = 30 frames -> 256 x 256, `augment` on, at `decode_workers` 0 and
16.  Per combination: one epoch to warm up, then wall-clock seconds of 5 epochs (10 batches, 300 views) ending in a device synchronise,
best and worst of 3 repeats; and the host's decode alone, one thread, ms a frame.  No threshold: the figures go to DESIGN.md and
profiles/.  `--device-decode` adds a second JPEG column: the same loader with `device_decode=True` (the Huffman scan on the host -- on the
decode workers, without the GIL --, the inverse DCT, upsampling and colour on the device: `ops.jpeg_decode`), and the host's entropy pass
alone, one thread, ms a frame.  `--device-entropy` adds a third: `device_entropy=True` (the workers only remove the byte stuffing, the
Huffman scan is decoded on the device too)."""
import json
import os
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import torch
import train_fixture as F
from mv_ldm_amd import dataset as D

F.SCENES = {f"t_{i:02d}": (8, 0.9, 0.1) for i in range(12)}
F.CHUNKS = {"000000.torch": tuple(F.SCENES)}
EPOCHS, REPEATS = 5, 3
DEVICE_DECODE = "--device-decode" in sys.argv
DEVICE_ENTROPY = "--device-entropy" in sys.argv
rec = {"frames": [F.H, F.W], "shape": [256, 256], "batch": "6 scenes x (2 + 3) views", "device": torch.cuda.get_device_name(0), "host_cpus_visible": len(os.sched_getaffinity(0)),
       "note": f"views/s over {EPOCHS} epochs of 2 batches (300 views) after a warm-up epoch, wall clock to a device synchronise, best / worst of {REPEATS}; "
               "frames are 8 x repeated noise (cheap to decode in either container)"}
with tempfile.TemporaryDirectory() as tmp:
    for kind in ("png", "jpeg"):
        root = F.build(Path(tmp) / kind, jpeg=kind == "jpeg")
        blobs = [D._frame_bytes(f) for f in torch.load(root / "train" / "000000.torch", weights_only=True)[0]["images"]]
        t0 = time.perf_counter()
        for _ in range(3):
            for b in blobs:
                D.decode_image(b)
        rec[f"{kind}_decode_ms_per_frame_one_thread"] = round((time.perf_counter() - t0) / (3 * len(blobs)) * 1e3, 3)
        rec[f"{kind}_bytes_per_frame"] = sum(len(b) for b in blobs) // len(blobs)
        if kind == "jpeg" and DEVICE_DECODE:
            import numpy as np
            from mv_ldm_amd import ops
            info = ops.jpeg_probe(blobs[0])
            coef, qt = np.zeros(ops.jpeg_coef_count(info.h, info.w, info.sampling), dtype=np.int16), np.zeros(192, dtype=np.uint16)
            t0 = time.perf_counter()
            for _ in range(3):
                for b in blobs:
                    assert ops.jpeg_entropy(b, coef, qt)[0] == 0
            rec["jpeg_entropy_ms_per_frame_one_thread"] = round((time.perf_counter() - t0) / (3 * len(blobs)) * 1e3, 3)
        modes = [""] + (["_device_decode"] if DEVICE_DECODE else []) + (["_device_entropy"] if DEVICE_ENTROPY else []) if kind == "jpeg" else [""]
        for workers, mode in [(w, d) for d in modes for w in (0, 16)]:
            torch.manual_seed(0)
            loader = D.RE10KTrainLoader(root, view_sampler=D.get_view_sampler("bounded", **F.SAMPLER), augment=True, decode_workers=workers,
                                        device_decode=mode == "_device_decode", device_entropy=mode == "_device_entropy")
            assert sum(len(b["scene"]) for b in loader) == 12
            rates = []
            for _ in range(REPEATS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                views = 0
                for _ in range(EPOCHS):
                    for b in loader:
                        views += b["context"]["image"].shape[0] * (b["context"]["image"].shape[1] + b["target"]["image"].shape[1])
                torch.cuda.synchronize()
                rates.append(views / (time.perf_counter() - t0))
            key = f"{kind}{mode}_workers{workers}_views_per_s"
            rec[key] = {"best": round(max(rates), 1), "worst": round(min(rates), 1)}
            print(key, rec[key], flush=True)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(rec, f, indent=1)
print(json.dumps(rec))
