"""time one `ops.image_metrics` launch (csrc/metrics.hip) on the sampler's output shape and set it against the time two reads of
the inputs take at an HBM rate.  python tools/metrics_time.py [n_img=256] [res=256] [--json OUT]
Both inputs (2 x n x 3 x res x res fp32) are larger than the 256 MB Infinity Cache at the default size; the buffers are rotated
anyway so that no launch finds the previous one's lines."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mv_ldm_amd import ops

args = [a for a in sys.argv[1:] if a.isdigit()]
n, res = (int(args[0]) if args else 256), (int(args[1]) if len(args) > 1 else 256)
HBM = 5.0e12          # B/s: the lower end of what GroupNorm's apply-only pass streams at (4.9 - 5.6 TB/s)
sets = [(torch.rand(n, 3, res, res, device="cuda"), torch.rand(n, 3, res, res, device="cuda")) for _ in range(3)]
out = (torch.empty(n, device="cuda"), torch.empty(n, device="cuda"))
ws = torch.empty(ops.image_metrics_workspace_bytes(n, 3, res, res), dtype=torch.uint8, device="cuda")
for a, b in sets:
    ops.image_metrics(a, b, out=out, ws=ws)
torch.cuda.synchronize()
times = []
for rep in range(5):
    iters = 60
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        a, b = sets[i % 3]
        ops.image_metrics(a, b, out=out, ws=ws)
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) * 1e3 / iters)
us = sorted(times)[len(times) // 2]
nbytes = 2 * n * 3 * res * res * 4
rec = {"shape": [n, 3, res, res], "launch_us_median_of_5x60": round(us, 1), "launch_us_all": [round(t, 1) for t in times],
       "input_bytes": nbytes, "achieved_read_GBps": round(nbytes / us / 1e3, 1), "hbm_rate_assumed_TBps": HBM / 1e12,
       "two_reads_at_hbm_rate_us": round(nbytes / HBM * 1e6, 1), "fma_per_pixel": 110,
       "note": "kernel + fold launches, device events around 60 back-to-back calls, inputs rotated over 3 buffer pairs"}
print(json.dumps(rec))
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(rec, f, indent=1)
