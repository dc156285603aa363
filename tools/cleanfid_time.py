"""time Clean-FID on the device (mv_ldm_amd/cleanfid.py, csrc/inception.hip):  python tools/cleanfid_time.py [images=32] [res=256] [--json OUT]
  * the extractor (resize to 299 x 299, the 94 convolutions, pools, the fp64 mean) in images / s at res x res uint8 inputs, in f32, f16 and
    bf16, and its parts at f32: the resize alone, the unfold launches alone;
  * the Frechet distance at d = 2048 in ms, on a rank-deficient pair of states (`images` samples a side: the reference's use) and on a
    full-rank pair, with the sweeps each solve took.
Random weights (timing does not depend on them).  Extractor figures: the median of 5 windows of back-to-back calls between device
events, after a warm-up; inputs rotate over 3 buffer sets.  The solve is timed call by call (it enqueues ~ 10^5 launches): median of 3."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mv_ldm_amd import ops
from mv_ldm_amd.cleanfid import FEATURES, LAYERS, SIZE, InceptionPool3

args = [a for a in sys.argv[1:] if a.isdigit()]
n, res = (int(args[0]) if args else 32), (int(args[1]) if len(args) > 1 else 256)


def median_us(fn, iters, windows=5):
    fn(0)
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / iters)
    return sorted(times)[len(times) // 2]


model = InceptionPool3(allow_random_init=True).cuda()
sets = [torch.randint(0, 256, (n, 3, res, res), dtype=torch.uint8, device="cuda") for _ in range(3)]
rec = {"images": n, "res": res, "note": "median of 5 windows of back-to-back calls between device events; 3 rotating input sets"}
out = torch.empty(n, FEATURES, dtype=torch.float64, device="cuda")
for dtype in (torch.float32, torch.float16, torch.bfloat16):
    name = str(dtype).split(".")[-1]
    ws = torch.empty(model.workspace_bytes(n, res, res, dtype), dtype=torch.uint8, device="cuda")
    us = median_us(lambda i: model.features(sets[i % 3], dtype=dtype, out=out, ws=ws), 3)
    rec[name] = {"extractor_us": us, "images_per_s": n / (us * 1e-6)}
    print(f"{name}: extractor {us / 1e3:.2f} ms for {n} images of {res} x {res} = {n / (us * 1e-6):.0f} images / s")
us = median_us(lambda i: ops.inception_prep(sets[i % 3], torch.float32, SIZE, SIZE), 10)
rec["float32"]["prep_us"] = us
unfolded = [(c_in, k) for _, c_in, _, k, _, _ in LAYERS if not (k[0] == k[1] and k[0] in (1, 3))]
edge = {48: 35, 128: 17, 160: 17, 192: 17, 384: 8}
maps = [torch.randn(n, edge[c], edge[c], c, device="cuda") for c, _ in unfolded]
us_unfold = median_us(lambda i: [ops.inception_unfold(x, *k) for x, (_, k) in zip(maps, unfolded)], 3)
rec["float32"]["unfold_us"] = us_unfold
print(f"float32 parts: resize {us / 1e3:.2f} ms, the {len(unfolded)} unfold launches {us_unfold / 1e3:.2f} ms")
del maps

# the solve
d = FEATURES
score = torch.empty(1, device="cuda")
info = torch.empty(ops.FID_INFO, dtype=torch.float64, device="cuda")
ws = torch.empty(ops.frechet_workspace_bytes(d), dtype=torch.uint8, device="cuda")


def state_of(rows, seed):
    f = torch.rand(rows, d, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(seed)) * torch.linspace(0.2, 2.0, d, dtype=torch.float64, device="cuda")
    st = torch.zeros(ops.frechet_state_size(d), dtype=torch.float64, device="cuda")
    for i in range(0, rows, 256):
        ops.frechet_accumulate(f[i:i + 256].contiguous(), st)
    return st


for label, rows in (("deficient", n), ("full_rank", 2 * d)):
    s1, s2 = state_of(rows, 1), state_of(rows, 2)
    times = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.frechet_compute(s1, s2, score, info, ws)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    rec[f"solve_{label}"] = {"samples_a_side": rows, "ms": sorted(times)[1], "sweeps": [int(info[0]), int(info[2])], "capped": int(info[4]), "fid": float(score)}
    print(f"solve d = {d}, {label} ({rows} samples a side): {sorted(times)[1]:.0f} ms, sweeps {int(info[0])} + {int(info[2])}, capped {int(info[4])}")
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(rec, f, indent=1)
print(json.dumps(rec))
