"""time DISTS on the device (mv_ldm_amd/dists.py, csrc/dists.hip) at the sampler's output shape, in f32 and f16, and set the parts against
what they move:  python tools/dists_time.py [pairs=64] [res=256] [--json OUT]
  * the 13 convs of the trunk (2 x pairs images, one launch each) against their FLOPs -- at f16 also against the 16-bit conv rate measured
    in profiles/r05_conv_vs_miopen.json ("L0 320->320 @32", best tile: 1240 TFLOP/s); profiles/ holds no f32 conv rate, so f32 reports the
    achieved rate alone;
  * the six statistics launches (the raw image and the five stages; fp64 sums), the four L2 pools and the eight ReLU launches against
    their bytes at 5 TB/s (the streaming figure of DESIGN.md §3.5); the fold against the partials it reads;
  * end to end (prep + convs + ReLUs + statistics + pools + fold) against the PSNR / SSIM launch on the same pairs.
Random weights (timing does not depend on them).  Every figure is the median of 5 windows of back-to-back calls between device events,
after a warm-up of every shape; inputs rotate over 3 buffer sets."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mv_ldm_amd import ops
from mv_ldm_amd.dists import DISTS, VGG_STAGES, VGG_WIDTH

args = [a for a in sys.argv[1:] if a.isdigit()]
n, res = (int(args[0]) if args else 64), (int(args[1]) if len(args) > 1 else 256)
HBM = 5.0e12
CONV_RATE = {"float16": 1240e12}          # profiles/r05_conv_vs_miopen.json, "L0 320->320 @32", tile 10


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


model = DISTS(allow_random_init=True).cuda()
sets = [(torch.rand(n, 3, res, res, device="cuda"), torch.rand(n, 3, res, res, device="cuda")) for _ in range(3)]
rec = {"pairs": n, "res": res, "hbm_rate_assumed_TBps": HBM / 1e12, "note": "median of 5 windows of back-to-back calls between device events; 3 rotating input sets"}
out = torch.empty(n, device="cuda")
taps, stride = ops.dists_layout(res, res)
alpha, beta = model.alpha.view(-1), model.beta.view(-1)
for dtype in (torch.float32, torch.float16):
    name = str(dtype).split(".")[-1]
    es = 4 if dtype == torch.float32 else 2
    if DISTS.chunk_pairs(res, res, dtype) < n:
        raise SystemExit(f"{n} pairs of {res} x {res} in {name} are more than one chunk: time a smaller batch")
    ws = torch.empty(ops.dists_workspace_bytes(n, res, res), dtype=torch.uint8, device="cuda")
    convs, packs = model._packed(dtype)
    # the operands of every launch, as forward() makes them
    conv_jobs, relu_jobs, stat_jobs, pool_jobs = [], [], [], []
    flops = relu_bytes = pool_bytes = 0
    stat_bytes = 2 * n * 3 * res * res * 4 + n * ops.dists_stat_slots(res, res, 3) * 15 * 8     # tap 0: the raw fp32 images
    h = w = res
    c_in, k = ops.epc(dtype), 0
    for l, (s, idx) in enumerate(VGG_STAGES.items()):
        c = VGG_WIDTH[s]
        for j in range(len(idx)):
            x = torch.randn(2 * n, h, w, c_in, device="cuda").to(dtype)
            conv_jobs.append((x, packs[k], convs[k].bias))
            flops += 2 * 2 * n * h * w * 9 * (3 if k == 0 else c_in) * c
            if j + 1 < len(idx):
                relu_jobs.append(torch.randn(2 * n, h, w, c, device="cuda").to(dtype))
                relu_bytes += 2 * 2 * n * h * w * c * es
            c_in, k = c, k + 1
        feat = torch.randn(2 * n, h, w, c, device="cuda").to(dtype)
        stat_jobs.append((feat, taps[l + 1][3]))
        stat_bytes += 2 * n * h * w * c * es + n * ops.dists_stat_slots(h, w, c) * 5 * c * 8
        if l < 4:
            pool_jobs.append(feat)
            pool_bytes += 2 * n * h * w * c * es + 2 * n * ((h + 1) // 2) * ((w + 1) // 2) * c * es
        h, w = (h + 1) // 2, (w + 1) // 2
    t_conv = median_us(lambda i: [ops.conv2d(x, pw, b) for x, pw, b in conv_jobs], 6)
    t_relu = median_us(lambda i: [ops.lpips_relu(x) for x in relu_jobs], 10)

    def stats(i):
        ops.dists_stats(sets[i % 3][0], ws, taps[0][3], stride, feat_b=sets[i % 3][1])
        for f, off in stat_jobs:
            ops.dists_stats(f, ws, off, stride)
    t_stat = median_us(stats, 10)
    t_pool = median_us(lambda i: [ops.dists_l2pool(f) for f in pool_jobs], 10)
    t_fold = median_us(lambda i: ops.dists_fold(ws, n, res, res, alpha, beta, out), 20)
    del conv_jobs, relu_jobs, stat_jobs, pool_jobs
    t_all = median_us(lambda i: model(*sets[i % 3], dtype=dtype, out=out, ws=ws), 6)
    r = {"convs_us": round(t_conv, 1), "conv_flops": flops, "conv_achieved_TFLOPs": round(flops / t_conv / 1e6, 1),
         "relu_us_8_launches": round(t_relu, 1), "relu_bytes": relu_bytes, "relu_at_hbm_rate_us": round(relu_bytes / HBM * 1e6, 1),
         "stats_us_6_launches": round(t_stat, 1), "stats_bytes": stat_bytes, "stats_at_hbm_rate_us": round(stat_bytes / HBM * 1e6, 1),
         "l2pool_us_4_launches": round(t_pool, 1), "l2pool_bytes": pool_bytes, "l2pool_at_hbm_rate_us": round(pool_bytes / HBM * 1e6, 1),
         "fold_us": round(t_fold, 1), "fold_bytes": n * stride * 8, "fold_at_hbm_rate_us": round(n * stride * 8 / HBM * 1e6, 1),
         "end_to_end_us": round(t_all, 1)}
    if name in CONV_RATE:
        r["convs_at_measured_conv_rate_us"] = round(flops / CONV_RATE[name] * 1e6, 1)
    rec[name] = r
mws = torch.empty(ops.image_metrics_workspace_bytes(n, 3, res, res), dtype=torch.uint8, device="cuda")
mout = (torch.empty(n, device="cuda"), torch.empty(n, device="cuda"))
rec["psnr_ssim_launch_us"] = round(median_us(lambda i: ops.image_metrics(*sets[i % 3], out=mout, ws=mws), 60), 1)
print(json.dumps(rec))
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(rec, f, indent=1)
