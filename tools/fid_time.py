"""time FID on the device (mv_ldm_amd/fid.py, csrc/fid.hip) on scenes of 4 and of 64 views at the sampler's output shape, in f32 and f16:
    python tools/fid_time.py [res=256] [--json OUT]
  * the four kernels alone -- prep (quantise + resize to 299 x 299), pool (ReLU + max-pool + sum, fp64), accumulate (fold + state) and
    compute (the two 64 x 64 Jacobi solves, one workgroup) -- prep and pool also against the bytes they move at 5 TB/s (the streaming
    figure of DESIGN.md §3.5);
  * the three convs of the stem against their FLOPs (the achieved rate alone: profiles/ holds no rate for these thin layers);
  * the whole `metrics.compute_fid` of a scene: update(real), update(fake), compute(), reset().
Random weights (timing does not depend on them; the solves run on the states of random images, rank-deficient at 4 views as a scene is).
Every figure is the median of 5 windows of back-to-back calls between device events, after a warm-up of every shape; inputs rotate over
3 buffer sets."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mv_ldm_amd import metrics, ops
from mv_ldm_amd.fid import FEATURES, LAYERS, MAP, SIZE, FrechetInceptionDistance

args = [a for a in sys.argv[1:] if a.isdigit()]
res = int(args[0]) if args else 256
HBM = 5.0e12


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


rec = {"res": res, "hbm_rate_assumed_TBps": HBM / 1e12, "note": "median of 5 windows of back-to-back calls between device events; 3 rotating input sets"}
for views in (4, 64):
    sets = [(torch.rand(views, 3, res, res, device="cuda"), torch.rand(views, 3, res, res, device="cuda")) for _ in range(3)]
    for dtype in (torch.float32, torch.float16):
        name = str(dtype).split(".")[-1]
        es = 4 if dtype == torch.float32 else 2
        model = FrechetInceptionDistance(dtype=dtype, allow_random_init=True).cuda()
        packs = model._packed(dtype)
        ws = torch.empty(model.workspace_bytes(views), dtype=torch.uint8, device="cuda")
        # the operands of every launch, as update() makes them
        x = ops.fid_prep(sets[0][0], dtype, SIZE, SIZE)
        conv_jobs, flops, edge = [], 0, SIZE
        for layer, c_in, c_out, _, stride, (pad, _) in LAYERS:           # three 3 x 3 kernels with square padding
            conv_jobs.append((x, *packs[layer], stride, pad))
            x = ops.conv2d(x, *packs[layer], stride=stride, pad=pad)
            edge = x.shape[1]
            flops += 2 * views * edge * edge * 9 * c_in * c_out
        assert edge == MAP
        feat = x
        t_prep = median_us(lambda i: ops.fid_prep(sets[i % 3][0], dtype, SIZE, SIZE), 20)
        t_conv = median_us(lambda i: [ops.conv2d(a, pw, b, stride=s, pad=p) for a, pw, b, s, p in conv_jobs], 10)
        t_pool = median_us(lambda i: ops.fid_pool(feat, ws), 20)
        state = torch.zeros(ops.FID_STATE, dtype=torch.float64, device="cuda")
        t_acc = median_us(lambda i: ops.fid_accumulate(ws, views, MAP, MAP, FEATURES, state), 20)
        model.reset()
        model.update(sets[0][0], real=True, ws=ws)
        model.update(sets[0][1], real=False, ws=ws)
        out = torch.empty((), device="cuda")
        t_comp = median_us(lambda i: model.compute(out=out), 5)
        info = model.info.tolist()
        t_all = median_us(lambda i: metrics.compute_fid(sets[i % 3][0], sets[i % 3][1], model), 4)
        prep_bytes = views * 3 * res * res * 4 + views * SIZE * SIZE * ops.epc(dtype) * es
        pool_bytes = views * MAP * MAP * FEATURES * es
        rec[f"{views}_views/{name}"] = {
            "prep_us": round(t_prep, 1), "prep_bytes": prep_bytes, "prep_at_hbm_rate_us": round(prep_bytes / HBM * 1e6, 1),
            "convs_us": round(t_conv, 1), "conv_flops": flops, "conv_achieved_TFLOPs": round(flops / t_conv / 1e6, 1),
            "pool_us": round(t_pool, 1), "pool_bytes": pool_bytes, "pool_at_hbm_rate_us": round(pool_bytes / HBM * 1e6, 1),
            "accumulate_us": round(t_acc, 1), "compute_us": round(t_comp, 1), "compute_sweeps": [int(info[0]), int(info[2])],
            "compute_fid_end_to_end_us": round(t_all, 1)}
        del conv_jobs, feat, x
print(json.dumps(rec))
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(rec, f, indent=1)
