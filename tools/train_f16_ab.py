"""Training-step time of the three precision modes at the BASELINE.json configs[3] shape on one GPU (GPU):
bf16, f16 under the dynamic loss scaler (`16-mixed`), f16 with `GradScalerCfg(enabled=False)` -- the last isolates the scaler's own
cost.  One optimizer step = one `training_window` (2 micro-batches of B scenes x (1 ctx + 3 tgt) views @ 256x256, next window
encoded ahead as in bench.py --train).  Same process, same box, one trainer at a time, each from the same random initialisation;
the modes run in the order A B C C B A and the faster pass of each is reported.
    python tools/train_f16_ab.py [scenes=4] [steps=10] [warmup=3]
Prints one line per pass and mode (views/s, ms per optimizer step, loss scale and skipped steps at the end), then the best of each."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
import mv_ldm_amd
from mv_ldm_amd.mvunet import MultiViewUNet, MultiViewUNetCfg
from mv_ldm_amd.scheduler import DDIMScheduler
from mv_ldm_amd.train import GradScalerCfg, MVLDMTrainer, TrainCfg
from mv_ldm_amd.vae import AutoencoderKL

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 3
torch.set_grad_enabled(False)
dev = torch.device("cuda", 0)
with torch.device(dev):
    den = MultiViewUNet(MultiViewUNetCfg(pretrained_from="stabilityai/stable-diffusion-2-1", allow_random_init=True), 11, 4)
    vae = AutoencoderKL.from_pretrained("stabilityai/stable-diffusion-2-1", allow_random_init=True)
bench.random_init_(den, 1234)
bench.random_init_(vae, 1235)
batch = bench.synthetic_batch(B, 1, 3, 256, 4000, dev)
batch["target"]["image"] = torch.rand(B, 3, 3, 256, 256, generator=torch.Generator().manual_seed(77)).to(dev)
ch = dict(index=1, unconditional=False)
modes = [("bf16", torch.bfloat16, GradScalerCfg()), ("f16 + scaler", torch.float16, GradScalerCfg()),
         ("f16, scaler off", torch.float16, GradScalerCfg(enabled=False))]
best = {}
for name, dtype, sc in modes + modes[::-1]:
    bench.random_init_(den, 1234)
    torch.manual_seed(1234)
    mv_ldm_amd.set_compute_dtype(dtype)
    tr = MVLDMTrainer(den, vae, DDIMScheduler(clip_sample=False), dtype=dtype, train_cfg=TrainCfg(grad_scaler=sc))
    acc = tr.cfg.accumulate_grad_batches
    win_b, win_c = [batch] * acc, [ch] * acc
    for _ in range(warmup):
        tr.training_window(win_b, win_c, prefetch=(win_b, win_c))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        losses = tr.training_window(win_b, win_c, prefetch=(win_b, win_c))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    extra = "" if tr.grad_scale is None else f"  scale {float(tr.grad_scale):g}  skipped {int(tr.skipped_steps)}"
    print(f"{name:16s} {B * 4 * acc * steps / dt:8.2f} views/s  {1e3 * dt / steps:8.1f} ms/step  loss {float(losses.mean()):.4f}{extra}", flush=True)
    best[name] = min(best.get(name, dt), dt)
    tr._take_prefetched(())
    del tr, losses
    torch.cuda.empty_cache()
for name, _, _ in modes:
    print(f"best {name:16s} {B * 4 * 2 * steps / best[name]:8.2f} views/s  {1e3 * best[name] / steps:8.1f} ms/step", flush=True)
