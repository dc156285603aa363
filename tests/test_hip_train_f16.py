"""GPU: f16 training with dynamic loss scaling (`16-mixed`, the reference's trainer.precision: baseline.yaml:60) on the HIP path --
the f16 forms of every training kernel (data gradients through the forward implicit GEMM on transposed packs, weight gradients,
attention / norm backward, the elementwise and column-sum kernels) and the device-resident scaler (mvldm_amp_state).

Tolerances of the G9 parity: 2 x the maxima measured on MI355X (tests/golden/measured_errors_f16.json), each no looser than the bf16
bound of the same quantity (tests/test_hip_train.py): loss 4.1e-4 (measured 2.0e-4), worst parameter-gradient norm 3.5e-3 (1.7e-3),
global gradient norm 1.4e-3 (7.0e-4), sampled gradient entries 6.5e-3 (3.1e-3)."""
import socket

import numpy as np
import pytest
import torch

from conftest import record_err
from test_hip_train import build_trainer, hip_choices
from test_oracle_train import g9_case

GRAD_ENABLED = True
pytestmark = pytest.mark.gpu

# bf16 bounds of tests/test_hip_train.py, and the f16 ones (2 x measured_errors_f16.json)
BF16 = dict(loss=1.3e-3, worst=3e-2, glob=8e-3, sampled=5.5e-2)
F16 = dict(loss=4.1e-4, worst=3.5e-3, glob=1.4e-3, sampled=6.5e-3)


def _window(tr, cis=(0, 2), g=None):
    cases = [g9_case(g, ci) for ci in cis]
    return tr.training_window([c[0] for c in cases], [hip_choices(c[1]) for c in cases])


def test_f16_bounds_are_no_looser_than_bf16():
    assert all(F16[k] <= BF16[k] for k in BF16)


def test_f16_training_step_vs_reference_golden(golden):
    """the loss and the gradients (divided by the loss scale S) of one f16 micro-batch against the REFERENCE's own training_step +
    autograd (G9), per case"""
    g = golden("g9_training_step")
    names = [str(n) for n in g["names"]]
    tr = build_trainer(g, torch.float16)
    assert tr.grad_scale is not None and float(tr.grad_scale) == 2.0 ** 16
    own = dict(tr.denoiser.named_parameters())
    in_flat = {id(q) for q in tr.flat.params}
    for ci in range(int(g["n"])):
        p = f"c{ci}_"
        batch, ch = g9_case(g, ci)
        tr.micro = 0
        loss = float(tr.training_step(batch, **hip_choices(ch)))        # accumulate_grad_batches 2: no optimizer step, raw gradients x 1/2
        torch.cuda.synchronize()
        s = float(tr.grad_scale)
        assert s == 2.0 ** 16 and bool(torch.isfinite(tr.flat.grad).all())
        ref_loss = float(g[p + "loss"])
        e = record_err("g9_loss/float16", abs(loss - ref_loss) / ref_loss)
        assert e < F16["loss"], (ci, loss, ref_loss)
        want = dict(zip(names, g[p + "grad_norms"]))
        worst, tot_got, tot_ref = 0.0, 0.0, 0.0
        for n, prm in own.items():
            if want[n] < 0:
                assert id(prm) not in in_flat, n
                continue
            gn = 2.0 * float(prm.grad.double().norm()) / s
            tot_got, tot_ref = tot_got + gn * gn, tot_ref + want[n] ** 2
            if want[n] == 0:
                assert gn == 0.0, n
            else:
                worst = max(worst, abs(gn - want[n]) / want[n])
        record_err("g9_worst_param_grad_norm/float16", worst)
        e_glob = record_err("g9_global_grad_norm/float16", abs(tot_got ** 0.5 - tot_ref ** 0.5) / tot_ref ** 0.5)
        assert worst < F16["worst"], (ci, worst)
        assert e_glob < F16["glob"], (ci, e_glob)
        for k in g.files:
            if k.startswith(p + "grad/"):
                got = 2.0 * own[k[len(p) + 5:]].grad.reshape(-1).float().cpu() / s
                got = got[::max(1, got.numel() // 2048)][:2048]
                ref = torch.from_numpy(g[k])
                e = record_err("g9_sampled_grad/float16", float((got - ref).norm() / ref.norm().clamp_min(1e-30)))
                assert e < F16["sampled"], (k, e)


def test_f16_gradients_drift_less_than_bf16_at_full_width():
    """configs[3]-shaped micro-batch at full width (the inputs of test_bf16_gradients_against_the_f32_hip_path_at_full_width): the
    f16 gradients (unscaled) against the f32 HIP plan drift less than the bf16 ones, and stay under a stated bound.  The noise and
    timestep draws are not pinned (they follow the process's RNG state), so the bounds are ~3x the largest of the measured runs:
    global relative L2 6e-3 (measured 1.8e-3 / 2.2e-3; bf16 1.5e-2 .. 1.7e-2), worst large parameter 1.2e-2 (3.1e-3 / 3.8e-3;
    bf16 2.7e-2), norm ratio 2e-3 (1.3e-4 / 4.5e-4), loss 1e-3 (2.7e-5 / 1.2e-4)"""
    import bench
    import mv_ldm_amd
    from mv_ldm_amd.mvunet import MultiViewUNet, MultiViewUNetCfg
    from mv_ldm_amd.scheduler import DDIMScheduler
    from mv_ldm_amd.train import MVLDMTrainer, gradient_drift_vs_f32
    from mv_ldm_amd.vae import AutoencoderKL
    with torch.device("cuda"):
        den = MultiViewUNet(MultiViewUNetCfg(pretrained_from="stabilityai/stable-diffusion-2-1", allow_random_init=True), 11, 4)
        vae = AutoencoderKL.from_pretrained("stabilityai/stable-diffusion-2-1", allow_random_init=True)
    bench.random_init_(den, 1234)
    bench.random_init_(vae, 1235)
    b = 4
    batch = bench.synthetic_batch(b, 1, 3, 256, 4000, torch.device("cuda"))
    batch["target"]["image"] = torch.rand(b, 3, 3, 256, 256, generator=torch.Generator().manual_seed(77)).cuda()
    r = {}
    for dtype in (torch.bfloat16, torch.float16):
        mv_ldm_amd.set_compute_dtype(dtype)
        tr = MVLDMTrainer(den, vae, DDIMScheduler(clip_sample=False), dtype=dtype)
        r[dtype] = gradient_drift_vs_f32(tr, batch, index=1, unconditional=False)
        print(r[dtype])
        del tr
        torch.cuda.empty_cache()
    lo, bf = r[torch.float16], r[torch.bfloat16]
    record_err("full_width_grad_rel_l2/float16", lo["grad_rel_l2"])
    record_err("full_width_worst_large_param_rel_l2/float16", lo["worst_large_param_rel_l2"])
    assert lo["grad_rel_l2"] < bf["grad_rel_l2"] and lo["worst_large_param_rel_l2"] < bf["worst_large_param_rel_l2"], (lo, bf)
    assert lo["grad_rel_l2"] < 6e-3 and lo["worst_large_param_rel_l2"] < 1.2e-2, lo
    assert abs(lo["grad_norm_ratio"] - 1.0) < 2e-3 and lo["loss_rel"] < 1e-3, lo


def _overflow_run(g, **kw):
    from mv_ldm_amd.train import GradScalerCfg, OptimizerCfg, TrainCfg, linear_lr_factor
    sc = GradScalerCfg(init_scale=2.0 ** 60, backoff_factor=2.0 ** -44)
    tr = build_trainer(g, torch.float16, optimizer_cfg=OptimizerCfg(lr=1e-3), train_cfg=TrainCfg(grad_scaler=sc), **kw)
    w0, m0, v0 = tr.flat.flat.clone(), tr.opt.exp_avg.clone(), tr.opt.exp_avg_sq.clone()
    losses = _window(tr, g=g)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses).all()), losses                     # the loss itself is unscaled
    assert not bool(torch.isfinite(tr.flat.grad).all())                   # 2^60 x dY overflowed f16, and the overflow reached the gradient
    assert torch.equal(tr.flat.flat, w0) and torch.equal(tr.opt.exp_avg, m0) and torch.equal(tr.opt.exp_avg_sq, v0)
    assert int(tr.skipped_steps) == 1 and tr.adam_step == 0 and float(tr.grad_scale) == 2.0 ** 16
    assert tr.global_step == 1 and tr.opt.step_count == 1                 # the LR schedule and global_step advance on the skip
    sch = tr.opt.sched["kwargs"]
    assert tr.opt.lr() == pytest.approx(1e-3 * linear_lr_factor(1, **sch)) and tr.opt.lr() != tr.opt.lr0 * linear_lr_factor(0, **sch)
    _window(tr, g=g)                                                      # S = 2^16: a normal step
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.flat.grad).all()) and bool(torch.isfinite(tr.flat.flat).all())
    assert int(tr.skipped_steps) == 1 and tr.adam_step == 1 and tr.global_step == 2 and tr.opt.step_count == 2
    assert not torch.equal(tr.flat.flat, w0) and float(tr.grad_scale) == 2.0 ** 16
    sd = tr.scaler_state_dict()
    assert sd["scale"] == 2.0 ** 16 and sd["_growth_tracker"] == 1 and sd["backoff_factor"] == 2.0 ** -44
    return tr


@pytest.mark.parametrize("collective", [False, True], ids=["plain", "nccl1"])
def test_forced_overflow_skips_the_step_and_backs_off(golden, collective, monkeypatch):
    """init_scale 2^60: window 1's scaled loss gradient overflows f16 -> skipped step (masters, moments, AdamW's step count
    bit-identical), S backs off to 2^16, LR schedule / global_step advance; window 2 takes a normal step.  Also under the RCCL branch
    (1-rank nccl group, collective=True: the found-inf decision from the all-reduced sum of squares)"""
    g = golden("g9_training_step")
    if not collective:
        _overflow_run(g)
        return
    import torch.distributed as dist
    monkeypatch.setenv("MVLDM_TRAIN_AUTOTUNE", "0")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    assert not dist.is_initialized()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        tr = _overflow_run(g, bucket_bytes=2 << 20, group=dist.group.WORLD, collective=True)
        assert tr.opt.collective and len(tr.opt.buckets) > 8
        del tr
    finally:
        dist.destroy_process_group()


def test_recorded_plans_read_the_scale_at_run_time(golden, monkeypatch):
    """trainer A (growth_interval 1) doubles S after window 1; trainer C is fresh, starts at A's new S and holds A's post-window-1
    weights: window 2's flat gradient is bit-identical in both -- A's plan, recorded when S was half as large, kept no stale S"""
    from mv_ldm_amd.train import GradScalerCfg, OptimizerCfg, TrainCfg
    monkeypatch.setenv("MVLDM_TRAIN_AUTOTUNE", "0")
    monkeypatch.setenv("MVLDM_AUTOTUNE", "0")
    g = golden("g9_training_step")
    a = build_trainer(g, torch.float16, optimizer_cfg=OptimizerCfg(lr=1e-3), train_cfg=TrainCfg(grad_scaler=GradScalerCfg(growth_interval=1)))
    _window(a, g=g)
    torch.cuda.synchronize()
    assert float(a.grad_scale) == 2.0 ** 17 and int(a.skipped_steps) == 0
    c = build_trainer(g, torch.float16, optimizer_cfg=OptimizerCfg(lr=1e-3),
                      train_cfg=TrainCfg(grad_scaler=GradScalerCfg(init_scale=2.0 ** 17, growth_interval=1)))
    c.load_denoiser_state_dict(a.denoiser.state_dict())
    assert torch.equal(c.flat.flat, a.flat.flat)
    la, lc = _window(a, g=g), _window(c, g=g)
    torch.cuda.synchronize()
    assert torch.equal(la, lc), (la, lc)
    assert bool(torch.isfinite(a.flat.grad).all()) and torch.equal(a.flat.grad, c.flat.grad), float((a.flat.grad - c.flat.grad).abs().max())


def test_f16_windows_follow_the_f32_trainer(golden):
    """three accumulation windows + AdamW steps (lr 1e-3, clip 0.1) in f16 under the scaler against the f32 HIP trainer from the same
    weights and inputs: relative L2 of the weight change within 1e-2 (measured 4.0e-3; AdamW normalises tiny gradients, so 1/sqrt(v)
    amplifies the f16 rounding where gradients are near zero), no skipped step"""
    from mv_ldm_amd.train import OptimizerCfg
    g = golden("g9_training_step")
    got = {}
    for dtype in (torch.float32, torch.float16):
        tr = build_trainer(g, dtype, optimizer_cfg=OptimizerCfg(lr=1e-3))
        w0 = tr.flat.flat.clone()
        for k in range(3):
            _window(tr, (0, 2) if k % 2 == 0 else (1, 0), g=g)
        torch.cuda.synchronize()
        got[dtype] = (tr.flat.flat - w0).double().cpu()
        if dtype == torch.float16:
            assert int(tr.skipped_steps) == 0 and tr.adam_step == 3 and tr.global_step == 3
        del tr
    d32, d16 = got[torch.float32], got[torch.float16]
    e = record_err("multi_window_weight_delta_vs_f32/float16", float((d16 - d32).norm() / d32.norm()))
    assert float(d32.norm()) > 0 and e < 1e-2, e
