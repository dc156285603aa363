"""CPU: f16 dynamic loss scaling of the training path (`GradScalerCfg`, DistributedOptimizer's scaler) against torch's own
`torch.amp.GradScaler` under Lightning's automatic optimisation (`16-mixed`): scale / growth tracker / skip decisions, AdamW's step
count, the weights, the LR schedule; the ZeRO-1 skip on gloo world 2; the `GradScaler.state_dict()` round trip.  The scaler's four
device operations are injected in torch form (tests/torch_optimizer_ops.py: the arithmetic of the HIP kernels in train_misc.hip)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from torch_optimizer_ops import TorchOptimizerOps

GRAD_ENABLED = True       # tests/conftest.py::_grad_mode: the torch reference runs scaler.scale(loss).backward()


def _model():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(13, 24), torch.nn.LayerNorm(24), torch.nn.Linear(24, 7, bias=False))
    m.pretrained_from = None
    return m


def _scripted_grad(step, shape_numel, rank=0):
    g = torch.randn(shape_numel, generator=torch.Generator().manual_seed(1000 * step + rank)) * 0.05
    return g


BAD = {2: float("inf"), 5: float("nan"), 6: float("-inf")}       # step -> value put into one gradient entry


def _make_opt(model, world=1, rank=0, **scaler_kw):
    from mv_ldm_amd.train import DistributedOptimizer, GradScalerCfg, OptimizerCfg, _flat_padded
    flat = _flat_padded(model, world)
    sched = {"name": "LinearLR", "kwargs": {"start_factor": 0.5, "total_iters": 4}}
    opt = DistributedOptimizer(flat, OptimizerCfg(lr=1e-2, scheduler=sched), world, rank, bucket_bytes=256, max_norm=0.1,
                               scaler=GradScalerCfg(**scaler_kw), ops=TorchOptimizerOps())
    return flat, opt


def test_scaler_config_defaults_are_torchs_and_only_f16_scales():
    from mv_ldm_amd.train import GradScalerCfg, TrainCfg, training_precision
    ref = torch.amp.GradScaler("cpu")
    cfg = GradScalerCfg()
    assert cfg.enabled and cfg.init_scale == ref.get_scale() and cfg.growth_factor == ref.get_growth_factor()
    assert cfg.backoff_factor == ref.get_backoff_factor() and cfg.growth_interval == ref.get_growth_interval()
    assert TrainCfg().grad_scaler == cfg
    assert training_precision("16-mixed") == (torch.float16, True)
    assert training_precision("16") == (torch.float16, True)
    assert training_precision("bf16-mixed") == (torch.bfloat16, False)
    assert training_precision("32-true") == (torch.float32, False)
    assert training_precision(None) == (torch.float32, False)
    with pytest.raises(ValueError):
        training_precision("64-true")


def test_scaler_state_machine_matches_torch_grad_scaler():
    """Lightning `16-mixed` automatic optimisation, step by step: scaler.scale(loss).backward(), scaler.unscale_(opt),
    clip_grad_norm_(0.1), scaler.step(opt), scaler.update(), lr_scheduler.step() -- against the sharded optimizer's scaler (world 1),
    with inf / NaN gradients at fixed steps and growth_interval 2 (the scale grows AND backs off within the run)"""
    from mv_ldm_amd.train import linear_lr_factor
    ref_model, model = _model(), _model()
    flat, opt = _make_opt(model, init_scale=2.0 ** 10, growth_interval=2)
    params = list(ref_model.parameters())
    topt = torch.optim.AdamW(params, lr=1e-2)
    tsch = torch.optim.lr_scheduler.LinearLR(topt, start_factor=0.5, total_iters=4)
    scaler = torch.amp.GradScaler("cpu", init_scale=2.0 ** 10, growth_interval=2)
    n_real = sum(p.numel() for p in params)
    skipped = 0
    for step in range(9):
        gr = _scripted_grad(step, n_real)
        if step in BAD:
            gr[3 + step] = BAD[step]
        # torch: the scripted gradient as d/dp of sum(p * G), scaled by the scaler's backward
        topt.zero_grad()
        off, loss = 0, 0.0
        for p in params:
            loss = loss + (p * gr[off:off + p.numel()].view(p.shape)).sum()
            off += p.numel()
        scaler.scale(loss).backward()
        scaler.unscale_(topt)
        torch.nn.utils.clip_grad_norm_(params, 0.1)
        scaler.step(topt)
        scaler.update()
        tsch.step()
        # ours: the flat gradient holds S x g, as the f16 backward leaves it
        s_before = float(opt.grad_scale)
        w0, m0, v0 = flat.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
        flat.grad.zero_()
        off = 0
        for q in flat.params:
            o = flat.offset[id(q)]
            flat.grad[o:o + q.numel()] = gr[off:off + q.numel()] * torch.tensor(s_before, dtype=torch.float32)
            off += q.numel()
        opt.step()
        skipped += step in BAD
        assert opt.scaler_state_dict() == scaler.state_dict(), (step, opt.scaler_state_dict(), scaler.state_dict())
        t_step = int(topt.state[params[0]]["step"]) if topt.state.get(params[0]) else 0
        assert opt.adam_step == t_step == step + 1 - skipped, (step, opt.adam_step, t_step)
        assert int(opt.skipped_steps) == skipped
        assert opt.step_count == step + 1                                          # the LR schedule advances on a skipped step too
        assert abs(opt.lr() - tsch.get_last_lr()[0]) < 1e-12 and opt.lr() == pytest.approx(1e-2 * linear_lr_factor(step + 1, 0.5, 1.0, 4))
        if step in BAD:                                                              # skipped: masters and moments bit-identical
            assert torch.equal(flat.flat, w0) and torch.equal(opt.exp_avg, m0) and torch.equal(opt.exp_avg_sq, v0), step
        else:
            assert not torch.equal(flat.flat, w0), step
        got = torch.cat([q.detach().reshape(-1) for q in model.parameters()])
        want = torch.cat([q.detach().reshape(-1) for q in params])
        assert (got - want).abs().max() < 2e-6, (step, float((got - want).abs().max()))
    assert skipped == len(BAD)


def _ddp_amp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        model = _model()
        flat, opt = _make_opt(model, world, rank, init_scale=2.0 ** 8, growth_interval=2)
        first = opt.buckets[0]
        res = []
        for step in range(4):
            g = _scripted_grad(step, flat.numel, rank) * float(opt.grad_scale)
            if step == 1 and rank == 1:
                g[first[0]] = float("inf")          # only rank 1's gradient, in the slice rank 0 owns: rank 1's own sum stays finite
            mask = torch.zeros(flat.numel)
            for p_ in flat.params:
                mask[flat.offset[id(p_)]:flat.offset[id(p_)] + p_.numel()] = 1.0
            flat.grad.copy_(torch.where(mask > 0, g, torch.zeros_like(g)))
            for k in reversed(range(len(opt.buckets))):
                opt.reduce_bucket(k)
            w0 = flat.flat.clone()
            opt.step()
            res.append((opt.scaler_state_dict(), opt.adam_step, int(opt.skipped_steps), bool(torch.equal(flat.flat, w0))))
        q.put((rank, res, flat.flat.numpy().copy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_an_inf_on_one_rank_makes_every_rank_skip_world2():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_ddp_amp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=180) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, r0, w0), (_, r1, w1) = got
    assert r0 == r1, (r0, r1)                       # same scale, tracker, step count, skips, decisions on both ranks
    assert [unchanged for *_, unchanged in r0] == [False, True, False, False]
    assert r0[1][0]["scale"] == 2.0 ** 7 and r0[1][2] == 1 and r0[1][0]["_growth_tracker"] == 0
    assert r0[-1][0]["scale"] == 2.0 ** 8 and r0[-1][1] == 3
    assert np.array_equal(w0, w1)


def test_scaler_state_dict_round_trip_reproduces_the_following_steps():
    """GradScaler.state_dict() layout out of one optimizer, into a fresh one (with the weights, moments, AdamW's step count and the
    schedule position a full resume carries): the next steps -- including a skip and a growth -- are bit-identical"""
    model_a, model_b = _model(), _model()
    flat_a, a = _make_opt(model_a, init_scale=2.0 ** 12, growth_interval=3, growth_factor=4.0, backoff_factor=0.25)
    flat_b, b = _make_opt(model_b, init_scale=1.0, growth_interval=2000)

    def step(flat, opt, k):
        g = _scripted_grad(k, flat.numel) * float(opt.grad_scale)
        if k == 4:
            g[5] = float("nan")
        flat.grad.copy_(g)
        opt.step()

    for k in range(4):          # one skip-free run of 4 steps: tracker 1 after the growth at step 3
        step(flat_a, a, k)
    sd = a.scaler_state_dict()
    assert sd["_growth_tracker"] == 1 and sd["scale"] == 2.0 ** 14 and sd["growth_factor"] == 4.0 and sd["growth_interval"] == 3
    b.load_scaler_state_dict(sd)
    assert b.scaler_state_dict() == sd
    flat_b.flat.copy_(flat_a.flat)
    b.exp_avg.copy_(a.exp_avg)
    b.exp_avg_sq.copy_(a.exp_avg_sq)
    b.adam_step, b.step_count = a.adam_step, a.step_count
    for k in range(4, 9):
        step(flat_a, a, k)
        step(flat_b, b, k)
        assert a.scaler_state_dict() == b.scaler_state_dict(), k
        assert torch.equal(flat_a.flat, flat_b.flat) and torch.equal(a.exp_avg_sq, b.exp_avg_sq), k
    assert int(a.skipped_steps) == 1 and int(b.skipped_steps) == 1 and a.adam_step == b.adam_step == 8


def test_scaler_is_off_for_bf16_and_f32_and_for_a_disabled_config():
    from mv_ldm_amd.train import DistributedOptimizer, GradScalerCfg, _flat_padded
    flat = _flat_padded(_model(), 1)
    opt = DistributedOptimizer(flat, scaler=GradScalerCfg(enabled=False))
    assert opt.amp_state is None and opt.grad_scale is None and opt.scaler_state_dict() == {}
    opt.load_scaler_state_dict({"scale": 2.0})                 # a disabled scaler ignores it, like torch's
    assert opt.adam_step == opt.step_count == 0
