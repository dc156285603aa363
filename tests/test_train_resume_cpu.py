"""CPU: saving and restoring the full trainer state (`DistributedOptimizer.state_dict / load_state_dict`, `MVLDMTrainer.state_dict /
load_state_dict / save_checkpoint / load_checkpoint`) -- the ZeRO-1 shards consolidated into `torch.optim.AdamW.state_dict()`'s layout
inside the container Lightning writes for the reference, resharded on load to any world size and bucket size.

The toy model, the scripted gradients, the torch stand-in for the four optimizer kernels and the spawn / gloo pattern are those of
tests/test_dist_gloo.py; the trainer is a real `MVLDMTrainer` around the toy model whose optimizer steps are driven by hand (there is
no CPU forward / backward).  Everything is compared with `torch.equal` except where two WORLD SIZES continue the same run: those differ
in the summation order of the gradient norm, and hold the 2e-6 of test_sharded_optimizer_equals_single_process_adamw_world2."""
import os
import socket
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from torch_optimizer_ops import TorchOptimizerOps

SCHED = {"name": "LinearLR", "kwargs": {"start_factor": 0.5, "total_iters": 4}}
N_GRAD = 8192          # the scripted gradient is drawn at one fixed length: the same values per parameter whatever the tail padding


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _toy_model():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(37, 64), torch.nn.Linear(64, 51, bias=False), torch.nn.LayerNorm(51), torch.nn.Linear(51, 10))
    m.pretrained_from = None
    return m


def _grad_mask(flat):
    m = torch.zeros(flat.numel)
    for q in flat.params:
        m[flat.offset[id(q)]:flat.offset[id(q)] + q.numel()] = 1.0
    return m


def _grad(flat, step, ranks):
    """the gradient of `step`, summed over `ranks` (a sharded rank passes its own; a smaller world passes all it stands for)"""
    assert flat.numel <= N_GRAD
    tot = sum(torch.randn(N_GRAD, generator=torch.Generator().manual_seed(100 * step + r)) * 0.01 for r in ranks)
    return tot[:flat.numel] * _grad_mask(flat)


def _trainer(world=1, rank=0, dtype=torch.float32, bucket_bytes=4096, scaler=None, ema_decay=None, sched=SCHED):
    from mv_ldm_amd.train import GradScalerCfg, MVLDMTrainer, OptimizerCfg, TrainCfg
    tr = MVLDMTrainer(_toy_model(), torch.nn.Module(), None, OptimizerCfg(lr=1e-2, scheduler=sched),
                      TrainCfg(gradient_clip_val=0.1, grad_scaler=scaler or GradScalerCfg()), dtype=dtype, world=world, rank=rank,
                      bucket_bytes=bucket_bytes, ema_decay=ema_decay)
    tr.opt._ops = TorchOptimizerOps()          # the four device operations of a step, in torch
    return tr


def _step(tr, step, ranks=None):
    """what `training_window` does around the plan, with the scripted gradient in place of the backward pass"""
    flat, opt = tr.flat, tr.opt
    g = _grad(flat, step, [tr.rank] if ranks is None else ranks)
    if opt.scaler is not None:                 # the f16 backward leaves S x g, through f16 activations: a huge S overflows to inf
        g = (g * float(opt.grad_scale)).to(torch.float16).float()
    flat.grad.copy_(g)
    for k in reversed(range(len(opt.buckets))):
        opt.reduce_bucket(k)
    tr.micro += tr.cfg.accumulate_grad_batches
    opt.step()
    tr.global_step += 1
    tr._weights_gen += 1


def _snapshot(tr):
    opt = tr.opt
    out = dict(flat=tr.flat.flat.clone().numpy(), m=opt.exp_avg.clone().numpy(), v=opt.exp_avg_sq.clone().numpy(), step_count=opt.step_count,
               adam_step=opt.adam_step, lr=opt.lr(), global_step=tr.global_step, owned=list(opt.owned))
    if opt.scaler is not None:
        out.update(scaler=tr.scaler_state_dict(), skipped=int(tr.skipped_steps))
    return out


def _init(rank, world, port):
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group("gloo", rank=rank, world_size=world)


def _done(world):
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _spawn(worker, world, *args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


def _eq(a, b):
    return torch.equal(torch.as_tensor(a), torch.as_tensor(b))


def _same(a, b, path=""):
    """two containers hold the same structure, the same tensors bit for bit and the same values"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (path, list(a)[:5], list(b)[:5])
        for k in a:
            _same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), path
    else:
        assert a == b, (path, a, b)


def _scaler_cfg(on):
    from mv_ldm_amd.train import GradScalerCfg
    return GradScalerCfg(init_scale=2.0 ** 60, backoff_factor=2.0 ** -44, growth_interval=3) if on else None


# ---- 1. same world: the resumed run is the straight run, bit for bit ---------------------------------------------------------------
def _straight_worker(rank, world, port, q, f16):
    _init(rank, world, port)
    tr = _trainer(world, rank, torch.float16 if f16 else torch.float32, scaler=_scaler_cfg(f16))
    for step in range(3):
        _step(tr, step)
    q.put((rank, _snapshot(tr)))
    _done(world)


def _save_worker(rank, world, port, q, f16, path):
    _init(rank, world, port)
    tr = _trainer(world, rank, torch.float16 if f16 else torch.float32, scaler=_scaler_cfg(f16))
    for step in range(2):
        _step(tr, step)
    tr.save_checkpoint(path)                   # every rank enters; rank 0 writes; the others wait at the barrier
    assert os.path.exists(path)
    q.put((rank, _snapshot(tr)))
    _done(world)


def _resume_worker(rank, world, port, q, f16, path):
    _init(rank, world, port)
    tr = _trainer(world, rank, torch.float16 if f16 else torch.float32, scaler=_scaler_cfg(f16))
    tr.load_checkpoint(path)
    loaded = _snapshot(tr)
    _step(tr, 2)
    q.put((rank, (loaded, _snapshot(tr))))
    _done(world)


@pytest.mark.parametrize("world,f16", [(2, False), (1, False), (2, True)], ids=["world2", "world1", "world2-scaler"])
def test_resumed_run_is_bit_identical_to_the_straight_run(tmp_path, world, f16):
    """three steps straight (LinearLR, clip 0.1) against two steps, a checkpoint file, FRESH processes / model / trainer, load, third
    step: masters, both moments, `step_count`, `adam_step`, `lr()` on every rank.  With the scaler, step 1 overflows (init scale 2^60
    through f16), so the scale, the growth tracker, the skipped-step count and `adam_step` (!= `step_count`) travel with non-trivial values."""
    path = str(tmp_path / "last.ckpt")
    want = _spawn(_straight_worker, world, f16)
    saved = _spawn(_save_worker, world, f16, path)
    got = _spawn(_resume_worker, world, f16, path)
    for rank in range(world):
        loaded, after = got[rank]
        for ref, new in ((saved[rank], loaded), (want[rank], after)):
            for k in ("flat", "m", "v"):
                assert _eq(ref[k], new[k]), (rank, k)
            for k in ("step_count", "adam_step", "lr", "global_step"):
                assert ref[k] == new[k], (rank, k, ref[k], new[k])
            if f16:
                assert ref["scaler"] == new["scaler"] and ref["skipped"] == new["skipped"], (ref["scaler"], new["scaler"])
        assert want[rank]["step_count"] == 3 and float(torch.as_tensor(want[rank]["m"]).abs().max()) > 0
        if f16:      # the overflow was skipped, the scale backed off, the growth tracker counts: nothing is at its initial value
            s = saved[rank]
            assert s["skipped"] == 1 and s["adam_step"] == 1 and s["step_count"] == 2
            assert s["scaler"]["scale"] == 2.0 ** 16 and s["scaler"]["_growth_tracker"] == 1 and s["scaler"]["backoff_factor"] == 2.0 ** -44
            assert want[rank]["adam_step"] == 2 and want[rank]["skipped"] == 1 and want[rank]["scaler"]["_growth_tracker"] == 2
        else:
            assert want[rank]["adam_step"] == 3
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert ckpt["global_step"] == 2 and ckpt["mv_ldm_amd"]["world"] == world and ("MixedPrecision" in ckpt) == f16
    assert ckpt["lr_schedulers"][0]["last_epoch"] == 2 and ckpt["lr_schedulers"][0]["_last_lr"] == [saved[0]["lr"]]


# ---- 2. resharding is pure data movement -------------------------------------------------------------------------------------------
def _reshard_worker(rank, world, port, q, src, dst, bucket_bytes):
    _init(rank, world, port)
    tr = _trainer(world, rank, bucket_bytes=bucket_bytes)
    if src is None:
        for step in range(2):
            _step(tr, step)
    else:
        tr.load_checkpoint(src)
    tr.save_checkpoint(dst)
    buckets = list(tr.opt.buckets)
    _step(tr, 2, ranks=[tr.rank] if world == 2 else [0, 1])
    tr.sync_masters()
    real = torch.cat([p.detach().reshape(-1) for p in tr.denoiser.parameters()])
    q.put((rank, (real.numpy(), buckets)))
    _done(world)


def test_resharding_to_another_world_or_bucket_size_only_moves_data(tmp_path):
    """world 2 / 4 KB buckets writes a file; world 1 and world 2 / 1 KB buckets load it and write it again: every tensor of the three
    files is the same, the param groups match; one more step from each agrees with the original world-2 continuation within 2e-6
    (the bound test_sharded_optimizer_equals_single_process_adamw_world2 holds for the same optimizer across world sizes)"""
    a, b1, b2 = (str(tmp_path / n) for n in ("a.ckpt", "b1.ckpt", "b2.ckpt"))
    base = _spawn(_reshard_worker, 2, None, a, 4096)
    one = _spawn(_reshard_worker, 1, a, b1, 4096)
    two = _spawn(_reshard_worker, 2, a, b2, 1024)
    assert base[0][1] != two[0][1] and len(two[0][1]) > len(base[0][1]) > 3          # really other shard boundaries
    ca, c1, c2 = (torch.load(f, map_location="cpu", weights_only=True) for f in (a, b1, b2))
    assert ca["mv_ldm_amd"].pop("world") == 2 and c1["mv_ldm_amd"].pop("world") == 1 and c2["mv_ldm_amd"].pop("world") == 2
    _same(ca, c1)
    _same(ca, c2)
    st = ca["optimizer_states"][0]["state"]
    assert len(st) == 7 and all(float(e["exp_avg"].abs().max()) > 0 and float(e["step"]) == 2.0 for e in st.values())
    ref = torch.as_tensor(base[0][0])
    assert _eq(ref, base[1][0])
    for other in (one[0][0], two[0][0], two[1][0]):
        err = float((torch.as_tensor(other) - ref).abs().max())
        assert err < 2e-6, err


# ---- 3. interop with torch.optim.AdamW, both directions ----------------------------------------------------------------------------
def _partial_flat(model):
    """the toy model with its second Linear never trained: torch keeps no state for it, `FlatParams` leaves it out"""
    from mv_ldm_amd.train import FlatParams
    return FlatParams(model, exclude=list(model[1].parameters()))


def _partial_opt(model):
    from mv_ldm_amd.train import DistributedOptimizer, OptimizerCfg
    flat = _partial_flat(model)
    return flat, DistributedOptimizer(flat, OptimizerCfg(lr=1e-2, scheduler=SCHED), bucket_bytes=4096, max_norm=0.1, ops=TorchOptimizerOps())


def test_torch_adamw_state_loads_here_and_ours_loads_into_torch_adamw():
    # forward: two steps of the real thing (clip_grad_norm_, LinearLR) -> our optimizer -> the third step of both
    ref_model = _toy_model()
    ref_flat = _partial_flat(ref_model)                     # (p.grad views for the trained parameters; None for the excluded one)
    params = list(ref_model.parameters())
    trained = [p for p in params if p.grad is not None]
    assert len(trained) == len(params) - 1
    topt = torch.optim.AdamW(params, lr=1e-2)
    tsch = torch.optim.lr_scheduler.LinearLR(topt, start_factor=0.5, total_iters=4)

    def torch_step(step):
        ref_flat.grad.copy_(_grad(ref_flat, step, [0]))
        torch.nn.utils.clip_grad_norm_(trained, 0.1)
        topt.step()
        tsch.step()
    for step in range(2):
        torch_step(step)
    tsd = topt.state_dict()
    assert sorted(tsd["state"]) == [0, 1, 3, 4, 5, 6]       # index 2 (the untrained weight) has no state
    model = _toy_model()
    flat, opt = _partial_opt(model)
    model.load_state_dict(ref_model.state_dict())
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # same hyper-parameters: nothing to warn about
        opt.load_state_dict(tsd)
        opt.load_lr_scheduler_state_dict(tsch.state_dict())
    assert opt.adam_step == opt.step_count == 2 and opt.lr() == pytest.approx(tsch.get_last_lr()[0], rel=1e-12)
    torch_step(2)
    flat.grad.copy_(_grad(flat, 2, [0]))
    opt.step()
    err = float((flat.flat - ref_flat.flat).abs().max())
    assert err < 2e-6 and float((flat.flat - _partial_flat(_toy_model()).flat).abs().max()) > 1e-3, err
    # reverse: our export -> a real AdamW over ALL the module's parameters; it steps, and holds our moments
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 3, 4, 5, 6] and sd["param_groups"][0]["params"] == list(range(7))
    assert set(sd["param_groups"][0]) == set(tsd["param_groups"][0])
    # it is the state torch itself would have written after the same three steps
    for i, e in topt.state_dict()["state"].items():
        assert torch.equal(e["step"], sd["state"][i]["step"]) and e["step"].dtype == sd["state"][i]["step"].dtype
        assert float((e["exp_avg"] - sd["state"][i]["exp_avg"]).abs().max()) < 2e-6
    other = torch.optim.AdamW(model.parameters(), lr=123.0)
    other.load_state_dict(sd)
    plist = list(model.parameters())
    for i, e in sd["state"].items():
        st = other.state[plist[i]]
        assert torch.equal(st["exp_avg"], e["exp_avg"]) and torch.equal(st["exp_avg_sq"], e["exp_avg_sq"]) and float(st["step"]) == 3.0
        assert e["exp_avg"].shape == plist[i].shape and e["exp_avg"].dtype == torch.float32 and e["step"].dim() == 0
    g = other.param_groups[0]
    assert g["lr"] == opt.lr() and g["initial_lr"] == 1e-2 and g["betas"] == (0.9, 0.999) and g["weight_decay"] == 1e-2
    before = flat.flat.clone()
    other.step()
    assert float(other.state[plist[0]]["step"]) == 4.0 and not torch.equal(before, flat.flat)


# ---- 4. exact masters under the 16-bit parameter gather ----------------------------------------------------------------------------
def _g16_worker(rank, world, port, q):
    _init(rank, world, port)
    out, cks, trs = {}, {}, {}
    for mode in ("fp32", "g16"):
        os.environ["MVLDM_TRAIN_GATHER16"] = "0" if mode == "fp32" else "1"
        tr = trs[mode] = _trainer(world, rank, torch.bfloat16)
        assert (tr.opt.gather_dtype is not None) == (mode == "g16")
        mid = None
        for step in range(3):
            _step(tr, step)
            if step == 1:
                mid = tr.state_dict()
        out[mode + "_raw"] = tr.flat.flat.clone().numpy()          # what a plain `denoiser.state_dict()` would read on this rank
        cks[mode] = (mid, tr.state_dict())
        assert tr.opt.masters_exact
    _same(cks["fp32"], cks["g16"])
    # rewind both to the step-2 checkpoint and take step 3 again: the 16-bit copy must have followed the load
    for mode in ("fp32", "g16"):
        tr = trs[mode]
        tr.load_state_dict(cks["fp32"][0])
        assert tr.opt.step_count == 2 and (tr.opt._p16 is None or torch.equal(tr.opt._p16, tr.flat.flat.bfloat16()))
        _step(tr, 2)
        out[mode + "_again"] = tr.flat.flat.clone().numpy()
        _same(tr.state_dict(), cks["fp32"][1])
    out["owned"] = list(trs["g16"].opt.owned)
    q.put((rank, out))
    _done(world)


def test_two_rank_checkpoint_under_the_16bit_gather_equals_the_fp32_gather_runs():
    """three world-2 steps with the bf16 parameter gather: the checkpoint (weights, moments, everything) equals, tensor for tensor, the
    one of the same run with the fp32 gather -- although a plain read of the flat masters on a non-owner differs (negative control).
    Loading a checkpoint into the live 16-bit-gather trainer and stepping gives the packs (`bfloat16()` of the masters) of the fp32 run."""
    got = _spawn(_g16_worker, 2)
    for rank in range(2):
        o = got[rank]
        ref, raw = torch.as_tensor(o["fp32_raw"]), torch.as_tensor(o["g16_raw"])
        assert not torch.equal(ref, raw)                                     # the test is sensitive: unsynced masters are rounded
        for oa, ob in o["owned"]:
            assert torch.equal(ref[oa:ob], raw[oa:ob])
        again32, again16 = torch.as_tensor(o["fp32_again"]), torch.as_tensor(o["g16_again"])
        assert torch.equal(again32, ref)                                     # the rewound step is the original third step
        assert torch.equal(again16.bfloat16(), again32.bfloat16()) and torch.equal(again16, raw)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_foreign_or_damaged_state_is_refused():
    tr = _trainer()
    for step in range(2):
        _step(tr, step)
    ck = tr.state_dict()
    good = ck["optimizer_states"][0]

    def variant(fn):
        sd = {"state": {i: dict(e) for i, e in good["state"].items()}, "param_groups": good["param_groups"]}
        fn(sd["state"])
        return sd
    # unequal step counts
    with pytest.raises(ValueError, match="step count"):
        tr.opt.load_state_dict(variant(lambda st: st[3].update(step=torch.tensor(5.0))))
    # a moment of the wrong shape names its parameter; the 2-D <-> 4-D view of a 1x1 conv is accepted
    with pytest.raises(ValueError, match=r"1\.weight"):
        tr.opt.load_state_dict(variant(lambda st: st[2].update(exp_avg=st[2]["exp_avg"].t().contiguous())))
    with pytest.raises(ValueError, match=r"2\.weight"):
        tr.opt.load_state_dict(variant(lambda st: st[3].update(exp_avg_sq=torch.zeros(52))))
    tr.opt.load_state_dict(variant(lambda st: st[2].update(exp_avg=st[2]["exp_avg"].reshape(51, 64, 1, 1))))
    assert _eq(tr.opt.state_dict()["state"][2]["exp_avg"], good["state"][2]["exp_avg"])
    # a trained parameter without state: refused; strict=False gives it zero moments and the shared step
    with pytest.raises(ValueError, match=r"0\.bias"):
        tr.opt.load_state_dict(variant(lambda st: st.pop(1)))
    with pytest.warns(UserWarning, match=r"0\.bias"):
        tr.opt.load_state_dict(variant(lambda st: st.pop(1)), strict=False)
    back = tr.opt.state_dict()["state"]
    assert float(back[1]["exp_avg"].abs().max()) == 0.0 and float(back[1]["exp_avg_sq"].abs().max()) == 0.0 and float(back[1]["step"]) == 2.0
    assert _eq(back[0]["exp_avg"], good["state"][0]["exp_avg"]) and _eq(back[6]["exp_avg_sq"], good["state"][6]["exp_avg_sq"])
    # an empty state is a fresh optimizer
    tr.opt.load_state_dict({"state": {}, "param_groups": good["param_groups"]})
    assert tr.opt.adam_step == 0 and float(tr.opt.exp_avg.abs().max()) == 0.0 and float(tr.opt.exp_avg_sq.abs().max()) == 0.0
    # differing hyper-parameters: the live ones win, with a warning
    other = {"state": good["state"], "param_groups": [dict(good["param_groups"][0], weight_decay=0.5, initial_lr=3e-4)]}
    with pytest.warns(UserWarning) as rec:
        tr.opt.load_state_dict(other)
    said = " ".join(str(w.message) for w in rec)
    assert "weight_decay = 0.5" in said and "initial_lr = 0.0003" in said
    assert tr.opt.weight_decay == 1e-2 and tr.opt.lr0 == 1e-2 and tr.opt.adam_step == 2
    # the container: other parameter names
    bad = dict(ck, mv_ldm_amd=dict(ck["mv_ldm_amd"], param_names=list(reversed(ck["mv_ldm_amd"]["param_names"]))))
    with pytest.raises(ValueError, match="parameter names"):
        tr.load_state_dict(bad)
    # ... and a save or load inside an accumulation window
    tr.load_state_dict(ck)
    tr.micro += 1
    with pytest.raises(RuntimeError, match="accumulation window"):
        tr.state_dict()
    with pytest.raises(RuntimeError, match="accumulation window"):
        tr.load_state_dict(ck)


def test_ema_and_scaler_cross_checks_and_a_foreign_lightning_checkpoint():
    """a checkpoint without the "mv_ldm_amd" entry, as Lightning writes it for the reference (16-mixed: `MixedPrecision`, or the older
    `MixedPrecisionPlugin`), loads through the same function; EMA / scaler presence is checked against the trainer"""
    tr = _trainer(dtype=torch.float16, scaler=_scaler_cfg(True), ema_decay=0.995)
    tr.ema.update()
    for step in range(3):
        _step(tr, step)
    tr.ema.avg.mul_(0.5)                                 # (the fused lerp is a HIP kernel: any average that is not the live weights will do)
    tr.ema.n_averaged = 3
    ck = tr.state_dict()
    want = _snapshot(tr)
    foreign = {k: v for k, v in ck.items() if k not in ("mv_ldm_amd", "MixedPrecision")}
    foreign["MixedPrecisionPlugin"] = ck["MixedPrecision"]
    new = _trainer(dtype=torch.float16, scaler=_scaler_cfg(True), ema_decay=0.995)
    new.load_state_dict(foreign)
    got = _snapshot(new)
    for k in ("flat", "m", "v"):
        assert _eq(want[k], got[k]), k
    assert all(want[k] == got[k] for k in ("step_count", "adam_step", "lr", "global_step", "scaler", "skipped")), (want, got)
    assert got["skipped"] == 1 and got["adam_step"] == 2 and new.ema.n_averaged == 3 and torch.equal(new.ema.avg, tr.ema.avg)
    # the record of the earlier Lightning binding
    old = {k: v for k, v in foreign.items() if k != "MixedPrecisionPlugin"}
    old["mv_ldm_amd_grad_scaler"] = {"scaler": ck["MixedPrecision"], "adam_step": 2}
    new = _trainer(dtype=torch.float16, scaler=_scaler_cfg(True), ema_decay=0.995)
    new.load_state_dict(old)
    assert new.scaler_state_dict() == want["scaler"] and new.adam_step == 2 and int(new.skipped_steps) == 1
    # EMA in the file, none in the trainer: a warning;  EMA in the trainer, none in the file: refused / restarted
    plain = _trainer(dtype=torch.float16, scaler=_scaler_cfg(True))
    with pytest.warns(UserWarning, match="EMA"):
        plain.load_state_dict(ck)
    no_ema = dict(ck, state_dict={k: v for k, v in ck["state_dict"].items() if not k.startswith("ema.")})
    new = _trainer(dtype=torch.float16, scaler=_scaler_cfg(True), ema_decay=0.995)
    with pytest.raises(ValueError, match="EMA"):
        new.load_state_dict(no_ema)
    new.load_state_dict(no_ema, strict=False)
    assert new.ema.n_averaged == 0 and torch.equal(new.ema.avg, new.flat.flat) and torch.equal(new.flat.flat, tr.flat.flat)
    # a scaler in the trainer, no record in the file
    with pytest.raises(ValueError, match="scaler"):
        _trainer(dtype=torch.float16, scaler=_scaler_cfg(True), ema_decay=0.995).load_state_dict(foreign | {"MixedPrecisionPlugin": None})
    # a record in the file, no scaler in the trainer: ignored with a warning; one step count, the scheduler's
    bf = _trainer(dtype=torch.bfloat16, ema_decay=0.995)
    with pytest.warns(UserWarning, match="loss-scaler"):
        bf.load_state_dict(ck)
    assert bf.opt.step_count == 3 and bf.global_step == 3


# ---- 6. the container --------------------------------------------------------------------------------------------------------------
def test_checkpoint_file_is_a_lightning_style_container_the_loaders_read(tmp_path):
    from types import SimpleNamespace
    from mv_ldm_amd.checkpoint import load_pipeline_checkpoint, read_state_dict, split_wrapper_state
    tr = _trainer(ema_decay=0.995)
    tr.ema.update()
    for step in range(2):
        _step(tr, step)
    tr.ema.n_averaged = 2
    path = tmp_path / "last.ckpt"
    tr.save_checkpoint(path)
    assert [f.name for f in tmp_path.iterdir()] == ["last.ckpt"]                  # the temporary file was renamed into place
    ck = torch.load(str(path), map_location="cpu", weights_only=True)
    assert list(ck) == ["state_dict", "optimizer_states", "lr_schedulers", "global_step", "epoch", "mv_ldm_amd"]
    assert ck["epoch"] == 0 and ck["global_step"] == 2 and isinstance(ck["global_step"], int)
    meta = ck["mv_ldm_amd"]
    assert meta == {"version": 1, "adam_step": 2, "skipped_steps": 0, "param_names": [n for n, _ in tr.denoiser.named_parameters()],
                    "dtype": "float32", "world": 1, "accumulate_grad_batches": 2}
    sch = ck["lr_schedulers"][0]
    assert sch == {"start_factor": 0.5, "end_factor": 1.0, "total_iters": 4, "base_lrs": [1e-2], "last_epoch": 2, "_step_count": 3,
                   "_last_lr": [tr.opt.lr()]}
    ref = torch.optim.lr_scheduler.LinearLR(torch.optim.AdamW(tr.denoiser.parameters(), lr=1e-2), start_factor=0.5, total_iters=4)
    ref.load_state_dict(sch)                                                      # torch's own scheduler takes it
    assert ref.get_last_lr() == [tr.opt.lr()] and ref.last_epoch == 2
    parts = split_wrapper_state(read_state_dict(path))
    assert not parts["other"] and not parts["autoencoder"]
    assert set(parts["denoiser"]) == set(tr.denoiser.state_dict()) and set(parts["ema"]) == {"module." + k for k in parts["denoiser"]} | {"n_averaged"}
    for k, v in tr.denoiser.state_dict().items():
        assert torch.equal(parts["denoiser"][k], v) and not torch.equal(parts["ema"]["module." + k], v)
    assert int(parts["ema"]["n_averaged"]) == 2
    # sampling from it: the live weights, or the averaged ones
    for use_ema in (False, True):
        pipe = SimpleNamespace(denoiser=_toy_model(), autoencoder=torch.nn.Module())
        with torch.no_grad():
            for p in pipe.denoiser.parameters():
                p.add_(1.0)
        rep = load_pipeline_checkpoint(pipe, path, use_ema=use_ema)
        assert rep["denoiser"].ok() and "autoencoder" not in rep
        want = tr.ema.state_dict() if use_ema else {"module." + k: v for k, v in tr.denoiser.state_dict().items()}
        for k, v in pipe.denoiser.state_dict().items():
            assert torch.equal(v, want["module." + k]), k
    # include_autoencoder adds the frozen VAE's tensors under the reference's prefix
    vae = torch.nn.Linear(2, 2)
    tr.autoencoder = vae
    sd = tr.state_dict(include_autoencoder=True)["state_dict"]
    assert torch.equal(sd["autoencoder.weight"], vae.weight) and "autoencoder.bias" in sd
    # no scheduler: an empty list, and the step count travels in global_step
    tr2 = _trainer(sched=None)
    _step(tr2, 0)
    ck2 = tr2.state_dict()
    assert ck2["lr_schedulers"] == [] and ck2["optimizer_states"][0]["param_groups"][0]["lr"] == 1e-2
    tr3 = _trainer(sched=None)
    tr3.load_state_dict(ck2)
    assert tr3.opt.step_count == 1 and tr3.global_step == 1 and _eq(tr3.opt.exp_avg, tr2.opt.exp_avg)
