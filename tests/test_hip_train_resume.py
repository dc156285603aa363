"""GPU: a training run stopped at a checkpoint and continued by a freshly built trainer (`MVLDMTrainer.save_checkpoint /
load_checkpoint`) is, bit for bit, the run that was never stopped -- through the HIP forward / backward plans, the fused clip + AdamW
step, the f16 loss scaler's device record, the RCCL branch with its 16-bit parameter gather, and the EMA.

The reduced-width G9 trainer of tests/test_hip_train.py, rule-based tiles (MVLDM_AUTOTUNE=0 / MVLDM_TRAIN_AUTOTUNE=0: two trainer
instances then record identical kernels, which is what test_ema_applied_right_after_a_window... and the 1-rank nccl tests already
rely on).  Every comparison is `torch.equal`; each test carries a negative control or a non-triviality check, so a comparison that
passes says something."""
import socket

import pytest
import torch

from test_hip_train import build_trainer, hip_choices
from test_oracle_train import g9_case

GRAD_ENABLED = True
pytestmark = pytest.mark.gpu

SEQ = [(0, 2), (1, 0), (0, 2), (1, 0)]          # the G9 cases of the four accumulation windows


def _window(tr, g, k):
    cases = [g9_case(g, ci) for ci in SEQ[k]]
    return tr.training_window([c[0] for c in cases], [hip_choices(c[1]) for c in cases]).clone()


def _kw(dtype, **more):
    from mv_ldm_amd.train import GradScalerCfg, OptimizerCfg, TrainCfg
    kw = dict(optimizer_cfg=OptimizerCfg(lr=1e-3), **more)
    if dtype == torch.float16:      # window 1 overflows f16 and is skipped (test_forced_overflow_skips_the_step_and_backs_off); S grows after window 4
        kw["train_cfg"] = TrainCfg(grad_scaler=GradScalerCfg(init_scale=2.0 ** 60, backoff_factor=2.0 ** -44, growth_interval=3))
    return kw


def _snap(tr, norm=True):
    torch.cuda.synchronize()
    s = dict(flat=tr.flat.flat.clone(), m=tr.opt.exp_avg.clone(), v=tr.opt.exp_avg_sq.clone(), global_step=tr.global_step,
             step_count=tr.opt.step_count, adam_step=tr.adam_step, lr=tr.opt.lr())
    if norm:
        s["norm"] = tr.opt.norm.clone()
    if tr.grad_scale is not None:
        s.update(scale=float(tr.grad_scale), skipped=int(tr.skipped_steps), scaler=tr.scaler_state_dict())
    if tr.ema is not None:
        s.update(ema=tr.ema.avg.clone(), n_averaged=tr.ema.n_averaged)
    return s


def _assert_same(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k, v in a.items():
        if torch.is_tensor(v):
            assert torch.equal(v, b[k]), (what, k, float((v.double() - b[k].double()).abs().max()))
        else:
            assert v == b[k], (what, k, v, b[k])


def _rules_only(monkeypatch):
    monkeypatch.setenv("MVLDM_AUTOTUNE", "0")
    monkeypatch.setenv("MVLDM_TRAIN_AUTOTUNE", "0")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_resumed_trainer_continues_bit_identically(golden, dtype, tmp_path, monkeypatch):
    """A: four windows, checkpoint after the second.  B: fresh trainer, `load_checkpoint`, windows 3-4: the losses, `opt.norm`, the
    masters, both moments, `global_step` / `adam_step` / `lr()` and (f16) the scale, growth tracker and skipped steps equal A's after
    each window.  C (negative control): fresh trainer with only A's WEIGHTS from the same file -- zero moments, step count 0 -- does
    not follow A."""
    from mv_ldm_amd.checkpoint import split_wrapper_state
    _rules_only(monkeypatch)
    g = golden("g9_training_step")
    path = tmp_path / "last.ckpt"
    a = build_trainer(g, dtype, **_kw(dtype))
    for k in (0, 1):
        _window(a, g, k)
    a.save_checkpoint(path)
    mid = _snap(a, norm=False)
    want = [(_window(a, g, k), _snap(a)) for k in (2, 3)]
    assert mid["global_step"] == 2 and float(mid["m"].abs().max()) > 0 and not torch.equal(mid["flat"], want[0][1]["flat"])
    if dtype == torch.float16:
        assert mid["skipped"] == 1 and mid["adam_step"] == 1 and mid["scale"] == 2.0 ** 16 and mid["scaler"]["_growth_tracker"] == 1
        assert want[0][1]["scaler"]["_growth_tracker"] == 2 and want[1][1]["scale"] == 2.0 ** 17
        assert want[1][1]["adam_step"] == 3 and want[1][1]["skipped"] == 1
    else:
        assert mid["adam_step"] == 2
    del a
    b = build_trainer(g, dtype, **_kw(dtype))
    ckpt = b.load_checkpoint(path)
    _assert_same(mid, _snap(b, norm=False), "after load")
    for i, k in enumerate((2, 3)):
        losses = _window(b, g, k)
        assert torch.equal(losses, want[i][0]), (k, losses, want[i][0])
        _assert_same(want[i][1], _snap(b), f"after window {k + 1}")
    del b
    c = build_trainer(g, dtype, **_kw(dtype))
    c.load_denoiser_state_dict({k: v.cuda() for k, v in split_wrapper_state(ckpt["state_dict"])["denoiser"].items()})
    assert torch.equal(c.flat.flat, mid["flat"])
    _window(c, g, 2)
    torch.cuda.synchronize()
    assert not torch.equal(c.flat.flat, want[0][1]["flat"])


def test_checkpoints_travel_between_the_rccl_branch_and_the_plain_trainer(golden, tmp_path, monkeypatch):
    """a `collective=True` trainer on a 1-rank nccl group (bf16: the 16-bit parameter gather and its `_p16` copy are live) and a plain
    trainer each run two windows and save; each then loads the OTHER's file into a fresh trainer of its own kind: window 3 is
    bit-identical to the third window of the uninterrupted runs, both ways"""
    import torch.distributed as dist
    _rules_only(monkeypatch)
    g = golden("g9_training_step")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    assert not dist.is_initialized()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        def build(collective):
            tr = build_trainer(g, torch.bfloat16, **_kw(torch.bfloat16, bucket_bytes=2 << 20, group=dist.group.WORLD if collective else None,
                                                        collective=collective))
            assert tr.opt.collective == collective and len(tr.opt.buckets) > 8
            assert (tr.opt.gather_dtype == torch.bfloat16) == collective
            return tr
        files, want = {}, {}
        for collective in (False, True):
            tr = build(collective)
            for k in (0, 1):
                _window(tr, g, k)
            files[collective] = tmp_path / f"{int(collective)}.ckpt"
            tr.save_checkpoint(files[collective])
            assert (tr.opt._p16 is not None) == collective
            want[collective] = (_window(tr, g, 2), _snap(tr))
            del tr
        _assert_same(want[False][1], want[True][1], "uninterrupted: plain vs collective")
        for collective in (False, True):
            tr = build(collective)
            tr.load_checkpoint(files[not collective])
            losses = _window(tr, g, 2)
            assert torch.equal(losses, want[collective][0])
            _assert_same(want[collective][1], _snap(tr), f"collective={collective} from the other's file")
            del tr
    finally:
        dist.destroy_process_group()


def test_ema_resumes_and_the_file_samples_with_the_averaged_weights(golden, tmp_path, monkeypatch):
    from mv_ldm_amd.checkpoint import load_pipeline_checkpoint
    from mv_ldm_amd.pipeline import MVLDMPipeline
    _rules_only(monkeypatch)
    g = golden("g9_training_step")
    path = tmp_path / "last.ckpt"
    a = build_trainer(g, torch.bfloat16, **_kw(torch.bfloat16, ema_decay=0.995))
    for k in (0, 1):
        _window(a, g, k)
    a.save_checkpoint(path)
    mid = _snap(a, norm=False)
    assert mid["n_averaged"] == 2 and not torch.equal(mid["ema"], mid["flat"])
    for k in (2, 3):
        _window(a, g, k)
    want = _snap(a)
    assert want["n_averaged"] == 4 and not torch.equal(want["ema"], mid["ema"])
    del a
    b = build_trainer(g, torch.bfloat16, **_kw(torch.bfloat16, ema_decay=0.995))
    b.load_checkpoint(path)
    _assert_same(mid, _snap(b, norm=False), "after load")
    for k in (2, 3):
        _window(b, g, k)
    _assert_same(want, _snap(b), "after window 4")
    del b
    # a pipeline loaded from the file: the averaged weights with use_ema, the live ones without
    for use_ema in (True, False):
        t = build_trainer(g, torch.bfloat16)              # a freshly seeded denoiser + VAE (its flat buffer: where the parameters live)
        pipe = MVLDMPipeline(t.denoiser, t.autoencoder, t.scheduler)
        assert not torch.equal(t.flat.flat, mid["flat"])
        rep = load_pipeline_checkpoint(pipe, path, use_ema=use_ema)
        assert rep["denoiser"].ok()
        torch.cuda.synchronize()
        assert torch.equal(t.flat.flat, mid["ema"] if use_ema else mid["flat"])
        del t, pipe


def test_exported_optimizer_state_is_a_torch_adamw_state_dict(golden, tmp_path, monkeypatch):
    """`optimizer_states[0]` loads into a real `torch.optim.AdamW(denoiser.parameters())` on the GPU: entries for exactly the trained
    parameters (the SD up-block transformers, never trained, have none), holding the flat moments; a checkpoint asked for in the
    middle of an accumulation window is refused"""
    _rules_only(monkeypatch)
    g = golden("g9_training_step")
    tr = build_trainer(g, torch.bfloat16, **_kw(torch.bfloat16))
    for k in (0, 1):
        _window(tr, g, k)
    ck = tr.state_dict()
    params = list(tr.denoiser.parameters())
    trained = {id(p) for p in tr.flat.params}
    idx = [i for i, p in enumerate(params) if id(p) in trained]
    assert 0 < len(idx) < len(params) and sorted(ck["optimizer_states"][0]["state"]) == idx
    assert ck["mv_ldm_amd"]["param_names"] == [n for n, _ in tr.denoiser.named_parameters()] and ck["global_step"] == 2
    topt = torch.optim.AdamW(params, lr=1.0)
    topt.load_state_dict(ck["optimizer_states"][0])
    assert topt.param_groups[0]["lr"] == tr.opt.lr() and len(topt.state) == len(idx)
    for i in idx:
        p, st = params[i], topt.state[params[i]]
        o = tr.flat.offset[id(p)]
        assert st["exp_avg"].is_cuda and st["exp_avg"].shape == p.shape and float(st["step"]) == 2.0
        assert torch.equal(st["exp_avg"].reshape(-1), tr.opt.exp_avg[o:o + p.numel()])
        assert torch.equal(st["exp_avg_sq"].reshape(-1), tr.opt.exp_avg_sq[o:o + p.numel()])
    batch, ch = g9_case(g, 0)
    tr.training_step(batch, **hip_choices(ch))            # micro-batch 1 of 2
    with pytest.raises(RuntimeError, match="accumulation window"):
        tr.save_checkpoint(tmp_path / "mid.ckpt")
    assert not list(tmp_path.iterdir())
    tr.training_step(batch, **hip_choices(ch))
    tr.save_checkpoint(tmp_path / "ok.ckpt")
    assert tr.global_step == 3 and torch.load(tmp_path / "ok.ckpt", weights_only=True)["global_step"] == 3
