"""GPU: PSNR / SSIM of image batches on the device (`csrc/metrics.hip`, `ops.image_metrics`, `mv_ldm_amd.metrics`) against the fp64
restatement of tests/metrics_ref.py, and `MVLDMTrainer.validation_step`.

Tolerances (absolute, to the fp64 restatement): SSIM 2e-5, PSNR 1e-4 dB.  An fp32 torch emulation of the same arithmetic on these
inputs and sizes stays within 3.8e-6 / 1.3e-6 dB on the CPU: the bounds leave about 5x for another fp32 summation order (more for the
PSNR, whose sum is formed in fp64).  The maxima measured on the MI355X are in tests/golden/measured_errors_metrics.json."""

import pytest
import torch

import metrics_ref as R
from conftest import record_err

pytestmark = pytest.mark.gpu

SSIM_TOL, PSNR_TOL = 2e-5, 1e-4


def _tile():
    from mv_ldm_amd import ops
    return ops.IMAGE_METRICS_TILE


def _check(kind, gt, pred, psnr, ssim, tag):
    want_p, want_s = R.compute_psnr(gt, pred), R.compute_ssim(gt, pred)
    got_p, got_s = psnr.double().cpu(), ssim.double().cpu()
    if kind == "identical":
        assert torch.equal(got_s, torch.ones_like(got_s)), (tag, got_s)
        assert bool(torch.isposinf(got_p).all()) and bool(torch.isposinf(want_p).all()), (tag, got_p)
        return
    es = record_err(f"ssim_abs/{kind}", float((got_s - want_s).abs().max()))
    ep = record_err(f"psnr_abs_db/{kind}", float((got_p - want_p).abs().max()))
    print(f"{tag} {kind}: ssim err {es:.3e} (ssim {float(want_s.mean()):.6f}), psnr err {ep:.3e} dB (psnr {float(want_p.mean()):.4f})")
    assert es <= SSIM_TOL, (tag, kind, es)
    assert ep <= PSNR_TOL, (tag, kind, ep)


# 11 x 11: a single output pixel; 43 x 43: a 33 x 33 map, one pixel past the kernel's 32 x 32 output tile in both directions
@pytest.mark.parametrize("hw", [(11, 11), (12, 19), (37, 45), "tile+1"], ids=["11x11", "12x19", "37x45", "tile_plus_1"])
@pytest.mark.parametrize("c,n", [(1, 1), (3, 1), (1, 5), (3, 5)])
def test_parity_with_the_fp64_restatement(hw, c, n):
    from mv_ldm_amd import metrics as M
    h, w = (_tile() + 11, _tile() + 11) if hw == "tile+1" else hw
    for kind in R.KINDS:
        gt, pred = R.make_pair(kind, n, c, h, w, seed=h * 1000 + w + 7 * c + n)
        psnr, ssim = M.image_metrics(gt.cuda(), pred.cuda())
        assert psnr.shape == ssim.shape == (n,) and psnr.dtype == torch.float32 and psnr.is_cuda
        _check(kind, gt, pred, psnr, ssim, f"{n}x{c}x{h}x{w}")


def test_parity_at_the_sampler_resolution():
    from mv_ldm_amd import metrics as M
    for kind in R.KINDS:
        gt, pred = R.make_pair(kind, 8, 3, 256, 256, seed=256)
        psnr, ssim = M.image_metrics(gt.cuda(), pred.cuda())
        _check(kind, gt, pred, psnr, ssim, "8x3x256x256")


def test_clipping_applies_to_the_psnr_only():
    """values outside [0, 1]: the PSNR equals the PSNR of the clipped pair, the SSIM does not equal the clipped pair's"""
    from mv_ldm_amd import metrics as M
    gt, pred = R.make_pair("out_of_range", 2, 3, 37, 45, seed=3)
    p, s = M.image_metrics(gt.cuda(), pred.cuda())
    pc, sc = M.image_metrics(gt.clip(0, 1).cuda(), pred.clip(0, 1).cuda())
    assert torch.equal(p, pc)
    assert float((s - sc).abs().min()) > 1e-3


def test_use_sample_covariance_is_a_parameter():
    from mv_ldm_amd import metrics as M, ops
    gt, pred = R.make_pair("noise05", 3, 3, 37, 45, seed=5)
    for flag in (True, False):
        _, s = ops.image_metrics(pred.cuda(), gt.cuda(), use_sample_covariance=flag)
        e = record_err("ssim_abs/noise05", float((s.double().cpu() - R.compute_ssim(gt, pred, flag)).abs().max()))
        assert e <= SSIM_TOL, (flag, e)
        assert torch.equal(s, M.compute_ssim(gt.cuda(), pred.cuda(), use_sample_covariance=flag))
    assert float((R.compute_ssim(gt, pred, True) - R.compute_ssim(gt, pred, False)).abs().min()) > 10 * SSIM_TOL      # the flag is visible


def test_launches_are_bit_identical_and_images_are_scored_independently():
    from mv_ldm_amd import metrics as M
    t = _tile()
    gt, pred = R.make_pair("noise05", 5, 3, 2 * t + 17, t + 13, seed=11)
    gt, pred = gt.cuda(), pred.cuda()
    p0, s0 = M.image_metrics(gt, pred)
    p1, s1 = M.image_metrics(gt, pred)
    assert torch.equal(p0, p1) and torch.equal(s0, s1)
    for i in range(5):                                          # alone
        p, s = M.image_metrics(gt[i:i + 1], pred[i:i + 1])
        assert torch.equal(p, p0[i:i + 1]) and torch.equal(s, s0[i:i + 1]), i
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")        # another position, another batch size
    p, s = M.image_metrics(gt[perm][:4].contiguous(), pred[perm][:4].contiguous())
    assert torch.equal(p, p0[perm][:4]) and torch.equal(s, s0[perm][:4])
    assert len(set(s0.tolist())) == 5                           # five different images


def test_the_reference_signatures_and_the_view_axis():
    from mv_ldm_amd import metrics as M
    gt, pred = R.make_pair("noise05", 6, 3, 24, 31, seed=13)
    gt, pred = gt.cuda(), pred.cuda()
    p, s = M.image_metrics(gt, pred)
    assert torch.equal(M.compute_psnr(gt, pred), p) and torch.equal(M.compute_ssim(gt, pred), s)
    p5, s5 = M.image_metrics(gt.view(2, 3, 3, 24, 31), pred.view(2, 3, 3, 24, 31))
    assert p5.shape == s5.shape == (2, 3) and torch.equal(p5.reshape(-1), p) and torch.equal(s5.reshape(-1), s)
    # 16-bit inputs go through the elementwise convert: the scores of the rounded images
    for dt in (torch.float16, torch.bfloat16):
        ph, sh = M.image_metrics(gt.to(dt), pred.to(dt))
        pf, sf = M.image_metrics(gt.to(dt).float(), pred.to(dt).float())
        assert ph.dtype == torch.float32 and torch.equal(ph, pf) and torch.equal(sh, sf)
    with pytest.raises(TypeError):
        M.image_metrics((gt * 255).to(torch.uint8), (pred * 255).to(torch.uint8))


def test_a_captured_launch_scores_the_new_contents_of_its_buffers():
    from mv_ldm_amd import ops
    n, c, h, w = 3, 3, 37, 45
    a0, b0 = R.make_pair("noise05", n, c, h, w, seed=17)
    a1, b1 = R.make_pair("random", n, c, h, w, seed=19)
    gt, pred = a0.cuda(), b0.cuda()
    out = (torch.empty(n, device="cuda"), torch.empty(n, device="cuda"))
    ws = torch.empty(ops.image_metrics_workspace_bytes(n, c, h, w), dtype=torch.uint8, device="cuda")
    want0 = tuple(t.clone() for t in ops.image_metrics(pred, gt))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.image_metrics(pred, gt, out=out, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.image_metrics(pred, gt, out=out, ws=ws)
    graph.replay()
    assert torch.equal(out[0], want0[0]) and torch.equal(out[1], want0[1])
    gt.copy_(a1)
    pred.copy_(b1)
    graph.replay()
    want1 = ops.image_metrics(b1.cuda(), a1.cuda())
    assert torch.equal(out[0], want1[0]) and torch.equal(out[1], want1[1])
    assert not torch.equal(want0[1], want1[1])


def test_refusals_return_a_status_and_launch_nothing():
    from mv_ldm_amd import _lib as L, metrics as M, ops
    lib = L.load()
    n, c = 2, 3
    x = torch.rand(n, c, 64, 64, device="cuda")
    psnr, ssim = torch.full((n,), -7.0, device="cuda"), torch.full((n,), -7.0, device="cuda")
    need = ops.image_metrics_workspace_bytes(n, c, 64, 64)
    assert need == n * c * 4 * 16                       # a 54 x 54 map: 2 x 2 tiles, one fp64 pair each
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    call = lambda h, w, nbytes, p=x.data_ptr(), cc=c: lib.mvldm_image_metrics(p, x.data_ptr(), n, cc, h, w, 1, psnr.data_ptr(), ssim.data_ptr(),
                                                                             ws.data_ptr(), nbytes, ops.stream())
    assert call(10, 64, need) < 0
    assert b"window" in lib.mvldm_last_error()
    assert call(64, 10, need) < 0 and ops.image_metrics_workspace_bytes(n, c, 10, 64) == 0
    assert call(64, 64, need - 8) < 0 and b"workspace" in lib.mvldm_last_error()
    assert call(64, 64, need, p=None) < 0 and b"null" in lib.mvldm_last_error()
    assert call(64, 64, need, cc=0) < 0
    torch.cuda.synchronize()
    assert bool((psnr == -7).all()) and bool((ssim == -7).all()) and not bool(ws.any())
    with pytest.raises(L.MvldmError, match="window"):
        M.image_metrics(x[:, :, :10].contiguous(), x[:, :, :10].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        M.image_metrics(x[:, :, ::2], x[:, :, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        ops.image_metrics(x.transpose(2, 3), x.transpose(2, 3))
    assert call(64, 64, need) == 0                       # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert bool(torch.isposinf(psnr).all()) and bool((ssim == 1).all())


# ---- MVLDMTrainer.validation_step -----------------------------------------------------------------------------------
# the reduced-width G9 trainer of tests/test_hip_train.py, f32, rule-based tiles and ONE pinned implicit-GEMM tile (as
# tests/test_hip_headline.py pins it): two pipelines over equal weights then run the same instruction sequences
def _pin(monkeypatch):
    monkeypatch.setenv("MVLDM_AUTOTUNE", "0")
    monkeypatch.setenv("MVLDM_TRAIN_AUTOTUNE", "0")
    monkeypatch.setenv("MVLDM_IGEMM_TILE", "2")


def _val_inputs(seed=23):
    g = torch.Generator().manual_seed(seed)
    return dict(x_T=torch.randn(2, 4, 4, 16, 16, generator=g), encode_noise=torch.randn(2, 4, 16, 16, generator=g),
                roundtrip_noise=torch.randn(8, 4, 16, 16, generator=g), second=1)


def test_validation_step_samples_with_the_weights_of_the_last_optimizer_step(golden, tmp_path, monkeypatch):
    import mv_ldm_amd
    from conftest import rel_err
    from mv_ldm_amd import metrics as M
    from mv_ldm_amd.checkpoint import load_pipeline_checkpoint
    from mv_ldm_amd.pipeline import MVLDMPipeline, SamplerCfg
    from mv_ldm_amd.train import OptimizerCfg
    from test_hip_train import build_trainer
    from test_hip_train_resume import _window
    from test_oracle_train import g9_case
    _pin(monkeypatch)
    g = golden("g9_training_step")
    batch, _ = g9_case(g, 0)                                   # 2 scenes, 2 context + 3 target views of 32 x 32
    kw = _val_inputs()
    with torch.enable_grad():
        tr = build_trainer(g, torch.float32, optimizer_cfg=OptimizerCfg(lr=1e-3))
        before = tr.validation_step(batch, num_inference_steps=2, **kw)
        _window(tr, g, 0)
        out = tr.validation_step(batch, num_inference_steps=2, **kw)
    b, v_t = 2, 4                                              # one context view kept, the other joins the 3 targets
    assert out["sampled"].shape == out["targets"].shape == out["targets_roundtrip"].shape == (b, v_t, 3, 32, 32)
    assert out["context"].shape == (b, 1, 3, 32, 32) and torch.equal(out["context"].cpu(), batch["context"]["image"][:, 1:2])
    assert torch.equal(out["targets"].cpu(), torch.cat([batch["target"]["image"], batch["context"]["image"][:, 0:1]], dim=1))
    assert all(out[k].shape == (b, v_t) and out[k].is_cuda for k in ("psnr", "ssim", "psnr_roundtrip", "ssim_roundtrip"))
    assert 0.0 <= float(out["sampled"].min()) and float(out["sampled"].max()) <= 1.0
    # the same sliced batch and noise through a pipeline loaded from the trainer's state_dict()
    path = tmp_path / "val.ckpt"
    tr.save_checkpoint(path)
    other = build_trainer(g, torch.float32)
    pipe = MVLDMPipeline(other.denoiser, other.autoencoder, other.scheduler, SamplerCfg(num_inference_steps=2))
    assert load_pipeline_checkpoint(pipe, path)["denoiser"].ok()
    pipe.set_timesteps()
    with mv_ldm_amd.compute_dtype(torch.float32):
        want, _ = pipe.sample(out["batch"], x_T=kw["x_T"], encode_noise=kw["encode_noise"])
    e = record_err("validation_sampled_vs_pipeline/float32", rel_err(out["sampled"], want))
    moved = rel_err(out["sampled"], before["sampled"])
    print(f"validation_step vs a pipeline loaded from state_dict(): rel-err {e:.3e}; against the weights one step earlier: {moved:.3e}")
    assert e < 2e-6, e
    assert moved > 1e-4, moved                                 # the optimizer step is visible in the sample: stale packs would not pass
    # the scores are the metrics of the returned images
    p, s = M.image_metrics(out["targets"], out["sampled"])
    assert torch.equal(out["psnr"], p) and torch.equal(out["ssim"], s)
    p, s = M.image_metrics(out["targets_roundtrip"], out["sampled"])
    assert torch.equal(out["psnr_roundtrip"], p) and torch.equal(out["ssim_roundtrip"], s)
    assert bool(torch.isfinite(out["psnr"]).all()) and not torch.equal(out["psnr"], out["psnr_roundtrip"])


def test_validation_step_leaves_training_untouched(golden, monkeypatch):
    """step -> validation_step -> step equals step -> step bit for bit (losses, masters, both moments), although the validation
    draws its own x_T and posterior noise (forked RNG scope); in the middle of an accumulation window it refuses"""
    from test_hip_train import build_trainer, hip_choices
    from test_hip_train_resume import _assert_same, _snap, _window
    from test_oracle_train import g9_case
    _pin(monkeypatch)
    g = golden("g9_training_step")
    batch, ch = g9_case(g, 0)
    with torch.enable_grad():
        runs = {}
        for validate in (False, True):
            tr = build_trainer(g, torch.float32)
            torch.manual_seed(5)
            losses = [_window(tr, g, 0)]
            state = torch.random.get_rng_state()
            if validate:
                out = tr.validation_step(batch, num_inference_steps=2)
                assert bool(torch.isfinite(out["ssim"]).all())
                assert torch.equal(torch.random.get_rng_state(), state)
            losses.append(_window(tr, g, 1))
            runs[validate] = (torch.stack(losses), _snap(tr))
        assert torch.equal(runs[True][0], runs[False][0]), (runs[True][0], runs[False][0])
        _assert_same(runs[False][1], runs[True][1], "with / without validation_step")
        assert runs[True][1]["global_step"] == 2
        tr.training_step(batch, **hip_choices(ch))              # micro-batch 1 of 2
        with pytest.raises(RuntimeError, match="accumulation window"):
            tr.validation_step(batch, num_inference_steps=2)
        tr.training_step(batch, **hip_choices(ch))
        with pytest.raises(NotImplementedError):
            tr.validation_step(batch, num_inference_steps=2, use_ema=True)


def test_validation_step_leaves_a_window_encoded_ahead_untouched(golden, monkeypatch):
    """window(prefetch=next) -> validation_step -> window(next): the next window's images are being encoded on the side stream, in
    the frozen VAE's one set of plan buffers, when the validation runs its own encodes and decodes through the same plans.  The
    prefetched latents are taken (no second encode) and both windows equal the run that never validated, bit for bit"""
    from test_hip_train import build_trainer, hip_choices
    from test_hip_train_resume import SEQ, _assert_same, _snap
    from test_oracle_train import g9_case
    _pin(monkeypatch)
    g = golden("g9_training_step")
    val_batch, _ = g9_case(g, 2)
    with torch.enable_grad():
        runs = {}
        for validate in (False, True):
            tr = build_trainer(g, torch.float32)
            encodes = []
            real = tr._prepare_window
            monkeypatch.setattr(tr, "_prepare_window", lambda b_, c_: (encodes.append(torch.cuda.current_stream()), real(b_, c_))[1])
            wins = []
            for k in (0, 1):
                cases = [g9_case(g, ci) for ci in SEQ[k]]
                wins.append(([c[0] for c in cases], [hip_choices(c[1]) for c in cases]))
            if validate:
                tr.validation_step(val_batch, num_inference_steps=2)        # records the VAE plans validation and training share
            losses = [tr.training_window(*wins[0], prefetch=wins[1]).clone()]
            assert len(encodes) == 2 and encodes[1] != encodes[0] and "_prefetched" in tr.__dict__      # window 1 is encoded ahead, on a side stream
            if validate:
                out = tr.validation_step(val_batch, num_inference_steps=2)
                assert bool(torch.isfinite(out["psnr_roundtrip"]).all()) and "_prefetched" in tr.__dict__
            losses.append(tr.training_window(*wins[1]).clone())
            assert len(encodes) == 2, "the window encoded ahead was not taken"
            runs[validate] = (torch.stack(losses), _snap(tr))
        assert torch.equal(runs[True][0], runs[False][0]), (runs[True][0], runs[False][0])
        _assert_same(runs[False][1], runs[True][1], "prefetched window, with / without validation_step")
