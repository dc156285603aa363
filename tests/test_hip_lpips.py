"""GPU: LPIPS(net="vgg") on the device (`csrc/lpips.hip`, `mv_ldm_amd.lpips.LPIPS`, `metrics.compute_lpips`) against the fp64
restatement of tests/lpips_ref.py with seeded random weights, and `MVLDMTrainer.validation_step(lpips=...)`.

Error of the whole metric: |got - want| / want per image.  The bounds come from the CPU (tests/golden/lpips_cpu_emulation.json, written by
tests/golden/make_lpips_bounds.py on exactly these inputs), never from the kernels: f32 -- 10 x the worst error of the fp32 torch
emulation of that pair kind (the MFMA sums K in another order through 13 layers; tests/test_hip_metrics.py leaves 5 x for one layer of
sums); f16 / bf16 -- 3 x the worst error of that type's rounding emulation.  The tap kernel alone: 1e-5 relative on the per-image sums
(fp32 sums of at most 512 non-negative terms per pixel, then fp64), its pooled output bit for bit.  The maxima measured on the MI355X
are in tests/golden/measured_errors_lpips.json."""
import json

import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R
from conftest import GOLDEN, record_err

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
NAME = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}
TAP_TOL = 1e-5


@pytest.fixture(scope="module")
def emu():
    return json.loads((GOLDEN / "lpips_cpu_emulation.json").read_text())


@pytest.fixture(scope="module")
def weights():
    return R.make_weights(R.WEIGHT_SEED)


@pytest.fixture(scope="module")
def model(weights):
    from mv_ldm_amd.lpips import LPIPS
    return LPIPS(weights=weights).cuda()


def bound(emu, dtype, kind):
    return (10.0 if dtype == torch.float32 else 3.0) * emu["worst_rel_err"][NAME[dtype]][kind]


# ---- the tap kernel alone ---------------------------------------------------------------------------------------------------------
def _tap_maps(n, h, w, c, dtype, seed):
    """pre-activation NHWC [2n, h, w, c] in `dtype`; an eighth of the pixels has every channel <= 0 in the first image only, another
    eighth in both (together at most a quarter of the map, so they cannot carry the case)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2 * n, h, w, c, generator=g)
    k = (h * w) // 8
    for i in range(n):
        px = torch.randperm(h * w, generator=g)[:2 * k]
        for j, p in enumerate(px.tolist()):
            y, xx = divmod(p, w)
            x[i, y, xx] = -x[i, y, xx].abs()
            if j >= k:
                x[n + i, y, xx] = -x[n + i, y, xx].abs()
    return x.to(dtype), k


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("c", [64, 128, 256, 512])
def test_tap_distance_and_pooled_map(c, dtype):
    from mv_ldm_amd import ops
    g = torch.Generator().manual_seed(c)
    worst = 0.0
    for (h, w) in ((1, 1), (2, 3), (5, 7), (33, 18)):
        for n in (1, 3):
            x, k = _tap_maps(n, h, w, c, dtype, seed=c + 31 * h + n)
            lw = torch.rand(c, generator=g) * 0.02
            slots = ops.lpips_tap_slots(h, w, c)
            assert slots == -(-((h + 1) // 2 * ((w + 1) // 2)) // max(8, 4096 // c))
            ws = torch.zeros(n * (slots + 2) * 8, dtype=torch.uint8, device="cuda")         # one unused slot on either side
            pooled = ops.lpips_tap(x.cuda(), lw.cuda(), ws, 1, slots + 2)
            part = ws.view(torch.float64).view(n, slots + 2).cpu()
            assert bool((part[:, 0] == 0).all()) and bool((part[:, -1] == 0).all())
            nchw = x.double().permute(0, 3, 1, 2)                                             # the rounded inputs, in fp64
            want = R.tap_distance(nchw[:n], nchw[n:], lw.double())
            got = part[:, 1:-1].sum(dim=1)
            assert bool(torch.isfinite(got).all()) and bool((want > 0).all())
            if k:                                                                             # a pixel dead in both images adds 0, in one: sum_c w_c b_c^2 / nb^2
                dead_one = (nchw[:n].amax(dim=1) <= 0) & (nchw[n:].amax(dim=1) > 0)
                assert int(dead_one.sum()) == n * k and int(((nchw[:n].amax(dim=1) <= 0) & (nchw[n:].amax(dim=1) <= 0)).sum()) == n * k
            e = float(((got - want).abs() / want).max())
            worst = max(worst, e)
            assert e <= TAP_TOL, (c, dtype, h, w, n, e)
            if h >= 2 and w >= 2:
                want_pool = F.max_pool2d(x.float().permute(0, 3, 1, 2).relu(), 2).permute(0, 2, 3, 1).to(dtype)
            else:                                                                             # a single row / column: nothing to pool
                want_pool = torch.empty(2 * n, h // 2, w // 2, c, dtype=dtype)
            assert pooled.shape == (2 * n, h // 2, w // 2, c) and pooled.dtype == dtype
            assert torch.equal(pooled.cpu(), want_pool), (c, dtype, h, w, n)
            assert ops.lpips_tap(x.cuda(), lw.cuda(), ws, 1, slots + 2, pool=False) is None  # tap 5: a null destination
            assert torch.equal(ws.view(torch.float64).view(n, slots + 2).cpu(), part)
    print(f"tap C={c} {NAME[dtype]}: worst rel err {record_err(f'tap_rel/{NAME[dtype]}', worst):.3e}")


# ---- the whole metric -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("n,h,w", R.CASES, ids=lambda v: str(v))
def test_parity_with_the_fp64_restatement(n, h, w, dtype, model, weights, emu):
    for kind in (R.KINDS if dtype == torch.float32 else (*R.KINDS_16BIT, "identical")):
        gt, pred = R.make_pair(kind, n, h, w, seed=R.case_seed(n, h, w))
        got = model(gt.cuda(), pred.cuda(), normalize=True, dtype=dtype)
        assert got.shape == (n, 1, 1, 1) and got.dtype == torch.float32 and got.is_cuda
        got = got.double().cpu().view(-1)
        if kind == "identical":
            assert torch.equal(got, torch.zeros(n, dtype=torch.float64)), (kind, got)
            continue
        if h * w <= 64 * 64:
            stats = {}
            want = R.lpips(gt, pred, weights, normalize=True, stats=stats)
            assert stats["min_norm"] >= 1.0, stats                   # well conditioned: no pixel's channel norm is near the 1e-10
            assert torch.allclose(want, torch.tensor(emu["want"][R.case_key(kind, n, h, w)], dtype=torch.float64), rtol=1e-9, atol=0)
        else:                                                        # 256 x 256: the fp64 scores the bounds script recorded
            want = torch.tensor(emu["want"][R.case_key(kind, n, h, w)], dtype=torch.float64)
        e = record_err(f"lpips_rel/{NAME[dtype]}/{kind}", float(((got - want).abs() / want).max()))
        print(f"{n}x3x{h}x{w} {NAME[dtype]} {kind}: rel err {e:.3e}, bound {bound(emu, dtype, kind):.3e} (lpips {float(want.mean()):.4e})")
        assert e <= bound(emu, dtype, kind), (kind, e, bound(emu, dtype, kind))
    assert emu["min_norm"] >= 1.0


def test_symmetry_and_normalize(model):
    gt, pred = R.make_pair("noise05", 3, 37, 45, seed=1)
    gt, pred = gt.cuda(), pred.cuda()
    ab, ba = model(gt, pred, normalize=True), model(pred, gt, normalize=True)
    assert torch.equal(ab, ba)                                       # (a - b)^2: the same bits either way round
    raw = model((2 * gt - 1).contiguous(), (2 * pred - 1).contiguous())
    assert float(((raw - ab).abs() / ab).max()) < 1e-5               # normalize = the 2x - 1 in front (2x - 1 is rounded once more here)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_launches_are_bit_identical(dtype, model):
    gt, pred = R.make_pair("random", 3, 37, 45, seed=2)
    a = model(gt.cuda(), pred.cuda(), normalize=True, dtype=dtype)
    b = model(gt.cuda(), pred.cuda(), normalize=True, dtype=dtype)
    assert torch.equal(a, b) and bool((a > 0).all()) and len(set(a.view(-1).tolist())) == 3


def test_an_image_scores_the_same_alone_elsewhere_and_in_chunks(model, emu, monkeypatch):
    """the conv tile may differ with the batch size, so not bit for bit: within the f32 bound of the batched value"""
    monkeypatch.setenv("MVLDM_AUTOTUNE", "0")
    kind, tol = "noise05", bound(emu, torch.float32, "noise05")
    gt, pred = R.make_pair(kind, 5, 37, 45, seed=3)
    gt, pred = gt.cuda(), pred.cuda()
    full = model(gt, pred, normalize=True).view(-1)
    rel = lambda a, b: float(((a - b).abs() / b).max())
    for i in range(5):
        assert rel(model(gt[i:i + 1], pred[i:i + 1], normalize=True).view(-1), full[i:i + 1]) <= tol, i
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    assert rel(model(gt[perm][:4].contiguous(), pred[perm][:4].contiguous(), normalize=True).view(-1), full[perm][:4]) <= tol
    # chunks of 2 + 2 + 1 pairs (what the 2 GiB rule does to a large batch) through one workspace
    monkeypatch.setattr(type(model), "chunk_pairs", staticmethod(lambda h, w, dtype: 2))
    assert rel(model(gt, pred, normalize=True).view(-1), full) <= tol
    monkeypatch.undo()
    assert type(model).chunk_pairs(256, 256, torch.float32) == 64 and type(model).chunk_pairs(256, 256, torch.float16) == 128
    assert type(model).chunk_pairs(2048, 2048, torch.float32) == 1


def test_a_captured_launch_scores_the_new_contents_of_its_buffers(model):
    from mv_ldm_amd import ops
    n, h, w = 3, 37, 45
    a0, b0 = R.make_pair("noise05", n, h, w, seed=17)
    a1, b1 = R.make_pair("random", n, h, w, seed=19)
    gt, pred = a0.cuda(), b0.cuda()
    out = torch.empty(n, 1, 1, 1, device="cuda")
    ws = torch.empty(ops.lpips_workspace_bytes(n, h, w), dtype=torch.uint8, device="cuda")
    want0 = model(gt, pred, normalize=True).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model(gt, pred, normalize=True, out=out, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                    # one stream: a single-branch graph
        model(gt, pred, normalize=True, out=out, ws=ws)
    graph.replay()
    assert torch.equal(out, want0)
    gt.copy_(a1)
    pred.copy_(b1)
    graph.replay()
    want1 = model(a1.cuda(), b1.cuda(), normalize=True)
    assert torch.equal(out, want1) and not torch.equal(want0, want1)


def test_refusals_return_a_status_and_launch_nothing(model):
    from mv_ldm_amd import _lib as L, ops
    lib = L.load()
    n, h, w, c = 2, 8, 8, 64
    x = torch.randn(2 * n, h, w, c, device="cuda")
    keep = x.clone()
    lw = torch.rand(c, device="cuda")
    slots = ops.lpips_tap_slots(h, w, c)
    assert slots == 1
    ws = torch.full((n * slots,), -7.0, dtype=torch.float64, device="cuda")
    pooled = torch.full((2 * n, h // 2, w // 2, c), -7.0, device="cuda")
    tap = lambda cc=c, nbytes=ws.numel() * 8, feat=x.data_ptr(), s0=0: lib.mvldm_lpips_tap(feat, lw.data_ptr(), pooled.data_ptr(), n, h, w, cc, L.F32,
                                                                                          ws.data_ptr(), nbytes, s0, slots, ops.stream())
    assert tap(cc=96) < 0 and b"multiples of 64" in lib.mvldm_last_error()
    assert tap(cc=576) < 0
    assert tap(nbytes=ws.numel() * 8 - 8) < 0 and b"workspace" in lib.mvldm_last_error()
    assert tap(s0=1) < 0 and b"partials" in lib.mvldm_last_error()
    assert tap(feat=None) < 0 and b"null" in lib.mvldm_last_error()
    assert lib.mvldm_lpips_relu(x.data_ptr(), x.numel() - 1, L.F32, ops.stream()) < 0
    out = torch.full((n,), -7.0, device="cuda")
    im = torch.rand(n, 3, 15, 64, device="cuda")
    dst = torch.full((2 * n, 15, 64, 4), -7.0, device="cuda")
    assert lib.mvldm_lpips_prep(im.data_ptr(), im.data_ptr(), dst.data_ptr(), n, 15, 64, 4, L.F32, 1, ops.stream()) < 0 and b"pool" in lib.mvldm_last_error()
    assert lib.mvldm_lpips_fold(ws.data_ptr(), ws.numel() * 8, n, 64, 64, out.data_ptr(), ops.stream()) < 0 and b"workspace" in lib.mvldm_last_error()
    torch.cuda.synchronize()
    assert bool((ws == -7).all()) and bool((pooled == -7).all()) and bool((out == -7).all()) and bool((dst == -7).all()) and torch.equal(x, keep)
    with pytest.raises(L.MvldmError, match="pool"):
        model(im, im)
    with pytest.raises(ValueError, match="contiguous"):
        model(torch.rand(n, 3, 32, 64, device="cuda")[:, :, :, ::2], torch.rand(n, 3, 32, 64, device="cuda")[:, :, :, ::2])
    with pytest.raises(TypeError):
        model(torch.zeros(n, 3, 16, 16, dtype=torch.uint8, device="cuda"), torch.zeros(n, 3, 16, 16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match=r"\[n, 3, h, w\]"):
        model(torch.rand(n, 1, 16, 16, device="cuda"), torch.rand(n, 1, 16, 16, device="cuda"))
    assert tap() == 0                                                # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    nchw = keep.double().permute(0, 3, 1, 2).cpu()
    want = R.tap_distance(nchw[:n], nchw[n:], lw.double().cpu())
    assert float(((ws.cpu() - want).abs() / want).max()) <= TAP_TOL and bool((pooled >= 0).all()) and torch.equal(x, keep)


def test_the_reference_signature_the_view_axis_and_16_bit_images(model):
    from mv_ldm_amd import metrics as M
    gt, pred = R.make_pair("noise05", 6, 24, 31, seed=13)
    gt, pred = gt.cuda(), pred.cuda()
    flat = M.compute_lpips(gt, pred, model)
    assert flat.shape == (6,) and flat.dtype == torch.float32 and torch.equal(flat, model(gt, pred, normalize=True)[:, 0, 0, 0])
    five = M.compute_lpips(gt.view(2, 3, 3, 24, 31), pred.view(2, 3, 3, 24, 31), model)
    assert five.shape == (2, 3) and torch.equal(five.reshape(-1), flat)
    for dt in (torch.float16, torch.bfloat16):                       # 16-bit images go through the elementwise convert: the scores of the rounded images
        lo = M.compute_lpips(gt.to(dt), pred.to(dt), model)
        assert lo.dtype == torch.float32 and torch.equal(lo, M.compute_lpips(gt.to(dt).float(), pred.to(dt).float(), model))


def test_relu_in_place(model):
    from mv_ldm_amd import ops
    for dtype in DTYPES:
        for numel in (8, 1024 * 8, 1024 * 8 * 3 + 8 * 5):             # one chunk, one workgroup's worth, a ragged tail
            x = torch.randn(numel, generator=torch.Generator().manual_seed(numel)).to(dtype).cuda()
            want = x.clone().relu()
            assert ops.lpips_relu(x) is x and torch.equal(x, want)


def test_validation_step_scores_with_the_network_it_is_given(golden, model, monkeypatch):
    from mv_ldm_amd import metrics as M
    from mv_ldm_amd.train import OptimizerCfg
    from test_hip_metrics import _pin, _val_inputs
    from test_hip_train import build_trainer
    from test_oracle_train import g9_case
    _pin(monkeypatch)
    g = golden("g9_training_step")
    batch, _ = g9_case(g, 0)
    kw = _val_inputs()
    with torch.enable_grad():
        tr = build_trainer(g, torch.float32, optimizer_cfg=OptimizerCfg(lr=1e-3))
        plain = tr.validation_step(batch, num_inference_steps=2, **kw)
        out = tr.validation_step(batch, num_inference_steps=2, lpips=model, **kw)
    keys = ["batch", "context", "psnr", "psnr_roundtrip", "sampled", "ssim", "ssim_roundtrip", "targets", "targets_roundtrip"]
    assert sorted(plain) == keys and sorted(out) == sorted([*keys, "lpips", "lpips_roundtrip"])
    assert torch.equal(plain["sampled"], out["sampled"]) and torch.equal(plain["psnr"], out["psnr"]) and torch.equal(plain["ssim"], out["ssim"])
    assert out["lpips"].shape == out["lpips_roundtrip"].shape == (2, 4) and out["lpips"].is_cuda and out["lpips"].dtype == torch.float32
    assert torch.equal(out["lpips"], M.compute_lpips(out["targets"], out["sampled"], model))
    assert torch.equal(out["lpips_roundtrip"], M.compute_lpips(out["targets_roundtrip"], out["sampled"], model))
    assert bool(torch.isfinite(out["lpips"]).all()) and bool((out["lpips"] > 0).all()) and not torch.equal(out["lpips"], out["lpips_roundtrip"])
