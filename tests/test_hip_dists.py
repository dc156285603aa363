"""GPU: DISTS on the device (`csrc/dists.hip`, `mv_ldm_amd.dists.DISTS`, `metrics.compute_dists`) against the fp64 restatement of
tests/dists_ref.py with seeded random weights, and `MVLDMTrainer.validation_step(dists=...)`.

Error of the whole metric: |got - want| / want per image.  The bounds come from the CPU (tests/golden/dists_cpu_emulation.json, written by
tests/golden/make_dists_bounds.py on exactly these inputs), never from the kernels: f32 -- 10 x the worst error of the fp32-trunk
emulation of that pair kind (the margin tests/test_hip_lpips.py gives the MFMA's other summation order through 13 layers); f16 / bf16 --
3 x the worst error of that type's rounding emulation.  The statistics kernel alone: 1e-12 relative on each of the five sums (fp64 sums
of exact products over fewer than 600 terms -- 4270 for the raw image -- so N 2^-53 < 1e-12).  The L2 pool alone: 1e-6 relative in f32
(nine fp32 products, eight adds and one sqrt: about 4e-7), the fp64 value rounded to the type or one of its two neighbours in 16 bit."""
import functools
import json

import pytest
import torch

import dists_ref as R
from conftest import GOLDEN, record_err

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
NAME = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}
MAPS = ((1, 1), (2, 3), (5, 7), (33, 18))
STAT_TOL = 1e-12
POOL_TOL_F32 = 1e-6


@pytest.fixture(scope="module")
def emu():
    return json.loads((GOLDEN / "dists_cpu_emulation.json").read_text())


@functools.lru_cache(maxsize=None)
def _weights():
    return R.make_weights(R.WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def _want(kind, n, h, w):
    """the fp64 restatement of one small case, computed once for the three dtypes"""
    gt, pred = R.make_pair(kind, n, h, w, seed=R.case_seed(n, h, w))
    return R.dists(gt, pred, _weights())


@pytest.fixture(scope="module")
def model():
    from mv_ldm_amd.dists import DISTS
    return DISTS(weights=_weights()).cuda()


def bound(emu, dtype, kind):
    return (10.0 if dtype == torch.float32 else 3.0) * emu["worst_rel_err"][NAME[dtype]][kind]


def _maps(n, h, w, c, dtype, seed):
    """pre-activation NHWC [2n, h, w, c] in `dtype`, about half the entries negative"""
    return torch.randn(2 * n, h, w, c, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _check_sums(part, want, what):
    """part [n, slots, 5, c] fp64 partials, want [n, 5, c]"""
    got = part.sum(dim=1)
    assert bool(torch.isfinite(got).all())
    assert bool(((got - want).abs() <= STAT_TOL * want.abs()).all()), what
    return float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())


# ---- the statistics kernel alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("c", [64, 128, 256, 512])
def test_the_five_sums_of_a_stage(c, dtype):
    from mv_ldm_amd import ops
    worst = 0.0
    for (h, w) in MAPS:
        for n in (1, 3):
            x = _maps(n, h, w, c, dtype, seed=c + 31 * h + n)
            slots = ops.dists_stat_slots(h, w, c)
            assert slots == -(-(h * w) // max(256, 32768 // c))
            per = ops.DISTS_SUMS * c
            ws = torch.zeros(n * (slots + 2) * per * 8, dtype=torch.uint8, device="cuda")     # one unused slot on either side
            ops.dists_stats(x.cuda(), ws, per, (slots + 2) * per)
            part = ws.view(torch.float64).view(n, slots + 2, ops.DISTS_SUMS, c).cpu()
            assert bool((part[:, 0] == 0).all()) and bool((part[:, -1] == 0).all())
            nchw = x.double().permute(0, 3, 1, 2).relu()                                      # the rounded inputs, in fp64
            assert bool((x < 0).any())
            worst = max(worst, _check_sums(part[:, 1:-1], R.five_sums(nchw[:n], nchw[n:]), (c, dtype, h, w, n)))
    print(f"stats C={c} {NAME[dtype]}: worst rel err {record_err(f'dists_stats_rel/{NAME[dtype]}', worst):.3e}")


def test_the_five_sums_of_the_raw_image():
    from mv_ldm_amd import ops
    worst = 0.0
    for (h, w) in (*MAPS, (70, 61)):                                                          # 4270 pixels: two workgroups
        for n in (1, 3):
            g = torch.Generator().manual_seed(h * 100 + w + n)
            x, y = torch.rand(n, 3, h, w, generator=g), torch.rand(n, 3, h, w, generator=g)
            slots = ops.dists_stat_slots(h, w, 3)
            assert slots == -(-(h * w) // 4096)
            per = ops.DISTS_SUMS * 3
            ws = torch.zeros(n * (slots + 2) * per * 8, dtype=torch.uint8, device="cuda")
            ops.dists_stats(x.cuda(), ws, per, (slots + 2) * per, feat_b=y.cuda())
            part = ws.view(torch.float64).view(n, slots + 2, ops.DISTS_SUMS, 3).cpu()
            assert bool((part[:, 0] == 0).all()) and bool((part[:, -1] == 0).all())
            worst = max(worst, _check_sums(part[:, 1:-1], R.five_sums(x, y), (h, w, n)))
    print(f"stats of the raw image: worst rel err {record_err('dists_stats_rel/raw', worst):.3e}")


# ---- the L2 pool alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("c", [64, 128, 256, 512])
def test_l2pool_values_shape_and_confined_writes(c, dtype):
    from mv_ldm_amd import _lib as L, ops
    lib, pad, worst = L.load(), 64, 0.0
    for (h, w) in MAPS:
        for n in (1, 3):
            x = _maps(n, h, w, c, dtype, seed=7 * c + 31 * h + n)
            x[0, 0, 0, : c // 2] = -x[0, 0, 0, : c // 2].abs()                               # dead entries: where the window holds nothing else,
            oh, ow = (h + 1) // 2, (w + 1) // 2                                               # sqrt(1e-12) = 1e-6, an f16 subnormal
            assert tuple(ops.dists_l2pool(x.cuda()).shape) == (2 * n, oh, ow, c)
            numel = 2 * n * oh * ow * c
            buf = torch.full((numel + 2 * pad,), -7.0, dtype=dtype, device="cuda")            # sentinels on both sides of the output
            xd = x.cuda()
            L.check(lib.mvldm_dists_l2pool(xd.data_ptr(), buf.data_ptr() + pad * buf.element_size(), n, h, w, c, ops.dt(dtype), ops.stream()))
            assert bool((buf[:pad] == -7).all()) and bool((buf[-pad:] == -7).all())
            got = buf[pad:-pad].view(2 * n, oh, ow, c).cpu()
            assert torch.equal(got, ops.dists_l2pool(xd).cpu())
            want = R.l2pool(x.double().permute(0, 3, 1, 2).relu()).permute(0, 2, 3, 1)
            assert bool((want >= 1e-6 * (1 - 1e-9)).all())
            if dtype == torch.float32:
                e = float(((got.double() - want).abs() / want).max())
                worst = max(worst, e)
                assert e <= POOL_TOL_F32, (c, h, w, n, e)
            else:                                                                             # positive values: the bit patterns are ordered
                steps = (got.view(torch.int16).int() - want.to(dtype).view(torch.int16).int()).abs()
                worst = max(worst, float(steps.max()))
                assert int(steps.max()) <= 1, (c, dtype, h, w, n)
                if dtype == torch.float16 and h * w == 1:                                    # the dead half of a 1 x 1 map: 1e-6, 17 subnormal steps
                    assert bool((got[0, 0, 0, : c // 2].view(torch.int16) == 17).all())
    print(f"l2pool C={c} {NAME[dtype]}: worst {record_err(f'dists_l2pool/{NAME[dtype]}', worst):.3e} ({'rel err' if dtype == torch.float32 else 'steps'})")


# ---- the whole metric -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("n,h,w", R.CASES, ids=lambda v: str(v))
def test_parity_with_the_fp64_restatement(n, h, w, dtype, model, emu):
    for kind in (R.KINDS if dtype == torch.float32 else (*R.KINDS_16BIT, "identical")):
        gt, pred = R.make_pair(kind, n, h, w, seed=R.case_seed(n, h, w))
        got = model(gt.cuda(), pred.cuda(), dtype=dtype)
        assert got.shape == (n,) and got.dtype == torch.float32 and got.is_cuda
        got = got.double().cpu()
        if kind == "identical":
            assert torch.equal(got, torch.zeros(n, dtype=torch.float64)), (kind, got)
            continue
        want = torch.tensor(emu["want"][R.case_key(kind, n, h, w)], dtype=torch.float64)
        if h * w <= 64 * 64:                                         # the small cases are recomputed, 256 x 256 is the recorded fp64 score
            assert torch.allclose(_want(kind, n, h, w), want, rtol=1e-9, atol=0)
            want = _want(kind, n, h, w)
        e = record_err(f"dists_rel/{NAME[dtype]}/{kind}", float(((got - want).abs() / want).max()))
        print(f"{n}x3x{h}x{w} {NAME[dtype]} {kind}: rel err {e:.3e}, bound {bound(emu, dtype, kind):.3e} (dists {float(want.mean()):.4e})")
        assert e <= bound(emu, dtype, kind), (kind, e, bound(emu, dtype, kind))


def test_symmetry(model):
    gt, pred = R.make_pair("noise05", 3, 37, 45, seed=1)
    gt, pred = gt.cuda(), pred.cuda()
    ab, ba = model(gt, pred), model(pred, gt)
    assert torch.equal(ab, ba) and bool((ab > 0).all())              # every term is symmetric in a and b: the same bits either way round


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_launches_are_bit_identical(dtype, model):
    gt, pred = R.make_pair("random", 3, 37, 45, seed=2)
    a = model(gt.cuda(), pred.cuda(), dtype=dtype)
    b = model(gt.cuda(), pred.cuda(), dtype=dtype)
    assert torch.equal(a, b) and bool((a > 0).all()) and len(set(a.tolist())) == 3


def test_an_image_scores_the_same_alone_elsewhere_and_in_chunks(model, emu, monkeypatch):
    """the conv tile may differ with the batch size, so not bit for bit: within the f32 bound of the batched value"""
    monkeypatch.setenv("MVLDM_AUTOTUNE", "0")
    kind, tol = "noise05", bound(emu, torch.float32, "noise05")
    gt, pred = R.make_pair(kind, 5, 37, 45, seed=3)
    gt, pred = gt.cuda(), pred.cuda()
    full = model(gt, pred)
    rel = lambda a, b: float(((a - b).abs() / b).max())
    for i in range(5):
        assert rel(model(gt[i:i + 1], pred[i:i + 1]), full[i:i + 1]) <= tol, i
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    assert rel(model(gt[perm][:4].contiguous(), pred[perm][:4].contiguous()), full[perm][:4]) <= tol
    # chunks of 2 + 2 + 1 pairs (what the 2 GiB rule does to a large batch) through one workspace
    monkeypatch.setattr(type(model), "chunk_pairs", staticmethod(lambda h, w, dtype: 2))
    assert rel(model(gt, pred), full) <= tol
    monkeypatch.undo()
    assert type(model).chunk_pairs(256, 256, torch.float32) == 64 and type(model).chunk_pairs(256, 256, torch.float16) == 128


def test_a_captured_launch_scores_the_new_contents_of_its_buffers(model):
    from mv_ldm_amd import ops
    n, h, w = 3, 37, 45
    a0, b0 = R.make_pair("noise05", n, h, w, seed=17)
    a1, b1 = R.make_pair("random", n, h, w, seed=19)
    gt, pred = a0.cuda(), b0.cuda()
    out = torch.empty(n, device="cuda")
    ws = torch.empty(ops.dists_workspace_bytes(n, h, w), dtype=torch.uint8, device="cuda")
    want0 = model(gt, pred).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model(gt, pred, out=out, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                    # one stream: a single-branch graph
        model(gt, pred, out=out, ws=ws)
    graph.replay()
    assert torch.equal(out, want0)
    gt.copy_(a1)
    pred.copy_(b1)
    graph.replay()
    want1 = model(a1.cuda(), b1.cuda())
    assert torch.equal(out, want1) and not torch.equal(want0, want1)


def test_refusals_return_a_status_and_launch_nothing(model):
    from mv_ldm_amd import _lib as L, ops
    lib = L.load()
    n, h, w, c = 2, 8, 8, 64
    x = torch.randn(2 * n, h, w, c, device="cuda")
    keep = x.clone()
    slots, per = ops.dists_stat_slots(h, w, c), ops.DISTS_SUMS * c
    assert slots == 1
    ws = torch.full((n * slots * per,), -7.0, dtype=torch.float64, device="cuda")
    pooled = torch.full((2 * n, h // 2, w // 2, c), -7.0, device="cuda")
    stats = lambda cc=c, nbytes=ws.numel() * 8, feat=x.data_ptr(), fb=None, off=0, hh=h: lib.mvldm_dists_stats(
        feat, fb, n, hh, w, cc, L.F32, ws.data_ptr(), nbytes, off, slots * per, ops.stream())
    pool = lambda cc=c, feat=x.data_ptr(), dst=pooled.data_ptr(), hh=h: lib.mvldm_dists_l2pool(feat, dst, n, hh, w, cc, L.F32, ops.stream())
    assert stats(cc=96) < 0 and b"multiples of 64" in lib.mvldm_last_error()
    assert stats(cc=576) < 0 and pool(cc=96) < 0 and pool(cc=3) < 0
    assert stats(nbytes=ws.numel() * 8 - 8) < 0 and b"workspace" in lib.mvldm_last_error()
    assert stats(off=1) < 0 and b"partials" in lib.mvldm_last_error()
    assert stats(feat=None) < 0 and b"null" in lib.mvldm_last_error()
    assert stats(feat=x.data_ptr() + 4) < 0 and b"unaligned" in lib.mvldm_last_error()
    assert stats(fb=x.data_ptr()) < 0 and b"second pointer" in lib.mvldm_last_error()
    assert stats(hh=0) < 0 and pool(hh=0) < 0
    assert pool(dst=None) < 0 and b"null" in lib.mvldm_last_error()
    out = torch.full((n,), -7.0, device="cuda")
    ab = torch.rand(1475, device="cuda")
    im = torch.rand(n, 3, 16, 16, device="cuda")
    dst = torch.full((2 * n, 16, 16, 4), -7.0, device="cuda")
    assert lib.mvldm_dists_prep(im.data_ptr(), im.data_ptr(), dst.data_ptr(), n, 16, 16, 8, L.F32, ops.stream()) < 0 and b"c_pad" in lib.mvldm_last_error()
    assert lib.mvldm_dists_prep(im.data_ptr(), None, dst.data_ptr(), n, 16, 16, 4, L.F32, ops.stream()) < 0
    assert lib.mvldm_dists_fold(ws.data_ptr(), ws.numel() * 8, n, 64, 64, ab.data_ptr(), ab.data_ptr(), out.data_ptr(), ops.stream()) < 0 \
        and b"workspace" in lib.mvldm_last_error()
    torch.cuda.synchronize()
    assert bool((ws == -7).all()) and bool((pooled == -7).all()) and bool((out == -7).all()) and bool((dst == -7).all()) and torch.equal(x, keep)
    with pytest.raises(NotImplementedError):
        model(im, im, require_grad=True)
    with pytest.raises(NotImplementedError):
        model(im, im, batch_average=True)
    with pytest.raises(ValueError, match="contiguous"):
        model(torch.rand(n, 3, 32, 64, device="cuda")[:, :, :, ::2], torch.rand(n, 3, 32, 64, device="cuda")[:, :, :, ::2])
    with pytest.raises(TypeError):
        model(torch.zeros(n, 3, 16, 16, dtype=torch.uint8, device="cuda"), torch.zeros(n, 3, 16, 16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match=r"\[n, 3, h, w\]"):
        model(torch.rand(n, 1, 16, 16, device="cuda"), torch.rand(n, 1, 16, 16, device="cuda"))
    assert stats() == 0 and pool() == 0                              # and the same calls with nothing wrong run
    torch.cuda.synchronize()
    nchw = keep.double().permute(0, 3, 1, 2).relu().cpu()
    _check_sums(ws.view(n, slots, ops.DISTS_SUMS, c).cpu(), R.five_sums(nchw[:n], nchw[n:]), "after the refusals")
    assert bool((pooled > 0).all()) and torch.equal(x, keep)


def test_the_reference_signature_the_view_axis_and_16_bit_images(model):
    from mv_ldm_amd import metrics as M
    gt, pred = R.make_pair("noise05", 6, 24, 31, seed=13)
    gt, pred = gt.cuda(), pred.cuda()
    flat = M.compute_dists(gt, pred, model)
    assert flat.shape == (6,) and flat.dtype == torch.float32 and torch.equal(flat, model(gt, pred))
    one = M.compute_dists(gt[:1], pred[:1], model)
    assert one.shape == (1,)                                         # always 1-d: no squeeze to 0-d for a single pair
    five = M.compute_dists(gt.view(2, 3, 3, 24, 31), pred.view(2, 3, 3, 24, 31), model)
    assert five.shape == (2, 3) and torch.equal(five.reshape(-1), flat)
    for dt in (torch.float16, torch.bfloat16):                       # 16-bit images go through the elementwise convert: the scores of the rounded images
        lo = M.compute_dists(gt.to(dt), pred.to(dt), model)
        assert lo.dtype == torch.float32 and torch.equal(lo, M.compute_dists(gt.to(dt).float(), pred.to(dt).float(), model))


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
        out = tr.validation_step(batch, num_inference_steps=2, dists=model, **kw)
    keys = ["batch", "context", "psnr", "psnr_roundtrip", "sampled", "ssim", "ssim_roundtrip", "targets", "targets_roundtrip"]
    assert sorted(plain) == keys and sorted(out) == sorted([*keys, "dists", "dists_roundtrip"])
    for k in keys:                                                   # every other entry: the same bits
        if torch.is_tensor(plain[k]):
            assert torch.equal(plain[k], out[k]), k
    assert out["dists"].shape == out["dists_roundtrip"].shape == (2, 4) and out["dists"].is_cuda and out["dists"].dtype == torch.float32
    assert torch.equal(out["dists"], M.compute_dists(out["targets"], out["sampled"], model))
    assert torch.equal(out["dists_roundtrip"], M.compute_dists(out["targets_roundtrip"], out["sampled"], model))
    assert bool(torch.isfinite(out["dists"]).all()) and bool((out["dists"] > 0).all()) and not torch.equal(out["dists"], out["dists_roundtrip"])
