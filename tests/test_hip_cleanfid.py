"""GPU: Clean-FID on the device (`csrc/inception.hip`, `mv_ldm_amd.cleanfid`) against PIL's own resize (tests/golden/cleanfid_resize.npz)
and the fp64 restatement of tests/cleanfid_ref.py with seeded random weights.

Error of a score: |got - want| / (|mu1 - mu2|^2 + tr Sigma1 + tr Sigma2), as in tests/test_hip_fid.py.  Error of a feature or a map entry:
|got - want| / the RMS of that image's vector or map.  The bounds come from the CPU (tests/golden/cleanfid_cpu_emulation.json, written by
tests/golden/make_cleanfid_bounds.py on exactly these inputs), never from the kernels: f32 -- 10 x the worst error of the fp32 emulation
(the margin tests/test_hip_lpips.py gives the MFMA's other summation order); f16 / bf16 -- 3 x the worst error of that type's rounding
emulation; the solve alone -- 10 x the worst error of the numpy emulation of the kernels' rotation order on that class of states, and at
d = 2048 (where the emulation would run for an hour) the larger of that at d = 192 and the case's own distance between the symmetric and
the scipy-sqrtm route.  The whole-extractor scores are expected in the factored form (`frechet_factored`), which has no null-space
round-off.  Means and states: 1e-12 relative (fp64 sums of fewer than 5.4 k exact terms)."""
import functools
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cleanfid_ref as R
from conftest import GOLDEN, record_err

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
NAME = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}
MANT = {torch.float32: (23, -126), torch.float16: (10, -14), torch.bfloat16: (7, -126)}       # mantissa bits, least normal exponent
SUM_TOL = 1e-12
SENTINEL = -7.0


@pytest.fixture(scope="module")
def emu():
    return json.loads((GOLDEN / "cleanfid_cpu_emulation.json").read_text())


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLDEN / "cleanfid_features.npz", allow_pickle=False)


@pytest.fixture(scope="module")
def model():
    from mv_ldm_amd.cleanfid import InceptionPool3
    return InceptionPool3(weights=R.make_weights()).cuda()


@pytest.fixture(scope="module")
def metric(model):
    from mv_ldm_amd.cleanfid import CleanFID
    return CleanFID(model)


def margin(dtype):
    return 10.0 if dtype == torch.float32 else 3.0


def _ulp(v, dtype):
    """the spacing of `dtype` at |v| (fp64 tensor)"""
    mant, emin = MANT[dtype]
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def _guarded(numel, dtype, pad=64):
    """a sentinel-filled buffer and the view of its middle"""
    buf = torch.full((numel + 2 * pad,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[pad:pad + numel]


def _untouched(buf, numel, pad=64):
    return bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + numel:] == SENTINEL).all())


def _rel_rms(got, want):
    n = want.shape[0]
    g, w = got.double().reshape(n, -1), want.double().reshape(n, -1)
    return float(((g - w).abs().amax(1) / w.pow(2).mean(1).sqrt()).max())


# ---- prep alone ---------------------------------------------------------------------------------------------------------------------
def _prep_raw(src, oh, ow, dtype):
    """mvldm_inception_prep into the middle of sentinel-filled buffers (output and workspace): NHWC [n, oh, ow, c_pad] on the host"""
    from mv_ldm_amd import _lib as L, ops
    n, _, h, w = src.shape
    cp = ops.epc(dtype)
    buf, mid = _guarded(n * oh * ow * cp, dtype)
    need = ops.inception_workspace_bytes(n, h, ow)
    assert need == n * 3 * h * ow * 4
    wbuf, wmid = _guarded(need // 4, torch.float32)
    L.check(L.load().mvldm_inception_prep(src.data_ptr(), int(src.dtype == torch.uint8), mid.data_ptr(), n, h, w, oh, ow, cp, ops.dt(dtype),
                                          wmid.data_ptr(), need, ops.stream()))
    assert _untouched(buf, mid.numel()) and _untouched(wbuf, wmid.numel())
    got = mid.view(n, oh, ow, cp)
    assert torch.equal(got, ops.inception_prep(src, dtype, oh, ow))
    return got.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("h,w,oh,ow", R.RESIZE_CASES, ids=str)
def test_prep_resizes_like_pil(h, w, oh, ow, dtype):
    """PIL's own output, clipped and centred as the package does it, in fp32 ((v - 128) / 128 of a float32 v: the subtraction rounds to
    the spacing of v - 128, up to 2^-17, so the fp64 value of the expression is NOT what the package feeds its network): f32 within one
    float32 step of max(|v|, 1) / 128 (the kernel does PIL's double sums in PIL's order, so only a contraction could move a rounding), 16
    bit within one step of that type"""
    g = np.load(GOLDEN / "cleanfid_resize.npz", allow_pickle=False)
    src = torch.from_numpy(g[f"src_{h}x{w}_{oh}x{ow}"])
    pil = torch.from_numpy(g[f"out_{h}x{w}_{oh}x{ow}"])
    assert pil.dtype == torch.float32
    want = ((pil.clamp(0, 255) - 128) / 128).permute(0, 2, 3, 1).double()
    pil = pil.double()
    got_u8 = _prep_raw(src.cuda(), oh, ow, dtype)
    flt = (src.float() / 255).contiguous()
    assert torch.equal(flt * 255, src.float())                                    # the float image holds the same bytes
    got = _prep_raw(flt.cuda(), oh, ow, dtype)
    assert torch.equal(got, got_u8)
    assert bool((got[..., 3:] == 0).all())                                        # padding channels exactly 0
    err = (got[..., :3].double() - want).abs()
    if dtype == torch.float32:
        step = _ulp(pil.clamp(0, 255).permute(0, 2, 3, 1).abs().clamp_min(1.0), torch.float32) / 128
    else:
        step = _ulp(torch.maximum(want.abs(), got[..., :3].double().abs()), dtype)
    e = record_err(f"cleanfid_prep/{NAME[dtype]}_steps", float((err / step).max()))
    print(f"prep {h}x{w} -> {oh}x{ow} {NAME[dtype]}: worst {e:.3f} steps")
    assert e <= 1.0, e
    if (h, w) == (oh, ow):
        assert torch.equal(got[..., :3].double(), want) or dtype != torch.float32


# ---- unfold + conv ------------------------------------------------------------------------------------------------------------------
def _nhwc(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("k,pad", R.CONV_KERNELS, ids=str)
def test_unfold_and_the_oblong_convolutions(k, pad, dtype, emu):
    from mv_ldm_amd import _lib as L, cleanfid, ops
    kh, kw = k
    for hw in R.CONV_MAPS[k]:
        x, w, b = R.conv_case(k, hw)
        n, c, (h, wd) = R.CONV_N, R.CONV_CIN, hw
        xs = _nhwc(x, dtype)
        # the unfold alone, into a guarded buffer: exactly the gather, zeros outside the map
        buf, mid = _guarded(n * h * wd * kh * kw * c, dtype)
        L.check(L.load().mvldm_inception_unfold(xs.data_ptr(), mid.data_ptr(), n, h, wd, c, kh, kw, pad[0], pad[1], ops.dt(dtype), ops.stream()))
        assert _untouched(buf, mid.numel())
        xp = F.pad(xs.cpu().float(), (0, 0, pad[1], pad[1], pad[0], pad[0]))
        gather = torch.stack([xp[:, dy:dy + h, dx:dx + wd, :] for dy in range(kh) for dx in range(kw)], dim=3).reshape(n, h, wd, kh * kw * c)
        assert torch.equal(mid.view(n, h, wd, -1).cpu().float(), gather)
        assert torch.equal(ops.inception_unfold(xs, kh, kw), mid.view(n, h, wd, -1))
        if hw != (9, 11):
            assert bool((gather == 0).any(-1).all())                              # every window hits the padding
        # the convolution through it
        got = cleanfid.conv(xs, cleanfid.pack_conv(w.cuda(), dtype), b.cuda(), k, 1, pad)
        assert tuple(got.shape) == (n, h, wd, R.CONV_NOUT) and got.dtype == dtype
        want = R.conv_want(x, w, b, pad).permute(0, 2, 3, 1)
        e = record_err(f"cleanfid_conv/{NAME[dtype]}", _rel_rms(got.cpu(), want))
        bound = margin(dtype) * emu["conv_err"][NAME[dtype]]
        print(f"conv {k} on {hw} {NAME[dtype]}: err {e:.3e}, bound {bound:.3e}")
        assert e <= bound, (k, hw, e, bound)


# ---- pools and concat ---------------------------------------------------------------------------------------------------------------
def _into_slice(fn, n, oh, ow, c, dtype, ld, off):
    """run fn(dst pointer) on a guarded [n, oh, ow, ld] buffer of sentinels; returns the slice, after checking everything else stayed"""
    buf, mid = _guarded(n * oh * ow * ld, dtype)
    fn(mid.view(n, oh, ow, ld))
    assert _untouched(buf, mid.numel())
    out = mid.view(n, oh, ow, ld).cpu()
    keep = torch.ones(ld, dtype=torch.bool)
    keep[off:off + c] = False
    assert bool((out[..., keep] == SENTINEL).all())                               # the columns outside the slice are untouched
    return out[..., off:off + c]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("c", [16, 288])
def test_pools_write_their_slice(c, dtype):
    from mv_ldm_amd import ops
    ld, off, n = c + 48, 32, 2
    for kind, (h, w), stride, pad in (("max", (8, 9), 2, 0), ("max", (3, 3), 2, 0), ("max", (3, 3), 1, 1), ("max", (5, 4), 1, 1),
                                      ("avg", (3, 3), 1, 1), ("avg", (5, 7), 1, 1)):
        g = torch.Generator().manual_seed(c + 10 * h + w)
        x = torch.randn(n, c, h, w, generator=g)
        if kind == "max" and pad == 1:
            x = -x.abs() - 0.01                                                   # all negative: the padding must not win
        x = x.to(dtype).float()
        xs = _nhwc(x, dtype)
        oh, ow = (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1
        if kind == "max":
            got = _into_slice(lambda dst: ops.inception_maxpool(xs, stride, pad, dst, off), n, oh, ow, c, dtype, ld, off)
            want = F.max_pool2d(x, 3, stride, pad).permute(0, 2, 3, 1)
            assert (oh, ow) == tuple(want.shape[1:3]) and ((h, w) != (8, 9) or (oh, ow) == (3, 4))
            assert torch.equal(got.float(), want), (kind, h, w, stride, pad)
            assert torch.equal(ops.inception_maxpool(xs, stride, pad).cpu(), got)
        else:
            got = _into_slice(lambda dst: ops.inception_avgpool(xs, dst, off), n, oh, ow, c, dtype, ld, off)
            want = F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=False).permute(0, 2, 3, 1)
            if (h, w) == (3, 3):                                                  # every pixel is a border pixel: divisors 4, 6, 9
                assert torch.equal(want[:, 0, 0], x.double()[:, :, :2, :2].sum((2, 3)) / 4) and torch.equal(want[:, 1, 1], x.double().sum((2, 3)) / 9)
            steps = (got.double() - want).abs() / _ulp(torch.maximum(want.abs(), got.double().abs()), dtype)
            e = record_err(f"cleanfid_avgpool/{NAME[dtype]}_steps", float(steps.max()))
            assert e <= 2.0, (h, w, e)
    # concat: a copy, with and without ReLU
    x = torch.randn(n, 5, 7, c).to(dtype).cuda()
    for relu in (False, True):
        got = _into_slice(lambda dst: ops.inception_concat(x, dst, off, relu), n, 5, 7, c, dtype, ld, off)
        assert torch.equal(got, (x.relu() if relu else x).cpu())


# ---- features / accumulate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_features_are_the_fp64_mean(dtype):
    from mv_ldm_amd import ops
    worst = 0.0
    for (h, w) in ((8, 8), (1, 1), (3, 5)):
        x = torch.randn(3, h, w, 2048, generator=torch.Generator().manual_seed(h + w)).relu().to(dtype)
        buf, mid = _guarded(3 * 2048, torch.float64)
        ops.inception_features(x.cuda(), mid.view(3, 2048))
        assert _untouched(buf, mid.numel())
        want = x.double().mean((1, 2))
        got = mid.view(3, 2048).cpu()
        assert bool(((got - want).abs() <= SUM_TOL * want.abs()).all()), (h, w)
        worst = max(worst, float(((got - want).abs() / want.abs().clamp_min(1e-300)).max()))
    record_err(f"cleanfid_features_mean/{NAME[dtype]}", worst)


@pytest.mark.parametrize("d", [128, 2048])
def test_accumulate_adds_rows_in_order(d):
    from mv_ldm_amd import ops
    size = ops.frechet_state_size(d)
    f = torch.rand(5, d, dtype=torch.float64, generator=torch.Generator().manual_seed(d)) * 3

    def run(parts):
        buf, st = _guarded(size, torch.float64)
        st.zero_()
        for p in parts:
            ops.frechet_accumulate(p.cuda().contiguous(), st)
        assert _untouched(buf, size)
        return st.cpu()

    worst = 0.0
    for n in (1, 5):
        got, want = run([f[:n]]), R.state(f[:n])
        assert float(got[0]) == n
        assert bool(((got - want).abs() <= SUM_TOL * want.abs()).all())
        worst = max(worst, float(((got - want).abs() / want.abs()).max()))
        assert torch.equal(got, run([f[:n]]))                                     # the same bits every time
    split, whole = run([f[:2], f[2:]]), run([f])
    assert float(split[0]) == 5 and bool(((split - whole).abs() <= SUM_TOL * whole.abs()).all())
    record_err(f"cleanfid_accumulate/{d}", worst)


# ---- the solve alone ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthetic(d):
    return R.synthetic_cases(d)


def _compute(s1, s2, ws=None):
    from mv_ldm_amd import ops
    out = torch.full((1,), SENTINEL, device="cuda")
    info = torch.full((ops.FID_INFO,), SENTINEL, dtype=torch.float64, device="cuda")
    ops.frechet_compute(s1.cuda(), s2.cuda(), out, info, ws)
    return out.cpu(), info.cpu()


def _check_solve(name, d, emu, bound, repeat):
    from mv_ldm_amd import ops
    cls, s1, s2, c = _synthetic(d)[name]
    rec = emu["solve"]["cases"][f"{name}/{d}"]
    sc = R.scale(s1, s2) if d <= 192 else rec["scale"]
    want = (sc - 2 * c) if c is not None else (R.frechet_sym(s1, s2) if d <= 192 else rec["want"])
    assert rec["class"] == cls and abs(want - rec["want"]) <= 1e-6 * sc           # the same inputs (the null eigenvalues' noise differs between hosts)
    need = ops.frechet_workspace_bytes(d)
    wbuf, ws = _guarded(need // 8, torch.float64)
    out, info = _compute(s1, s2, ws)
    assert _untouched(wbuf, need // 8)
    got = float(info[5])
    e = record_err(f"cleanfid_solve/{d}/{cls}", abs(got - want) / sc)
    print(f"solve {name}/{d} ({cls}): err {e:.3e}, bound {bound:.3e}; sweeps {int(info[0])} + {int(info[2])}, residual {float(info[1]):.1e}, "
          f"{float(info[3]):.1e}; fid {got:.6e} of scale {sc:.3e}")
    assert not bool(torch.isnan(out).any()) and int(info[4]) == 0
    assert 0 < int(info[0]) < R.SWEEP_CAP and 0 < int(info[2]) < R.SWEEP_CAP
    assert float(info[1]) <= R.solve_tol(d) and float(info[3]) <= R.solve_tol(d)
    assert e <= bound, (name, d, e, bound)
    assert float(out) == float(torch.tensor(got, dtype=torch.float64).float())
    assert abs(float(info[7]) - sc) <= 1e-12 * sc
    if repeat:
        out2, info2 = _compute(s1, s2)                                            # repeated launches: the same bits
        assert torch.equal(out, out2) and torch.equal(info, info2)


@pytest.mark.parametrize("d", [128, 192])
@pytest.mark.parametrize("name", ["analytic", "full", "deficient", "deficient_vs_full", "identical", "identical_deficient"])
def test_solve_from_synthetic_states(name, d, emu):
    cls = _synthetic(d)[name][0]
    _check_solve(name, d, emu, 10.0 * emu["solve"]["worst"][str(d)][cls], repeat=True)


@pytest.mark.parametrize("name", ["analytic", "deficient"])
def test_solve_at_2048(name, emu):
    cls = _synthetic(2048)[name][0]
    bound = max(10.0 * emu["solve"]["worst"]["192"][cls], emu["solve"]["cases"][f"{name}/2048"]["sym_vs_pkg"])
    _check_solve(name, 2048, emu, bound, repeat=False)


def test_solve_refuses_on_the_device_what_the_host_cannot_see():
    """fewer than 2 samples in a state: NaN, as the package divides by n - 1 (the module refuses before the launch, from host counters)"""
    out, _ = _compute(R.random_state(1, 128, 3), R.random_state(5, 128, 4))
    assert bool(torch.isnan(out).all())


# ---- the whole extractor ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("n_real,n_fake,h,w", R.CASES, ids=lambda v: str(v))
def test_features_and_maps_are_the_restatement(n_real, n_fake, h, w, dtype, model, emu, ref):
    key = R.case_key("other", n_real, n_fake, h, w)
    real, fake = R.case_sets("other", n_real, n_fake, h, w)
    imgs = torch.cat([real, fake]).cuda()
    got, maps = model.features(imgs, dtype=dtype, return_maps=R.MAPS)
    assert got.shape == (n_real + n_fake, 2048) and got.dtype == torch.float64 and got.is_cuda and sorted(maps) == sorted(R.MAPS)
    want = torch.from_numpy(np.concatenate([ref[f"{key}/real"], ref[f"{key}/fake"]]))
    for name in R.MAPS:                                                           # in forward order: a wrong branch is found where it happens
        m = maps[name].permute(0, 3, 1, 2)
        sample = m.reshape(m.shape[0], -1)[:, R.map_sample(name, m.shape[1:]).cuda()].cpu()
        e = record_err(f"cleanfid_map/{NAME[dtype]}/{name}", _rel_rms(sample, torch.from_numpy(ref[f"{key}/{name}"])))
        bound = margin(dtype) * emu["map_err"][NAME[dtype]][name]
        print(f"{key} {NAME[dtype]} {name} {tuple(m.shape)}: err {e:.3e}, bound {bound:.3e}")
        assert e <= bound, (name, e, bound)
    e = record_err(f"cleanfid_features/{NAME[dtype]}", _rel_rms(got.cpu(), want))
    bound = margin(dtype) * emu["feature_err"][NAME[dtype]]
    print(f"{key} {NAME[dtype]} features: err {e:.3e}, bound {bound:.3e}")
    assert e <= bound, (e, bound)
    if dtype == torch.float32 and h == 64:
        assert torch.equal(model.features(imgs), got)                             # the module's dtype is the default; no maps: the tensor alone


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("n_real,n_fake,h,w", R.CASES, ids=lambda v: str(v))
def test_score_is_the_restatement(n_real, n_fake, h, w, dtype, metric, emu):
    """The expectation is the restatement's score in its factored form (`cleanfid_ref.frechet_factored`: the singular values of an
    n1 x n2 matrix), not numpy's eigh-twice route: on these states of 3 + 3 and 2 + 2 images against 2048 features that route carries
    1.1e-6 of the scale of null-space round-off (`sym_vs_factored` in the bounds file) -- eight times the f32 bound -- while the device's
    solve sits at the factored value.  Both sides of the bound (emulation and expectation) go through the factored form."""
    for pair in R.PAIRS:
        key = R.case_key(pair, n_real, n_fake, h, w)
        real, fake = R.case_sets(pair, n_real, n_fake, h, w)
        metric.reset()
        metric.update(real.cuda(), real=True, dtype=dtype)
        metric.update(fake.cuda(), real=False, dtype=dtype)
        out = metric.compute()
        assert out.shape == () and out.dtype == torch.float32 and out.is_cuda
        want, sc = emu["want"][key], emu["scale"][key]
        e = record_err(f"cleanfid_rel/{NAME[dtype]}/{pair}", abs(float(out) - want) / sc)
        bound = margin(dtype) * emu["worst_err"][NAME[dtype]][pair]
        print(f"{key} {NAME[dtype]}: err {e:.3e}, bound {bound:.3e} (fid {want:.4e}, scale {sc:.4e}); sweeps {int(metric.info[0])} + {int(metric.info[2])}")
        assert e <= bound, (pair, e, bound)
        assert int(metric.info[4]) == 0
    metric.reset()


def test_too_few_samples_and_bad_inputs_are_refused(model, metric):
    imgs = R.case_sets("other", 3, 3, 64, 48)[0].cuda()
    metric.reset()
    with pytest.raises(RuntimeError, match="More than one sample"):
        metric.compute()
    with pytest.raises(ValueError, match=r"\[n, 3, h, w\]"):
        metric.update(imgs[:, :1].contiguous(), real=True)
    with pytest.raises(ValueError, match="contiguous"):
        metric.update(imgs[..., ::2], real=True)
    with pytest.raises(TypeError):
        metric.update(imgs.to(torch.int32), real=True)
    with pytest.raises(ValueError, match="return_maps"):
        model.features(imgs, return_maps=("Mixed_9z",))
    assert metric._n == {True: 0, False: 0} and bool((metric.real_state == 0).all())


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_folders_the_command_line_and_a_captured_update(model, metric, tmp_path):
    from mv_ldm_amd import cleanfid
    from mv_ldm_amd.image_io import save_image
    a = R.make_images(3, 20, 28, seed=31)
    b = R.make_images(2, 24, 16, seed=32)
    c = R.make_images(4, 20, 28, seed=33)
    for i, img in enumerate(a):
        save_image(img, tmp_path / "one" / f"{i:03d}.png")
    for i, img in enumerate(b):
        save_image(img, tmp_path / "one" / "nested" / "deeper" / f"{i:03d}.png")
    for i, img in enumerate(c):
        save_image(img, tmp_path / "two" / f"scene_{i % 2}" / f"{i:03d}.png")
    assert len(cleanfid.list_images(tmp_path / "one")) == 5 and len(cleanfid.list_images(tmp_path / "two")) == 4
    metric.reset()
    for folder, real in ((tmp_path / "one", False), (tmp_path / "two", True)):
        for imgs in cleanfid.iter_batches(folder, batch=2):
            assert imgs.dtype == torch.uint8 and imgs.shape[0] <= 2
            metric.update(imgs.cuda(), real=real)
    assert metric._n == {False: 5, True: 4}
    want = float(metric.compute())
    assert np.isfinite(want)
    got = cleanfid.compute_fid(tmp_path / "one", tmp_path / "two", model, batch=2)
    assert got == want
    torch.save(R.with_other_layers(R.make_weights()), tmp_path / "inception.pth")
    assert cleanfid.main([str(tmp_path / "one"), str(tmp_path / "two"), "--weights", str(tmp_path / "inception.pth"), "--json", str(tmp_path / "out.json"),
                          "--batch", "2"]) == 0
    rec = json.loads((tmp_path / "out.json").read_text())
    assert rec["fidclean"] == want and rec["n1"] == 5 and rec["n2"] == 4 and rec["solve"]["capped"] == 0
    # a captured update with a caller-owned workspace replays on the new contents of its input
    imgs = torch.stack([(t * 255).round().to(torch.uint8) for t in a]).cuda()
    other = torch.stack([(t * 255).round().to(torch.uint8) for t in c[:3]]).cuda()
    ws = torch.empty(model.workspace_bytes(3, 20, 28), dtype=torch.uint8, device="cuda")
    metric.reset()
    metric.update(other, real=True)
    eager = metric.real_state.clone()
    buf = imgs.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        metric.update(buf, real=True, ws=ws)                                      # warm-up: packs and scratch exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                 # one stream: a single-branch graph
        metric.update(buf, real=True, ws=ws)
    metric.reset()
    buf.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(metric.real_state, eager)
    metric.reset()
