"""GPU: FID on the device (`csrc/fid.hip`, `mv_ldm_amd.fid.FrechetInceptionDistance`, `metrics.compute_fid`) against the fp64
restatement of tests/fid_ref.py with seeded random weights, `metrics.score_trees(fid=...)` and `MVLDMTrainer.validation_step(fid=...)`.

Error of a score: |got - want| / (|mu1 - mu2|^2 + tr Sigma1 + tr Sigma2), the scale from the fp64 states -- the score itself can be ~ 0.
The bounds come from the CPU (tests/golden/fid_cpu_emulation.json, written by tests/golden/make_fid_bounds.py on exactly these inputs),
never from the kernels: the whole metric in f32 -- 10 x the worst error of the fp32-stem emulation of that kind of pair (the margin
tests/test_hip_lpips.py gives the MFMA's other summation order); f16 / bf16 -- 3 x the worst error of that type's rounding emulation;
the solve alone -- 10 x the worst error of the numpy emulation of the kernel's own rotation order on that class of states (full rank /
rank-deficient: there the null eigenvalues are +- 1e-17 noise and the square root amplifies it to 1e-8-class, in every route).  The pool
and the accumulation alone: 1e-12 relative (fp64 sums of exact terms, fewer than 5.4 k of them, so N 2^-53 < 1e-12)."""
import functools
import json

import numpy as np
import pytest
import torch

import fid_ref as R
from conftest import GOLDEN, record_err

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
NAME = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}
MANT = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}       # mantissa bits, least normal exponent
SUM_TOL = 1e-12
PREP_TOL_F32 = 1e-6


@pytest.fixture(scope="module")
def emu():
    return json.loads((GOLDEN / "fid_cpu_emulation.json").read_text())


@functools.lru_cache(maxsize=None)
def _weights():
    return R.make_weights(R.WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def _want(pair, n_real, n_fake, h, w):
    """(fp64 score, scale) of one small case, computed once for the three dtypes"""
    real, fake = R.make_sets(pair, n_real, n_fake, h, w, seed=R.case_seed(n_real, n_fake, h, w))
    want, s1, s2 = R.fid(real, fake, _weights())
    return want, R.scale(s1, s2)


@functools.lru_cache(maxsize=None)
def _synthetic():
    return R.synthetic_cases()


@pytest.fixture(scope="module")
def model():
    from mv_ldm_amd.fid import FrechetInceptionDistance
    return FrechetInceptionDistance(weights=_weights()).cuda()


def bound(emu, dtype, pair):
    return (10.0 if dtype == torch.float32 else 3.0) * emu["worst_err"][NAME[dtype]][pair]


def _score(model, real, fake, dtype=None, **kw):
    model.reset()
    model.update(real.cuda(), real=True, dtype=dtype, **kw)
    model.update(fake.cuda(), real=False, dtype=dtype, **kw)
    out = model.compute()
    assert out.shape == () and out.dtype == torch.float32 and out.is_cuda
    return out


def _ulp(v, dtype):
    """the spacing of `dtype` at |v| (fp64 tensor)"""
    mant, emin = MANT[dtype]
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


# ---- prep alone ---------------------------------------------------------------------------------------------------------------------
def _prep_raw(src, oh, ow, dtype, pad=64):
    """mvldm_fid_prep into the middle of a sentinel-filled buffer: the NHWC output [n, oh, ow, c_pad] on the host"""
    from mv_ldm_amd import _lib as L, ops
    n, _, h, w = src.shape
    cp = ops.epc(dtype)
    buf = torch.full((n * oh * ow * cp + 2 * pad,), -7.0, dtype=dtype, device="cuda")
    L.check(L.load().mvldm_fid_prep(src.data_ptr(), int(src.dtype == torch.uint8), buf.data_ptr() + pad * buf.element_size(), n, h, w, oh, ow, cp,
                                    ops.dt(dtype), ops.stream()))
    assert bool((buf[:pad] == -7).all()) and bool((buf[-pad:] == -7).all())
    got = buf[pad:-pad].view(n, oh, ow, cp)
    assert torch.equal(got, ops.fid_prep(src, dtype, oh, ow))
    return got.cpu()


def test_prep_quantises_like_the_package():
    """(x * 255).byte() in fp32 on every k / 255, its two fp32 neighbours and the midpoints, at equal size (the resize is the identity, so
    the output is (q - 128) / 128 exactly); the neighbour below k / 255 truncates to k - 1, and so must the kernel.  Outside [0, 1] the
    kernel clamps (documented in include/mvldm.h; the package's .byte() wraps there)."""
    k = torch.arange(256, dtype=torch.float32)
    base = k / 255
    vals = torch.cat([base, torch.nextafter(base, torch.tensor(2.0)), torch.nextafter(base, torch.tensor(-1.0)).clamp_min(0), (k[:-1] + 0.5) / 255,
                      torch.tensor([1.0])])
    assert vals.numel() == 1024
    x = torch.stack([vals.roll(s) for s in (0, 341, 682)]).view(1, 3, 32, 32).contiguous()
    want = (R.quantise(x) - 128) / 128
    assert bool((R.quantise(torch.nextafter(base[1:], torch.tensor(-1.0))) == k[1:].double() - 1).any())      # the k - 1 cases exist
    assert torch.equal(R.quantise(x), (x * 255).byte().double())
    got = _prep_raw(x.cuda(), 32, 32, torch.float32)
    assert torch.equal(got[..., :3].permute(0, 3, 1, 2).double(), want) and bool((got[..., 3] == 0).all())
    out = torch.tensor([-0.5, -1e-9, 1.0 + 1e-6, 7.0]).view(1, 1, 2, 2).expand(1, 3, 2, 2).contiguous()
    got = _prep_raw(out.cuda(), 2, 2, torch.float32)[0, :, :, 0].reshape(-1)
    assert torch.equal(got, (torch.tensor([0.0, 0.0, 255.0, 255.0]) - 128) / 128)


def _pattern(n, h, w):
    """uint8 [n, 3, h, w] whose horizontal and vertical neighbours always differ (by 101 and 37 mod 256): a wrong tap cannot hide"""
    i, c, y, x = torch.meshgrid(torch.arange(n), torch.arange(3), torch.arange(h), torch.arange(w), indexing="ij")
    return ((37 * y + 101 * x + 59 * c + 83 * i) % 256).to(torch.uint8).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("h,w,oh,ow", [(1, 1, 3, 3), (2, 3, 5, 4), (5, 7, 5, 7), (8, 6, 4, 3), (7, 5, 299, 299), (301, 300, 299, 299)], ids=str)
def test_prep_resizes_like_tensorflow1(h, w, oh, ow, dtype):
    """Against `fid_ref.resize_tf1` (coordinates in fp32, values in fp64).  The taps: neighbouring bytes of the pattern differ by at least
    37, so a tap one pixel off moves the output by up to 37 / 128 -- five orders above the bound.  f32 bound, 1e-6 absolute: the bytes are
    integers <= 255, so a00 - a01 is exact and every other fp32 operation rounds a value below 256 by at most 2^-17 = 7.6e-6: v0 and v1
    carry 2 roundings each (1.5e-5), v1 - v0 inherits both and adds one (3.8e-5), times dy < 1 and one more (4.6e-5), plus v0 and one more
    (6.9e-5); the subtraction of 128 is exact in that range or rounds by 2^-18; / 128 gives 5.4e-7, and the last rounding adds 2^-25.
    16 bit: the kernel rounds its fp32 value once, so the output is within one step of the type of a value within that fp32 bound of
    the reference: |got - want| <= 1e-6 + one step.  (Near x = 0, where (v - 128) / 128 cancels, an f16 step is 6e-8, finer than the fp32
    arithmetic on values of 255: "one step of the reference rounded" would be wrong there.)"""
    n = 2
    src = _pattern(n, h, w)
    flt = ((src.float() + 0.5) / 255).contiguous()                               # k / 255 + delta: quantises to k on both paths
    assert torch.equal(R.quantise(flt), src.double())
    want = R.prep(src, torch.float64, oh, ow).permute(0, 2, 3, 1)
    if (h, w, oh, ow) == (5, 7, 5, 7):
        assert torch.equal(want, ((src.double() - 128) / 128).permute(0, 2, 3, 1))                       # identity
    if (h, w, oh, ow) == (8, 6, 4, 3):
        assert torch.equal(want, ((src.double() - 128) / 128)[:, :, ::2, ::2].permute(0, 2, 3, 1))       # exact 2 x decimation
    if (h, w) == (7, 5):
        assert int(R.taps(h, oh)[1].max()) == h - 1 and int((R.taps(h, oh)[0] == h - 1).sum()) > 0      # the `hi` clamp is exercised
    got_u8 = _prep_raw(src.cuda(), oh, ow, dtype)
    got = _prep_raw(flt.cuda(), oh, ow, dtype)
    assert torch.equal(got, got_u8)                                               # the uint8 path equals the float path
    assert bool((got[..., 3:] == 0).all())                                        # padding channels exactly 0
    err = (got[..., :3].double() - want).abs()
    if dtype == torch.float32:
        e = record_err("fid_prep/float32_abs", float(err.max()))
        assert e <= PREP_TOL_F32, e
    else:
        steps = (err - PREP_TOL_F32).clamp_min(0) / _ulp(torch.maximum(want.abs(), got[..., :3].double().abs()), dtype)
        e = record_err(f"fid_prep/{NAME[dtype]}_steps", float(steps.max()))
        assert e <= 1.0, e
    print(f"prep {h}x{w} -> {oh}x{ow} {NAME[dtype]}: worst {e:.3e}")


# ---- the pool alone -----------------------------------------------------------------------------------------------------------------
def _pool(x, extra_slots=1):
    """the partial sums [n, slots, c] of NHWC x, with `extra_slots` unused slots on either side checked to stay zero"""
    from mv_ldm_amd import ops
    n, h, w, c = x.shape
    slots = ops.fid_pool_slots(h, w, c)
    ow = (w - 3) // 2 + 1
    assert slots == -(-((h - 3) // 2 + 1) // -(-512 // ow))
    ws = torch.zeros((n * slots + 2 * extra_slots) * c * 8, dtype=torch.uint8, device="cuda")
    ops.fid_pool(x.cuda(), ws[extra_slots * c * 8: ws.numel() - extra_slots * c * 8])
    part = ws.view(torch.float64).cpu()
    assert bool((part[: extra_slots * c] == 0).all()) and bool((part[-extra_slots * c:] == 0).all())
    return part[extra_slots * c: -extra_slots * c].view(n, slots, c)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("c", [64, 128])
def test_pool_sums_the_max_pooled_relu(c, dtype):
    worst = 0.0
    for (h, w) in ((3, 3), (4, 4), (5, 5), (7, 6), (9, 147), (147, 147)):
        for n in (1, 3):
            g = torch.Generator().manual_seed(c + 31 * h + w + n)
            x = (torch.randn(n, h, w, c, generator=g) - 0.3).to(dtype)             # more than half the entries negative
            x[..., 5] = -x[..., 5].abs() - 0.01                                   # a channel of all-negative windows
            assert float((x < 0).float().mean()) >= 0.5
            part = _pool(x)
            got = part.sum(1)
            px = ((h - 3) // 2 + 1) * ((w - 3) // 2 + 1)
            want = R.maxpool_mean(x.double().permute(0, 3, 1, 2)) * px             # the rounded inputs, in fp64
            assert bool((part[..., 5] == 0).all())                                # exactly 0
            assert bool(((got - want).abs() <= SUM_TOL * want.abs()).all()), (c, dtype, h, w, n)
            worst = max(worst, float(((got - want).abs() / want.abs().clamp_min(1e-300)).max()))
            if (h, w) == (4, 4):                                                  # one window: the last row and column are never read
                for poison in (-1e4, 1e4):
                    y = x.clone()
                    y[:, 3, :, :] = poison
                    y[:, :, 3, :] = poison
                    assert torch.equal(_pool(y), part), poison
    print(f"pool C={c} {NAME[dtype]}: worst rel err {record_err(f'fid_pool/{NAME[dtype]}', worst):.3e}")


# ---- the accumulation alone ---------------------------------------------------------------------------------------------------------
def test_accumulate_folds_and_adds_in_a_fixed_order():
    from mv_ldm_amd import ops
    h = w = 147
    c, px = 64, 73 * 73
    slots = ops.fid_pool_slots(h, w, c)
    assert slots == 10

    def run(parts):
        state = torch.zeros(ops.FID_STATE, dtype=torch.float64, device="cuda")
        feats = []
        for p in parts:
            n = p.shape[0]
            ws = torch.zeros(ops.fid_workspace_bytes(n, h, w, c), dtype=torch.uint8, device="cuda")
            assert ws.numel() == n * (slots + 1) * c * 8
            ws.view(torch.float64)[: p.numel()] = p.reshape(-1).cuda()
            f = torch.full((n, c), -7.0, dtype=torch.float64, device="cuda")
            ops.fid_accumulate(ws, n, h, w, c, state, f)
            feats.append(f.cpu())
        return state.cpu(), feats

    worst = 0.0
    for n in (1, 2, 5):
        g = torch.Generator().manual_seed(n)
        parts = [torch.rand(n, slots, c, generator=g, dtype=torch.float64) * 500, torch.rand(n + 1, slots, c, generator=g, dtype=torch.float64) * 500]
        state, feats = run(parts)
        again, feats2 = run(parts)
        assert torch.equal(state, again) and all(torch.equal(a, b) for a, b in zip(feats, feats2))       # the same bits every time
        for p, f in zip(parts, feats):                                                                   # the features are the fold, bit for bit
            fold = torch.zeros(p.shape[0], c, dtype=torch.float64)
            for b in range(slots):
                fold = fold + p[:, b]
            assert torch.equal(f, fold / px)
        f = torch.cat(feats)
        want = R.state(f)
        assert float(state[0]) == 2 * n + 1                                                              # the count, exact
        assert bool(((state - want).abs() <= SUM_TOL * want.abs()).all())
        worst = max(worst, float(((state - want).abs() / want.abs()).max()))
        mu, sigma = R.moments(state)
        assert np.allclose(sigma, np.cov(f.numpy().T), rtol=1e-9, atol=1e-12)
    print(f"accumulate: worst rel err {record_err('fid_accumulate/rel', worst):.3e}")


def test_accumulate_and_frechet_accumulate_write_the_same_state():
    """fid_accumulate ends in frechet_accumulate's kernel: the same bits, a second call adds, and no images leave the state alone"""
    from mv_ldm_amd import ops
    n, h, w, c = 3, 5, 5, 64                                            # a 2 x 2 pooled map
    x = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(11)).cuda()
    ws = torch.zeros(ops.fid_workspace_bytes(n, h, w, c), dtype=torch.uint8, device="cuda")
    ops.fid_pool(x, ws)
    s1 = torch.zeros(ops.FID_STATE, dtype=torch.float64, device="cuda")
    s2 = torch.zeros(ops.frechet_state_size(c), dtype=torch.float64, device="cuda")
    f = torch.full((n, c), -7.0, dtype=torch.float64, device="cuda")
    ops.fid_accumulate(ws, n, h, w, c, state=s1, features=f)
    once = s1.clone()
    assert float(once[0]) == n and float(once[1:].abs().max()) > 0 and bool((f >= 0).all())
    ops.fid_accumulate(ws, n, h, w, c, state=s1, features=f)
    assert torch.equal(s1, 2 * once) and not torch.equal(s1, once)     # the second call adds: v + v, exact in binary
    ops.frechet_accumulate(f, s2)
    assert torch.equal(s2, once)
    ops.frechet_accumulate(f, s2)
    assert torch.equal(s1, s2)
    ops.fid_accumulate(ws, 0, h, w, c, state=s1)
    ops.frechet_accumulate(f[:0], s2)
    assert torch.equal(s1, 2 * once) and torch.equal(s2, 2 * once)


# ---- the Frechet distance alone -----------------------------------------------------------------------------------------------------
def _compute(s1, s2):
    from mv_ldm_amd import ops
    out = torch.full((1,), -7.0, device="cuda")
    info = torch.full((ops.FID_INFO,), -7.0, dtype=torch.float64, device="cuda")
    ops.fid_compute(s1.cuda(), s2.cuda(), out, info)
    return out.cpu(), info.cpu()


@pytest.mark.parametrize("name", sorted(R.synthetic_cases()), ids=str)
def test_compute_from_synthetic_states(name, emu):
    """Each case against `frechet_sym` (numpy `eigh` twice; the analytic value for the commuting and the diagonal pair), bounded by
    10 x the worst error the numpy emulation of the kernel's rotation order has on its class of states.  info[5] is the score before
    its rounding to fp32; the fp32 output is that value rounded."""
    from mv_ldm_amd import ops
    cls, s1, s2, c = _synthetic()[name]
    rec = emu["jacobi"]["cases"][name]
    sc = R.scale(s1, s2)
    want = R.frechet_sym(s1, s2) if c is None else sc - 2 * c
    assert rec["class"] == cls and abs(want - rec["want"]) <= 1e-6 * sc           # the same inputs (the null eigenvalues' noise differs between hosts)
    tol = 10.0 * emu["jacobi"]["worst"][cls]
    out, info = _compute(s1, s2)
    got = float(info[5])
    e = record_err(f"fid_compute/{cls}", abs(got - want) / sc)
    print(f"compute {name} ({cls}): err {e:.3e}, bound {tol:.3e}; sweeps {int(info[0])} + {int(info[2])}, off {float(info[1]):.1e}, {float(info[3]):.1e}; "
          f"fid {got:.6e} of scale {sc:.3e}")
    assert e <= tol, (name, e, tol)
    assert float(out) == float(torch.tensor(got, dtype=torch.float64).float())
    assert int(info[4]) == 0 and 0 <= int(info[0]) < R.SWEEP_CAP and 0 <= int(info[2]) < R.SWEEP_CAP      # both solves converged below the cap
    assert float(info[1]) <= R.TOL * (1 + 1e-9) and float(info[3]) <= R.TOL * (1 + 1e-9)
    assert abs(float(info[7]) - sc) <= 1e-12 * sc
    back, info_b = _compute(s2, s1)                                                # symmetric in its arguments, within the bound
    assert abs(float(info_b[5]) - want) / sc <= tol and int(info_b[4]) == 0
    out2, info2 = _compute(s1, s2)                                                 # repeated launches: the same bits
    assert torch.equal(out, out2) and torch.equal(info, info2)
    if name.startswith("identical"):                                              # no sign and no zero is demanded
        assert abs(got) / sc <= tol


def test_compute_refuses_on_the_device_what_the_host_cannot_see():
    """fewer than 2 samples in a state: NaN, as the package divides by n - 1 (the module refuses before the launch, from host counters)"""
    s1 = R.random_state(1, 3)
    out, info = _compute(s1, R.random_state(5, 4))
    assert bool(torch.isnan(out).all())


# ---- the whole metric ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("n_real,n_fake,h,w", R.CASES, ids=lambda v: str(v))
def test_parity_with_the_fp64_restatement(n_real, n_fake, h, w, dtype, model, emu):
    for pair in R.PAIRS:
        real, fake = R.make_sets(pair, n_real, n_fake, h, w, seed=R.case_seed(n_real, n_fake, h, w))
        key = R.case_key(pair, n_real, n_fake, h, w)
        want, sc = emu["want"][key], emu["scale"][key]
        if h * w <= 64 * 64:                                         # the small cases are recomputed, 256 x 256 is the recorded fp64 score
            w2, sc2 = _want(pair, n_real, n_fake, h, w)
            assert abs(w2 - want) <= 1e-6 * sc and abs(sc2 - sc) <= 1e-9 * sc      # the same inputs (the null eigenvalues' noise differs between hosts)
            want, sc = w2, sc2
        got = float(_score(model, real, fake, dtype))
        e = record_err(f"fid_rel/{NAME[dtype]}/{pair}", abs(got - want) / sc)
        print(f"{key} {NAME[dtype]}: err {e:.3e}, bound {bound(emu, dtype, pair):.3e} (fid {want:.4e}, scale {sc:.4e})")
        assert e <= bound(emu, dtype, pair), (pair, e, bound(emu, dtype, pair))
        assert int(model.info[4]) == 0


def test_features_are_the_fp64_restatement(model):
    imgs = R.make_images(3, 16, 24, seed=5)
    got = model.features(imgs.cuda())
    assert got.shape == (3, 64) and got.dtype == torch.float64 and got.is_cuda
    want = R.features(imgs, _weights())
    e = record_err("fid_features/float32", float(((got.cpu() - want).abs().max() / want.abs().max())))
    # three fp32 layers of at most K = 288 products each: sqrt(K) 2^-24 ~ 1e-6 a layer, 3e-6 through the stem, and a mean of 5329 maxima does
    # not add to it; 1e-5 of the largest feature.  The score's own bound is the test above.
    assert e <= 1e-5, e
    # features() leaves the running states alone
    before = model.real_state.clone()
    model.features(imgs.cuda())
    assert torch.equal(before, model.real_state)


def test_updates_in_chunks_score_within_the_f32_bound(model, emu, monkeypatch):
    """the conv tile may differ with the batch size, so not bit for bit: within the f32 bound of the single call"""
    monkeypatch.setenv("MVLDM_AUTOTUNE", "0")
    real, fake = R.make_sets("other", 5, 5, 16, 24, seed=R.case_seed(5, 5, 16, 24))
    _, sc = _want("other", 5, 5, 16, 24)
    full = float(_score(model, real, fake))
    monkeypatch.setattr(type(model), "chunk_images", staticmethod(lambda dtype: 2))       # 2 + 2 + 1 images a side through one workspace
    chunked = float(_score(model, real, fake))
    monkeypatch.undo()
    assert abs(chunked - full) / sc <= bound(emu, torch.float32, "other")
    assert type(model).chunk_images(torch.float32) == 388 and type(model).chunk_images(torch.float16) == 776
    assert 388 * 147 * 147 * 64 * 4 < 2 ** 31 <= 389 * 147 * 147 * 64 * 4


def test_reset_really_clears(model):
    a_real, a_fake = R.make_sets("other", 3, 3, 16, 24, seed=1)
    b_real, b_fake = R.make_sets("brighter", 2, 4, 16, 24, seed=2)
    b_alone = _score(model, b_real, b_fake).clone()
    a = _score(model, a_real, a_fake).clone()                        # _score resets first
    model.reset()
    assert model._n == {True: 0, False: 0} and bool((model.real_state == 0).all()) and bool((model.fake_state == 0).all())
    model.update(b_real.cuda(), real=True)
    model.update(b_fake.cuda(), real=False)
    assert torch.equal(model.compute(), b_alone) and not torch.equal(a, b_alone)
    model.update(a_real.cuda(), real=True)                           # and without a reset the sets add up
    assert float(model.real_state[0]) == 5 and not torch.equal(model.compute(), b_alone)
    model.reset()


def test_too_few_samples_and_other_taps_are_refused(model):
    from mv_ldm_amd.fid import FrechetInceptionDistance
    imgs = R.make_images(3, 16, 24, seed=3).cuda()
    model.reset()
    with pytest.raises(RuntimeError, match="More than one sample"):
        model.compute()
    model.update(imgs, real=True)
    model.update(imgs[:1], real=False)
    with pytest.raises(RuntimeError, match="More than one sample"):
        model.compute()
    model.update(imgs[1:2], real=False)
    assert bool(torch.isfinite(model.compute()))
    model.reset()
    for feature in (192, 768, 2048):
        with pytest.raises(NotImplementedError, match="feature=64"):
            FrechetInceptionDistance(feature=feature)
    with pytest.raises(TypeError):
        model.update(torch.zeros(2, 3, 8, 8, dtype=torch.uint8, device="cuda"), real=True)          # normalize=True takes floats
    with pytest.raises(ValueError, match=r"\[n, 3, h, w\]"):
        model.update(torch.rand(2, 1, 8, 8, device="cuda"), real=True)
    with pytest.raises(ValueError, match="contiguous"):
        model.update(torch.rand(2, 3, 8, 16, device="cuda")[..., ::2], real=True)
    assert model._n == {True: 0, False: 0}


def test_uint8_images_score_like_their_floats():
    from mv_ldm_amd.fid import FrechetInceptionDistance
    m8 = FrechetInceptionDistance(normalize=False, weights=_weights()).cuda()
    mf = FrechetInceptionDistance(normalize=True, weights=_weights()).cuda()
    real, fake = _pattern(3, 9, 11), _pattern(4, 9, 11).flip(0).contiguous()
    flt = lambda t: ((t.float() + 0.5) / 255).contiguous()
    a = _score(m8, real, fake)
    assert torch.equal(a, _score(mf, flt(real), flt(fake))) and bool(torch.isfinite(a))


def test_a_captured_launch_scores_the_new_contents_of_its_buffers(model):
    n, h, w = 3, 16, 24
    a_real, a_fake = R.make_sets("other", n, n, h, w, seed=17)
    b_real, b_fake = R.make_sets("noise", n, n, h, w, seed=19)
    real, fake = a_real.cuda(), a_fake.cuda()
    out = torch.empty((), device="cuda")
    ws = torch.empty(model.workspace_bytes(n), dtype=torch.uint8, device="cuda")

    def run():
        model.reset()
        model.update(real, real=True, ws=ws)
        model.update(fake, real=False, ws=ws)
        model.compute(out=out)

    want0 = _score(model, a_real, a_fake).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                    # one stream: a single-branch graph
        run()
    graph.replay()
    assert torch.equal(out, want0)
    real.copy_(b_real)
    fake.copy_(b_fake)
    graph.replay()
    torch.cuda.synchronize()
    got1 = out.clone()
    want1 = _score(model, b_real, b_fake)
    assert torch.equal(got1, want1) and not torch.equal(want0, want1)
    model.reset()


def test_refusals_return_a_status_and_launch_nothing():
    from mv_ldm_amd import _lib as L, ops
    lib = L.load()
    n, h, w, c = 2, 9, 9, 64
    x = torch.randn(n, h, w, c, device="cuda")
    keep = x.clone()
    slots = ops.fid_pool_slots(h, w, c)
    assert slots == 1 and ops.fid_pool_slots(2, 9, c) == 0 and ops.fid_pool_slots(9, 9, 96) == 0 and ops.fid_workspace_bytes(n, 9, 2, c) == 0
    ws = torch.full((n * (slots + 1) * c,), -7.0, dtype=torch.float64, device="cuda")
    state = torch.full((ops.FID_STATE,), -7.0, dtype=torch.float64, device="cuda")
    feats = torch.full((n, c), -7.0, dtype=torch.float64, device="cuda")
    score = torch.full((1,), -7.0, device="cuda")
    info = torch.full((ops.FID_INFO,), -7.0, dtype=torch.float64, device="cuda")
    im = torch.rand(n, 3, 6, 5, device="cuda")
    dst = torch.full((n, 4, 4, 4), -7.0, device="cuda")
    s = ops.stream()
    pool = lambda feat=x.data_ptr(), hh=h, cc=c, nbytes=ws.numel() * 8, wsp=ws.data_ptr(): lib.mvldm_fid_pool(feat, n, hh, w, cc, L.F32, wsp, nbytes, s)
    acc = lambda hh=h, cc=c, nbytes=ws.numel() * 8, st=state.data_ptr(): lib.mvldm_fid_accumulate(ws.data_ptr(), nbytes, n, hh, w, cc, feats.data_ptr(), st, s)
    prep = lambda src=im.data_ptr(), d=dst.data_ptr(), oh=4, cp=4, hh=6: lib.mvldm_fid_prep(src, 0, d, n, hh, 5, oh, 4, cp, L.F32, s)
    comp = lambda cc=64, a=state.data_ptr(), o=score.data_ptr(): lib.mvldm_fid_compute(a, state.data_ptr(), cc, o, info.data_ptr(), s)
    assert pool(hh=2) < 0 and b"3 x 3 window" in lib.mvldm_last_error()
    assert pool(cc=96) < 0 and b"multiples of 64" in lib.mvldm_last_error()
    assert pool(nbytes=n * slots * c * 8 - 8) < 0 and b"workspace" in lib.mvldm_last_error()
    assert pool(feat=None) < 0 and b"null" in lib.mvldm_last_error()
    assert pool(feat=x.data_ptr() + 4) < 0 and b"unaligned" in lib.mvldm_last_error()
    assert pool(wsp=None) < 0
    assert acc(hh=2) < 0 and acc(cc=3) < 0 and acc(nbytes=ws.numel() * 8 - 8) < 0 and b"workspace" in lib.mvldm_last_error()
    assert acc(st=state.data_ptr() + 4) < 0 and b"unaligned" in lib.mvldm_last_error()
    assert prep(src=None) < 0 and b"null" in lib.mvldm_last_error()
    assert prep(d=dst.data_ptr() + 4) < 0 and b"unaligned" in lib.mvldm_last_error()
    assert prep(oh=0) < 0 and prep(hh=0) < 0 and b"edge below 1" in lib.mvldm_last_error()
    assert prep(cp=8) < 0 and b"c_pad" in lib.mvldm_last_error()
    assert comp(cc=128) < 0 and b"64" in lib.mvldm_last_error()
    assert comp(a=None) < 0 and comp(o=score.data_ptr() + 2) < 0
    torch.cuda.synchronize()
    for t in (ws, state, feats, score, info, dst):
        assert bool((t == -7).all())
    assert torch.equal(x, keep)
    state.zero_()                                                    # and the same calls with nothing wrong run
    assert pool() == 0 and acc() == 0 and prep() == 0 and acc() == 0 and comp() == 0
    torch.cuda.synchronize()
    want = R.maxpool_mean(keep.double().permute(0, 3, 1, 2).cpu())
    assert bool(((feats.cpu() - want).abs() <= SUM_TOL * want.abs()).all())
    assert float(state[0]) == 2 * n and bool((dst != -7).all()) and bool((info != -7).all())


def test_the_reference_signature_the_view_axis_and_16_bit_images(model):
    from mv_ldm_amd import metrics as M
    gt, pred = R.make_sets("noise", 6, 6, 16, 24, seed=13)
    gt, pred = gt.cuda(), pred.cuda()
    flat = M.compute_fid(gt, pred, model)
    assert flat.shape == () and flat.dtype == torch.float32 and flat.is_cuda and torch.equal(flat, _score(model, gt, pred))
    assert model._n == {True: 6, False: 6}
    model.reset()
    two = M.compute_fid(gt.view(2, 3, 3, 16, 24), pred.view(2, 3, 3, 16, 24), model)
    assert two.shape == (2,) and model._n == {True: 0, False: 0}
    assert torch.equal(two[0], M.compute_fid(gt[:3], pred[:3], model)) and torch.equal(two[1], M.compute_fid(gt[3:], pred[3:], model))
    for dt in (torch.float16, torch.bfloat16):                       # 16-bit images go through the elementwise convert: the scores of the rounded images
        lo = M.compute_fid(gt.to(dt), pred.to(dt), model)
        assert lo.dtype == torch.float32 and torch.equal(lo, M.compute_fid(gt.to(dt).float(), pred.to(dt).float(), model))
    with pytest.raises(RuntimeError, match="More than one sample"):
        M.compute_fid(gt[:1], pred[:1], model)
    model.reset()


def test_score_trees_reports_one_fid_per_scene(model, tmp_path, capsys):
    from mv_ldm_amd import metrics as M
    from mv_ldm_amd.image_io import load_image, save_image
    real, fake = R.make_sets("noise", 4, 4, 16, 24, seed=23)
    layout = {"scene_a": [0, 1, 2], "scene_b": [3]}
    for root, imgs in (("gt", real), ("pred", fake)):
        for scene, idx in layout.items():
            (tmp_path / root / scene / "color").mkdir(parents=True)
            for i in idx:
                save_image(imgs[i], tmp_path / root / scene / "color" / f"{i:06d}.png")
    plain = M.score_trees(tmp_path / "pred", tmp_path / "gt")
    rep = M.score_trees(tmp_path / "pred", tmp_path / "gt", fid=model)
    assert rep["scenes"]["scene_b"]["fid"] is None and isinstance(rep["scenes"]["scene_a"]["fid"], float)
    assert rep["overall"]["fid"] == rep["scenes"]["scene_a"]["fid"]
    g = torch.stack([load_image(tmp_path / "gt" / "scene_a" / "color" / f"{i:06d}.png") for i in layout["scene_a"]]).cuda()
    p = torch.stack([load_image(tmp_path / "pred" / "scene_a" / "color" / f"{i:06d}.png") for i in layout["scene_a"]]).cuda()
    scene_a = rep["scenes"]["scene_a"]["fid"]
    assert scene_a == float(M.compute_fid(g, p, model))
    for s in rep["scenes"].values():                                 # everything else: the report without a network, key for key
        s.pop("fid")
    rep["overall"].pop("fid")
    assert json.dumps(rep) == json.dumps(plain)
    torch.save(R.with_other_layers(_weights()), tmp_path / "inception.pth")      # and the command line prints the column
    assert M.main(["--pred", str(tmp_path / "pred"), "--gt", str(tmp_path / "gt"), "--fid", str(tmp_path / "inception.pth")]) == 0
    printed = capsys.readouterr().out
    assert f"fid {scene_a:.6f}" in printed and "scene_b" in printed and "fid -" in printed


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
        out = tr.validation_step(batch, num_inference_steps=2, fid=model, **kw)
    keys = ["batch", "context", "psnr", "psnr_roundtrip", "sampled", "ssim", "ssim_roundtrip", "targets", "targets_roundtrip"]
    assert sorted(plain) == keys and sorted(out) == sorted([*keys, "fid", "fid_roundtrip"])
    for k in keys:                                                   # every other entry: the same bits
        if torch.is_tensor(plain[k]):
            assert torch.equal(plain[k], out[k]), k
    assert out["fid"].shape == out["fid_roundtrip"].shape == (2,) and out["fid"].is_cuda and out["fid"].dtype == torch.float32
    assert torch.equal(out["fid"], M.compute_fid(out["targets"], out["sampled"], model))
    assert torch.equal(out["fid_roundtrip"], M.compute_fid(out["targets_roundtrip"], out["sampled"], model))
    assert bool(torch.isfinite(out["fid"]).all()) and not torch.equal(out["fid"], out["fid_roundtrip"])
