"""CPU: the fp64 restatement of FID (tests/fid_ref.py) against what it restates, the committed CPU bounds, the weight loading of
`mv_ldm_amd.fid.FrechetInceptionDistance`, the host-side refusals of `csrc/fid.hip`, and the reports with and without a FID network
(a stub network on the CPU: the plumbing, not the kernels)."""
import json
import warnings

import numpy as np
import pytest
import torch

import fid_ref as R
import metrics_ref as MR
from conftest import GOLDEN
from test_dist_gloo import _StubPipeline
from test_dists_cpu import _same_report, _todays_summarize


@pytest.fixture(scope="module")
def weights():
    return R.make_weights(R.WEIGHT_SEED)


@pytest.fixture(scope="module")
def emu():
    return json.loads((GOLDEN / "fid_cpu_emulation.json").read_text())


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_quantise_is_the_packages_byte_cast():
    k = torch.arange(256, dtype=torch.float32)
    base = k / 255
    mid = (k[:-1] + 0.5) / 255
    below = torch.nextafter(base[1:], torch.tensor(-1.0))
    for x in (base, mid, below, torch.rand(4096, generator=torch.Generator().manual_seed(0))):
        assert torch.equal(R.quantise(x), (x * 255).byte().double())
    assert torch.equal(R.quantise(mid), k[:-1].double())
    assert bool((R.quantise(below) == k[1:].double() - 1).any())       # truncation, not rounding: just below k / 255 is k - 1
    assert R.quantise(x).dtype == torch.float64


def test_resize_is_tensorflow1_bilinear():
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 256, (2, 3, 9, 13), generator=g).double()
    assert torch.equal(R.resize_tf1(x, 9, 13), x)                      # equal size: the identity
    big = torch.randint(0, 256, (1, 3, 598, 598), generator=g).double()
    assert torch.equal(R.resize_tf1(big, 299, 299), big[:, :, ::2, ::2])              # scale exactly 2: decimation, no averaging
    # 2 x 2 -> 3 x 3 by hand: coordinates 0, 2/3, 4/3 -> (lo, hi, d) = (0, 1, 0), (0, 1, 2/3), (1, 1, 1/3); the x lerp first
    small = torch.tensor([[1.0, 2.0], [3.0, 5.0]]).view(1, 1, 2, 2)
    s = float(np.float32(2) / np.float32(3))
    d1, d2 = float(np.float32(1) * np.float32(s)), float(np.float32(np.float32(2) * np.float32(s)) - np.float32(1))
    top = [1.0, 1.0 + (2.0 - 1.0) * d1, 2.0]
    bot = [3.0, 3.0 + (5.0 - 3.0) * d1, 5.0]
    want = torch.tensor([top, [t + (b - t) * d1 for t, b in zip(top, bot)], bot], dtype=torch.float64)
    assert torch.equal(R.resize_tf1(small, 3, 3)[0, 0], want)
    assert abs(d1 - 2 / 3) < 1e-7 and abs(d2 - 1 / 3) < 1e-7 and d1 != 2 / 3             # the coordinates are fp32
    lo, hi, d = R.taps(2, 3)
    assert lo.tolist() == [0, 0, 1] and hi.tolist() == [1, 1, 1] and d.dtype == torch.float32 and float(d[2]) == d2
    lo, hi, _ = R.taps(7, 299)
    assert int(lo.max()) == 6 and int(hi.max()) == 6                    # the clamp of `hi`
    assert tuple(R.prep(torch.rand(2, 3, 5, 4)).shape) == (2, 3, 299, 299)


def test_folded_batchnorm_is_batchnorm(weights):
    x = R.prep(R.make_images(2, 16, 24, seed=3))
    f64 = R.stem(x, weights)
    assert tuple(f64.shape) == (2, 64, 147, 147) and bool((f64 >= 0).all())
    f = x
    for name, _, _, stride, pad in R.LAYERS:                           # folded, in fp64
        w, b = R.fold_bn(weights, name)
        f = torch.nn.functional.conv2d(f, w, b, stride=stride, padding=pad).relu()
    assert float((f - f64).abs().max()) <= 1e-12 * float(f64.abs().max())
    feats = R.maxpool_mean(f64)
    assert tuple(feats.shape) == (2, 64) and torch.equal(feats, torch.nn.functional.max_pool2d(f64, 3, 2).mean((2, 3)))
    assert tuple(torch.nn.functional.max_pool2d(f64, 3, 2).shape[-2:]) == (73, 73)


def test_state_identity_is_the_sample_covariance():
    f = torch.rand(7, R.D, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    st = R.state(f)
    assert st.numel() == 1 + 64 + 64 * 64 and float(st[0]) == 7
    mu, sigma = R.moments(st)
    assert np.allclose(mu, f.mean(0).numpy(), rtol=1e-14, atol=0)
    assert np.allclose(sigma, torch.cov(f.t()).numpy(), rtol=1e-11, atol=1e-14)
    back = R.state_from_moments(mu, sigma, 7)
    assert np.allclose(back.numpy(), st.numpy(), rtol=1e-12, atol=1e-13)


def test_the_three_routes_agree_and_the_symmetric_form_is_the_packages(emu):
    """The condition the GPU bounds rest on, checked here and not on the GPU: on every golden case the symmetric form the device computes
    is within 1e-6 (on the error scale) of the package's `eigvals` route."""
    assert max(emu["sym_vs_pkg"].values()) <= 1e-6, emu["sym_vs_pkg"]
    assert set(emu["sym_vs_pkg"]) == {f"synthetic/{k}" for k in R.synthetic_cases()} | set(emu["want"])
    for name, (cls, s1, s2, c) in R.synthetic_cases().items():
        sc = R.scale(s1, s2)
        sym, pkg = R.frechet_sym(s1, s2), R.frechet_pkg(s1, s2)
        got, info = R.jacobi_emulation(s1, s2)
        assert abs(sym - pkg) <= 1e-6 * sc, name
        assert info[4] == 0 and info[0] < R.SWEEP_CAP and info[2] < R.SWEEP_CAP and max(info[1], info[3]) <= R.TOL * (1 + 1e-9), (name, info)
        assert abs(got - sym) <= 10 * emu["jacobi"]["worst"][cls] * sc, name
        if c is not None:
            assert abs(sym - (sc - 2 * c)) <= 1e-12 * sc, name         # the analytic value of the commuting and the diagonal pair
        if cls == "full" and name != "decades12":
            assert abs(sym - pkg) <= 1e-12 * sc, name                  # well-conditioned: the two routes agree to round-off


def test_jacobi_diagonalises():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((64, 64))
    a = a @ a.T
    lam, v, sweeps, off, ok = R.jacobi(a, vectors=True)
    assert ok and sweeps < R.SWEEP_CAP and off <= R.TOL
    assert np.allclose(np.sort(lam), np.linalg.eigvalsh(a), rtol=1e-12, atol=1e-12 * abs(lam).max())
    assert np.allclose((v * lam) @ v.T, a, rtol=0, atol=1e-12 * abs(a).max()) and np.allclose(v.T @ v, np.eye(64), atol=1e-13)
    for r in range(63):                                                # every round: 32 disjoint pairs; a sweep: every pair once
        p, q = R._round_pairs(r)
        assert sorted([*p, *q]) == list(range(64)) and bool((p < q).all())
    assert len({(int(a_), int(b_)) for r in range(63) for a_, b_ in zip(*R._round_pairs(r))}) == 64 * 63 // 2
    assert R.jacobi(np.zeros((64, 64)))[2:] == (0, 0.0, True)          # nothing to do
    bad = a.copy()
    bad[3, 4] = bad[4, 3] = float("nan")
    assert R.jacobi(bad)[2:5:2] == (R.SWEEP_CAP, False)                 # never spins: the cap, and it says so


def test_the_committed_bounds_are_those_of_the_restatement_on_the_tests_inputs(weights, emu):
    """the smallest case of every kind of pair and the synthetic states, recomputed (tests/golden/make_fid_bounds.py does all of them)"""
    assert emu["weights_seed"] == R.WEIGHT_SEED and [tuple(c) for c in emu["cases"]] == R.CASES
    assert set(emu["want"]) == {R.case_key(p, *c) for c in R.CASES for p in R.PAIRS} == set(emu["scale"])
    n_real, n_fake, h, w = R.CASES[0]
    for pair in R.PAIRS:
        real, fake = R.make_sets(pair, n_real, n_fake, h, w, seed=R.case_seed(n_real, n_fake, h, w))
        key = R.case_key(pair, n_real, n_fake, h, w)
        want, s1, s2 = R.fid(real, fake, weights)
        sc = R.scale(s1, s2)
        assert abs(sc - emu["scale"][key]) <= 1e-9 * sc and abs(want - emu["want"][key]) <= 1e-6 * sc      # (null eigenvalues: noise of the host's LAPACK)
        got, _, _ = R.fid(real, fake, weights, dtype=torch.float32, route=lambda a, b: R.jacobi_emulation(a, b)[0])
        assert abs(got - want) / sc <= 10 * emu["worst_err"]["float32"][pair]
    for name, rec in emu["jacobi"]["cases"].items():
        cls, s1, s2, c = R.synthetic_cases()[name]
        assert rec["class"] == cls and abs(rec["scale"] - R.scale(s1, s2)) <= 1e-12 * rec["scale"]
        assert rec["err"] <= emu["jacobi"]["worst"][cls]
    for name in ("float32", "float16", "bfloat16"):
        assert set(emu["worst_err"][name]) == set(R.PAIRS) and all(0 < v < 1e-2 for v in emu["worst_err"][name].values())
    # identical sets: no zero, no sign -- but within the noise floor of the rank-deficient class
    real = R.make_images(3, 16, 24, seed=4)
    same, s1, s2 = R.fid(real, real.clone(), weights)
    assert abs(same) <= 10 * emu["jacobi"]["worst"]["deficient"] * R.scale(s1, s2)


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def _module(**kw):
    from mv_ldm_amd.fid import FrechetInceptionDistance
    return FrechetInceptionDistance(**kw)


def test_both_weight_file_layouts_load_into_the_same_parameters(weights, tmp_path):
    a = _module(weights=R.with_other_layers(weights))                                   # torch-fidelity's pt_inception, all its other keys
    tm = R.with_other_layers(R.make_weights(R.WEIGHT_SEED, prefix="inception."), prefix="inception.")
    torch.save(tm, tmp_path / "tm.pth")
    b = _module(weights=str(tmp_path / "tm.pth"))                                       # torchmetrics' state dict, from a file
    sa, sb = a.state_dict(), b.state_dict()
    assert sorted(sa) == sorted(weights) == sorted(sb)                                   # the running states are no weights
    for k, v in weights.items():
        assert torch.equal(sa[k], v) and torch.equal(sb[k], v), k
    assert a.real_state.dtype == torch.float64 and a.half().real_state.dtype == torch.float64 and a.Conv2d_1a_3x3.conv.weight.dtype == torch.float16


def test_what_load_weights_and_the_constructor_refuse(weights):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = _module(allow_random_init=True)                                             # silent
    with pytest.warns(UserWarning, match="RANDOM initial weights"):
        _module()
    for feature in (192, 768, 2048):
        with pytest.raises(NotImplementedError, match="feature=64"):
            _module(feature=feature, allow_random_init=True)
    with pytest.raises(ValueError):
        _module(feature=65, allow_random_init=True)
    with pytest.raises(TypeError):
        _module(dtype=torch.float64, allow_random_init=True)
    missing = {k: v for k, v in weights.items() if k != "Conv2d_2a_3x3.bn.running_var"}
    with pytest.raises(KeyError, match="Conv2d_2a_3x3.bn.running_var"):
        m.load_weights(missing)
    with pytest.raises(KeyError, match="Conv2d_9z_3x3.conv.weight"):
        m.load_weights({**weights, "Conv2d_9z_3x3.conv.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match="real_features_sum"):
        m.load_weights({**R.make_weights(1, prefix="inception."), "real_features_sum": torch.zeros(64)})
    with pytest.raises(ValueError, match="shape"):
        m.load_weights({**weights, "Conv2d_2b_3x3.conv.weight": torch.zeros(64, 32, 1, 1)})
    var = weights["Conv2d_1a_3x3.bn.running_var"].clone()
    var[3] = -1e-3
    with pytest.raises(ValueError, match="not positive"):
        m.load_weights({**weights, "Conv2d_1a_3x3.bn.running_var": var})
    with pytest.raises(TypeError):
        m.load_weights([1, 2])
    before = {k: v.clone() for k, v in m.state_dict().items()}                          # a refused file changes nothing
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in before.items())
    with pytest.raises(RuntimeError, match="More than one sample"):
        m.compute()                                                                     # host counters: no device needed to refuse
    with pytest.raises(RuntimeError, match="HIP device"):
        m.update(torch.rand(2, 3, 8, 8), real=True)
    with pytest.raises(NotImplementedError):
        m(torch.rand(2, 3, 8, 8))
    assert m.chunk_images(torch.float32) * 147 * 147 * 64 * 4 < 2 ** 31 and m.chunk_images(torch.bfloat16) == 2 * m.chunk_images(torch.float32)


# ---- the library --------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_fid_entry_points_and_refuses_on_the_host():
    from mv_ldm_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.mvldm_abi_version() == 7
    for name in ("workspace_bytes", "pool_slots", "prep", "pool", "accumulate", "compute"):
        assert f"mvldm_fid_{name}" in _lib.SIGNATURES and hasattr(lib, f"mvldm_fid_{name}")
    slots = lib.mvldm_fid_pool_slots                                   # bands of ceil(512 / ow) output rows
    assert slots(147, 147, 64) == 10 and slots(9, 147, 64) == 1 and slots(3, 3, 128) == 1 and slots(147, 5, 64) == 1 and slots(2051, 3, 64) == 3
    assert slots(2, 9, 64) == 0 and slots(9, 2, 64) == 0 and slots(9, 9, 96) == 0 and slots(9, 9, 576) == 0 and slots(9, 9, 3) == 0
    assert lib.mvldm_fid_workspace_bytes(5, 147, 147, 64) == 5 * 11 * 64 * 8 and lib.mvldm_fid_workspace_bytes(0, 147, 147, 64) == 0
    err = lambda: lib.mvldm_last_error()
    prep = lambda n=1, h=8, w=8, oh=8, ow=8, cp=4, dtype=_lib.F32, src=None, dst=None, u8=0: lib.mvldm_fid_prep(src, u8, dst, n, h, w, oh, ow, cp, dtype, None)
    assert prep(h=0) == -1 and b"edge below 1" in err()
    assert prep(ow=0) == -1 and b"edge below 1" in err()
    assert prep(cp=8) == -1 and b"c_pad" in err()
    assert prep(cp=4, dtype=_lib.F16) == -1 and b"c_pad" in err()
    assert prep(dtype=9) == -1 and b"dtype" in err()
    assert prep(u8=2) == -1 and b"src_u8" in err()
    assert prep() == -1 and b"null" in err()
    assert prep(src=6, dst=16) == -1 and b"unaligned" in err()
    assert prep(n=0) == 0
    pool = lambda h=9, c=64, nbytes=1 << 20, feat=None, ws=None, n=2: lib.mvldm_fid_pool(feat, n, h, 9, c, _lib.F32, ws, nbytes, None)
    assert pool(h=2) == -1 and b"3 x 3 window" in err()
    assert pool(c=96) == -1 and b"multiples of 64" in err()
    assert pool(nbytes=2 * 64 * 8 - 8) == -1 and b"workspace" in err()
    assert pool() == -1 and b"null" in err()
    assert pool(feat=16, ws=4) == -1 and b"unaligned" in err()
    assert pool(n=0) == 0
    acc = lambda h=9, c=64, nbytes=1 << 20, ws=None, state=None, n=2: lib.mvldm_fid_accumulate(ws, nbytes, n, h, 9, c, None, state, None)
    assert acc(h=2) == -1 and b"refused" in err()
    assert acc(nbytes=2 * 2 * 64 * 8 - 8) == -1 and b"workspace" in err()
    assert acc() == -1 and b"null" in err()
    assert acc(n=0) == 0
    assert lib.mvldm_fid_compute(None, None, 128, None, None, None) == -1 and b"built for 64" in err()
    assert lib.mvldm_fid_compute(None, None, 64, None, None, None) == -1 and b"null" in err()


def test_the_fid_kernels_use_no_scratch():
    from mv_ldm_amd import _build
    _build.build()
    if not _build.RES.exists():
        _build.build(force=True)
    # fid_accumulate's second launch is frechet_state_kernel (inception.hip), the one state kernel of both Frechet distances
    res = {k: v for k, v in json.loads(_build.RES.read_text()).items() if "fid_" in k or "frechet_state_kernel" in k}
    for fam, count in (("fid_prep_kernel", 6), ("fid_pool_kernel", 3), ("fid_features_kernel", 1), ("frechet_state_kernel", 1), ("fid_compute_kernel", 1)):
        assert sum(1 for k in res if fam in k) == count, fam
    assert not any("fid_state_kernel" in k for k in res)
    bad = {k: (v["scratch"], v.get("vgpr_spill", 0)) for k, v in res.items() if v["scratch"] or v.get("vgpr_spill", 0)}
    assert not bad, bad
    (compute,) = [v for k, v in res.items() if "fid_compute_kernel" in k]
    assert compute["vgpr"] <= 128 and compute.get("agpr", 0) == 0          # the matrices live in LDS, not in registers


# ---- reports: a stub network (the fp64 restatement) on the CPU -- the plumbing, not the kernels ---------------------------------------
class _StubFid:
    def __init__(self, weights):
        self.weights, self.computes = weights, 0
        self.reset()

    def reset(self):
        self.f = {True: [], False: []}

    def update(self, imgs, real):
        self.f[bool(real)].append(R.features(imgs.float(), self.weights))

    def compute(self):
        if min(sum(len(t) for t in self.f[k]) for k in (True, False)) < 2:
            raise RuntimeError("More than one sample is required for both the real and fake distributed to compute FID")
        self.computes += 1
        return torch.tensor(R.frechet_sym(R.state(torch.cat(self.f[True])), R.state(torch.cat(self.f[False]))), dtype=torch.float32)


def test_compute_fid_follows_the_reference_call_order(weights):
    from mv_ldm_amd import metrics as M
    stub = _StubFid(weights)
    gt, pred = R.make_sets("noise", 4, 4, 8, 12, seed=5)
    stub.update(pred, real=True)                                       # whatever was there is dropped
    one = M.compute_fid(gt, pred, stub)
    want, _, _ = R.fid(gt, pred, weights)
    assert one.shape == () and one.dtype == torch.float32 and float(one) == float(torch.tensor(want).float())
    assert stub.f == {True: [], False: []}                             # reset() after compute(), as metric_computer.py:68
    two = M.compute_fid(gt.view(2, 2, 3, 8, 12), pred.view(2, 2, 3, 8, 12), stub)
    assert two.shape == (2,) and float(two[0]) == float(M.compute_fid(gt[:2], pred[:2], stub))
    with pytest.raises(ValueError):
        M.compute_fid(gt, pred[:3], stub)
    with pytest.raises(ValueError):
        M.compute_fid(gt[0], pred[0], stub)
    with pytest.raises(RuntimeError, match="More than one sample"):
        M.compute_fid(gt[:1], pred[:1], stub)


def test_score_trees_with_and_without_a_network(weights, tmp_path, monkeypatch):
    from mv_ldm_amd import metrics as M
    from mv_ldm_amd.image_io import load_image, save_image
    g = torch.Generator().manual_seed(0)
    layout = (("a", (1, 2, 3)), ("b", (7,)), ("c", (4, 5)))
    for side in ("pred", "gt"):
        for scene, frames in layout:
            for f in frames:
                save_image(torch.rand(3, 16, 16, generator=g), tmp_path / side / scene / "color" / f"{f:0>6}.png")
    monkeypatch.setattr(M, "image_metrics", lambda gt, pred: (MR.compute_psnr(gt, pred), MR.compute_ssim(gt, pred)))
    plain = M.score_trees(tmp_path / "pred", tmp_path / "gt", device="cpu", batch=2)
    today = _todays_summarize({s: v["per_frame"] for s, v in plain["scenes"].items()})
    today["missing"] = []
    assert _same_report(plain, today) and list(plain) == ["scenes", "overall", "missing"]           # without fid=: today's report, key for key
    assert "fid" not in json.dumps(plain)
    stub = _StubFid(weights)
    rep = M.score_trees(tmp_path / "pred", tmp_path / "gt", device="cpu", batch=2, fid=stub)
    assert stub.computes == 2 and list(rep) == ["scenes", "overall", "missing"]
    assert list(rep["scenes"]["a"]) == ["psnr", "ssim", "frames", "per_frame", "fid"] and list(rep["overall"]) == ["psnr", "ssim", "frames", "fid"]
    assert rep["scenes"]["b"]["fid"] is None                           # one frame: no covariance
    load = lambda side, s, fr: torch.stack([load_image(tmp_path / side / s / "color" / f"{f:0>6}.png") for f in fr])
    for s, fr in (("a", (1, 2, 3)), ("c", (4, 5))):                    # (ground truth = real, prediction = fake), a scene in chunks of `batch`
        want, _, _ = R.fid(load("gt", s, fr), load("pred", s, fr), weights)
        assert rep["scenes"][s]["fid"] == float(torch.tensor(want).float())
    assert rep["overall"]["fid"] == (rep["scenes"]["a"]["fid"] + rep["scenes"]["c"]["fid"]) / 2      # the mean over the scored scenes
    for s in rep["scenes"].values():
        s.pop("fid")
    rep["overall"].pop("fid")
    assert _same_report(rep, plain)                                    # the per-frame rows and every mean: unchanged
    only_b = M.score_trees(tmp_path / "pred" / "nowhere", tmp_path / "gt", device="cpu", fid=stub)
    assert only_b["overall"]["fid"] is None and only_b["scenes"] == {}


def test_evaluate_adds_fid_only_when_given_a_network(weights):
    from mv_ldm_amd import generate as G
    from test_metrics_cpu import _examples
    cfg = G.merge_config(G.DEFAULT_CONFIG, {"test": {"sampling_mode": "anchored", "num_anchors_views": 4}, "seed": 7})
    ref = lambda gt, pred: (MR.compute_psnr(gt, pred), MR.compute_ssim(gt, pred))
    ex = _examples([0])
    plain = G.evaluate(cfg, ex, pipe=_StubPipeline(), metric_fn=ref)
    got = G.evaluate(cfg, ex, pipe=_StubPipeline(), metric_fn=ref, fid=_StubFid(weights))
    name = ex[0]["scene"][0]
    m, m0 = got["metrics"][name], plain["metrics"][name]
    assert list(m0) == ["psnr", "ssim", "per_frame"] and list(m) == ["psnr", "ssim", "fid", "per_frame"]          # as today without
    assert m["psnr"] == m0["psnr"] and m["ssim"] == m0["ssim"] and m["per_frame"] == m0["per_frame"]
    frames = sorted(m["per_frame"])
    want, _, _ = R.fid(ex[0]["target"]["image"][0].float(), torch.stack([got["frames"][name][f] for f in frames]).float(), weights)
    assert m["fid"] == float(torch.tensor(want).float())
