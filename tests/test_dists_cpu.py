"""CPU: the parts of the DISTS work that need no GPU -- properties of the fp64 restatement the GPU tests compare against
(tests/dists_ref.py), the committed CPU bounds, the weight-file layouts `DISTS.load_weights` takes, the host-side counts and refusals
of the library's entry points, the refusal of CPU tensors, the shape of the reports of `metrics.summarize` / `score_trees` /
`generate.evaluate` with and without a network, and the kernels' register report."""
import json

import pytest
import torch

import dists_ref as R
import lpips_ref
import metrics_ref as MR
from conftest import GOLDEN
from test_dist_gloo import _StubPipeline

SMALL = [c for c in R.CASES if c[1] * c[2] <= 64 * 64]


@pytest.fixture(scope="module")
def weights():
    return R.make_weights(R.WEIGHT_SEED)


def _params(m):
    return {k: v.clone() for k, v in m.state_dict().items()}


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_restatement_properties(weights):
    gt, pred = R.make_pair("noise05", 2, 24, 19, seed=3)
    ab, ba = R.dists(gt, pred, weights), R.dists(pred, gt, weights)
    assert ab.dtype == torch.float64 and ab.shape == (2,) and bool((ab > 0).all()) and bool((ab < 1).all())
    assert float((ab - ba).abs().max()) <= 1e-15                                      # symmetric in its arguments
    direct = R.dists(gt, pred, weights, form="direct")
    assert torch.equal(direct, R.dists(pred, gt, weights, form="direct"))
    same, _ = R.make_pair("identical", 2, 24, 19, seed=4)
    assert float(R.dists(same, same.clone(), weights).abs().max()) <= 1e-15            # 1 - 0.99999...: to round-off
    assert torch.equal(R.dists(same, same.clone(), weights, form="direct"), torch.zeros(2, dtype=torch.float64))   # exactly 0
    far = R.dists(gt, gt + 0.2 * (pred - gt) / 0.05, weights)
    assert bool((far > ab).all())                                                       # more noise, more distance
    one = R.dists(torch.rand(1, 3, 1, 1), torch.rand(1, 3, 1, 1), weights)             # a 1 x 1 image is valid: every S2 is c2 / c2
    assert one.shape == (1,) and bool(torch.isfinite(one).all())


@pytest.mark.parametrize("n,h,w", SMALL, ids=lambda v: str(v))
def test_the_direct_form_is_the_package_form(n, h, w, weights):
    for kind in ("random", "noise05", "noise002"):
        gt, pred = R.make_pair(kind, n, h, w, seed=R.case_seed(n, h, w))
        taps = R.features(torch.cat([gt, pred]), weights)
        fx, fy = [t[:n] for t in taps], [t[n:] for t in taps]
        pkg, direct = R.score(fx, fy, weights["alpha"], weights["beta"], "package"), R.score(fx, fy, weights["alpha"], weights["beta"], "direct")
        assert float(((pkg - direct).abs() / direct).max()) <= 1e-10, kind
    assert [tuple(t.shape[1:]) for t in taps] == [(c, *hw) for c, hw in zip(R.CHANNELS, _map_sizes(h, w))]


def _map_sizes(h, w):
    out = [(h, w), (h, w)]
    for _ in range(4):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def test_map_sizes_of_the_odd_cases():
    assert _map_sizes(5, 7)[1:] == [(5, 7), (3, 4), (2, 2), (1, 1), (1, 1)]
    assert _map_sizes(37, 45)[1:] == [(37, 45), (19, 23), (10, 12), (5, 6), (3, 3)]


def test_l2_pool_of_a_constant_map():
    x = torch.full((1, 2, 6, 7), 3.0, dtype=torch.float64)
    y = R.l2pool(x)
    assert y.shape == (1, 2, 3, 4)
    assert float((y[:, :, 1:, 1:-1] - 3.0).abs().max()) <= 1e-12                      # the interior: the constant (the filter sums to 1)
    assert bool((y[:, :, 0, :] < 3.0 - 1e-3).all()) and bool((y[:, :, :, 0] < 3.0 - 1e-3).all())   # the zero-padded border: smaller
    assert abs(float(y[0, 0, 0, 0]) - 3.0 * 0.75) <= 1e-12                              # the corner: (2 + 1)(2 + 1) / 16 of the mass
    assert torch.equal(R.hann_filter(1)[0, 0] * 16, torch.tensor([[1.0, 2, 1], [2, 4, 2], [1, 2, 1]], dtype=torch.float64))
    dead = R.l2pool(torch.zeros(1, 1, 1, 1, dtype=torch.float64))
    assert dead.shape == (1, 1, 1, 1) and abs(float(dead) - 1e-6) <= 1e-18


def test_the_committed_bounds_are_those_of_the_restatement_on_the_tests_inputs(weights):
    """tests/golden/dists_cpu_emulation.json is what tests/golden/make_dists_bounds.py writes: the small cases against a fresh run"""
    g = json.loads((GOLDEN / "dists_cpu_emulation.json").read_text())
    assert g["weights_seed"] == R.WEIGHT_SEED and [tuple(c) for c in g["cases"]] == R.CASES
    assert sorted(g["worst_rel_err"]) == ["bfloat16", "float16", "float32"]
    assert sorted(g["worst_rel_err"]["float32"]) == ["noise002", "noise05", "random"]
    assert sorted(g["worst_rel_err"]["float16"]) == sorted(g["worst_rel_err"]["bfloat16"]) == ["noise05", "random"]
    assert len(g["want"]) == 3 * len(R.CASES)
    for n, h, w in SMALL[:6]:                                     # 5 x 7, 16 x 16, 37 x 45
        for kind in ("random", "noise05", "noise002"):
            gt, pred = R.make_pair(kind, n, h, w, seed=R.case_seed(n, h, w))
            want = R.dists(gt, pred, weights)
            assert torch.allclose(want, torch.tensor(g["want"][R.case_key(kind, n, h, w)], dtype=torch.float64), rtol=1e-12, atol=0)
    n, h, w = 3, 16, 16
    gt, pred = R.make_pair("noise05", n, h, w, seed=R.case_seed(n, h, w))
    want = R.dists(gt, pred, weights)
    for name, kw in (("float32", dict(dtype=torch.float32)), ("float16", dict(emulate=torch.float16)), ("bfloat16", dict(emulate=torch.bfloat16))):
        e = float(((R.dists(gt, pred, weights, **kw) - want).abs() / want).max())
        assert 0 < e <= g["worst_rel_err"][name]["noise05"], (name, e)


# ---- weights ----------------------------------------------------------------------------------------------------------------------
def test_both_weight_file_layouts_load_into_the_same_parameters(weights, tmp_path):
    from mv_ldm_amd.dists import DISTS
    full = DISTS(weights=weights)
    want = _params(full)
    consts = {k for k in weights if k in ("mean", "std") or k.endswith(".filter")}
    assert len(consts) == 6 and sorted(want) == sorted(set(weights) - consts) and all(torch.equal(want[k], weights[k]) for k in want)
    assert len([k for k in want if k.endswith(".weight")]) == 13 and want["alpha"].shape == want["beta"].shape == (1, 1475, 1, 1)
    assert want["stage1.0.weight"].shape == (64, 3, 3, 3) and want["stage5.28.bias"].shape == (512,)
    # the package's buffers are optional
    got = _params(DISTS(weights={k: v for k, v in weights.items() if k not in consts}))
    assert all(torch.equal(got[k], want[k]) for k in want)
    # torchvision's VGG-16 (features.* and its classifier) + the package's weights.pt, as files read with weights_only=True
    vgg, ab = R.split_weights(weights)
    assert any(k.startswith("classifier.") for k in vgg) and sorted(ab) == ["alpha", "beta"]
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(ab, tmp_path / "weights.pt")
    got = _params(DISTS(weights=tmp_path / "vgg16.pth", alpha_beta=str(tmp_path / "weights.pt")))
    assert all(torch.equal(got[k], want[k]) for k in want)
    torch.save(weights, tmp_path / "full.pth")
    m = DISTS(allow_random_init=True)
    assert not torch.equal(m.state_dict()["stage1.0.weight"], want["stage1.0.weight"])
    assert m.load_weights(tmp_path / "full.pth") is m and all(torch.equal(v, want[k]) for k, v in m.state_dict().items())


def test_what_load_weights_and_forward_refuse(weights):
    from mv_ldm_amd import metrics as M
    from mv_ldm_amd.dists import DISTS
    m = DISTS(allow_random_init=True)
    short = {k: v for k, v in weights.items() if k not in ("stage3.12.bias", "beta")}
    with pytest.raises(KeyError, match=r"missing keys \['beta', 'stage3.12.bias'\]"):
        m.load_weights(short)
    with pytest.raises(KeyError, match=r"unexpected keys \['stage9.0.weight'\]"):
        m.load_weights({**weights, "stage9.0.weight": torch.zeros(1)})
    vgg, ab = R.split_weights(weights)
    with pytest.raises(KeyError, match="alpha"):
        m.load_weights(vgg)                                       # a torchvision file alone has no alpha / beta
    with pytest.raises(KeyError, match=r"unexpected keys \['features.3.weight'\]"):
        m.load_weights({**vgg, "features.3.weight": torch.zeros(1)}, ab)
    with pytest.raises(ValueError, match="stage1.0.weight has shape"):
        m.load_weights({**weights, "stage1.0.weight": torch.zeros(64, 3, 1, 1)})
    with pytest.raises(ValueError, match="alpha has shape"):
        m.load_weights({**weights, "alpha": torch.ones(1, 1474, 1, 1)})
    for k, bad in (("mean", torch.zeros(1, 3, 1, 1)), ("std", torch.tensor([0.229, 0.224, 0.226]).view(1, 3, 1, 1)),
                   ("stage3.9.filter", torch.full((128, 1, 3, 3), 1.0 / 9))):
        with pytest.raises(ValueError, match="constant"):
            m.load_weights({**weights, k: bad})
    with pytest.raises(ValueError, match="sum"):
        m.load_weights({**weights, "alpha": torch.zeros(1, 1475, 1, 1), "beta": torch.zeros(1, 1475, 1, 1)})
    with pytest.raises(ValueError, match="sum"):
        m.load_weights({**weights, "alpha": -weights["alpha"], "beta": -weights["beta"]})
    with pytest.raises(TypeError):
        DISTS(dtype=torch.float64, allow_random_init=True)
    with pytest.warns(UserWarning, match="RANDOM initial weights"):
        DISTS()
    m.load_weights(weights)
    a = torch.rand(2, 3, 16, 16)
    with pytest.raises(NotImplementedError, match="require_grad"):
        m(a, a, require_grad=True)
    with pytest.raises(NotImplementedError, match="batch_average"):
        m(a, a, batch_average=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.compute_dists(a.view(1, 2, 3, 16, 16), a.view(1, 2, 3, 16, 16), m)
    with pytest.raises(ValueError):
        M.compute_dists(a, a[:1], m)


# ---- the library ------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_dists_entry_points_and_refuses_on_the_host():
    from mv_ldm_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.mvldm_abi_version() == 7
    for name in ("workspace_bytes", "stat_slots", "prep", "stats", "l2pool", "fold"):
        assert f"mvldm_dists_{name}" in _lib.SIGNATURES and hasattr(lib, f"mvldm_dists_{name}")
    # workgroups per pair: bands of 512 pixels at C = 64, of 256 above, of 4096 for the raw image
    slots = lib.mvldm_dists_stat_slots
    assert slots(64, 64, 64) == 8 and slots(32, 32, 128) == 4 and slots(33, 18, 256) == 3 and slots(5, 7, 512) == 1 and slots(1, 1, 64) == 1
    assert slots(64, 64, 3) == 1 and slots(70, 61, 3) == 2 and slots(256, 256, 3) == 16
    assert slots(8, 8, 96) == 0 and slots(8, 8, 576) == 0 and slots(8, 8, 4) == 0 and slots(0, 8, 64) == 0 and slots(8, 0, 3) == 0
    # 64 x 64: the raw image, then maps of 64, 64, 32, 16, 8, 4 pixels a side
    doubles = 5 * (1 * 3 + 8 * 64 + 4 * 128 + 1 * 256 + 1 * 512 + 1 * 512)
    assert lib.mvldm_dists_workspace_bytes(3, 64, 64) == 3 * doubles * 8
    assert lib.mvldm_dists_workspace_bytes(1, 1, 1) == 5 * 1475 * 8                 # no minimum edge
    assert lib.mvldm_dists_workspace_bytes(1, 0, 64) == 0 and lib.mvldm_dists_workspace_bytes(1, 64, 0) == 0 and lib.mvldm_dists_workspace_bytes(0, 64, 64) == 0
    # refusals are decided on the host, before any launch: they can be checked without a device
    err = lambda: lib.mvldm_last_error()
    assert lib.mvldm_dists_prep(None, None, None, 1, 0, 64, 4, _lib.F32, None) == -1 and b"image 0 x 64" in err()
    assert lib.mvldm_dists_prep(None, None, None, 1, 64, 64, 8, _lib.F32, None) == -1 and b"c_pad" in err()
    assert lib.mvldm_dists_prep(None, None, None, 1, 64, 64, 8, 9, None) == -1 and b"dtype" in err()
    assert lib.mvldm_dists_prep(None, None, None, 1, 1, 1, 8, _lib.F16, None) == -1 and b"null" in err()
    assert lib.mvldm_dists_prep(None, None, None, 0, 1, 1, 8, _lib.F16, None) == 0
    per = 5 * 64
    stats = lambda c, nbytes, off=0, stride=per, h=8, dtype=_lib.F32, feat=None: lib.mvldm_dists_stats(feat, None, 2, h, 8, c, dtype, None, nbytes, off, stride, None)
    assert stats(96, 1 << 20) == -1 and b"multiples of 64" in err()
    assert stats(576, 1 << 20) == -1 and b"multiples of 64" in err()
    assert stats(3, 1 << 20, dtype=_lib.F16) == -1 and b"fp32 NCHW" in err()
    assert stats(64, 1 << 20, h=0) == -1 and b"map 0 x 8" in err()
    assert stats(64, 2 * per * 8 - 8) == -1 and b"workspace" in err()
    assert stats(64, 1 << 20, off=1) == -1 and b"partials" in err()
    assert stats(64, 1 << 20, off=-per, stride=2 * per) == -1 and b"partials" in err()
    assert stats(64, 2 * per * 8) == -1 and b"null" in err()
    assert stats(64, 2 * per * 8, feat=24) == -1 and b"unaligned" in err()
    pool = lambda c, h=8, feat=None, dst=None: lib.mvldm_dists_l2pool(feat, dst, 2, h, 8, c, _lib.F32, None)
    assert pool(96) == -1 and b"multiples of 64" in err()
    assert pool(3) == -1 and b"multiples of 64" in err()
    assert pool(64, h=0) == -1 and b"map 0 x 8" in err()
    assert pool(64) == -1 and b"null" in err()
    assert pool(64, feat=16, dst=8) == -1 and b"unaligned" in err()
    assert lib.mvldm_dists_l2pool(None, None, 0, 8, 8, 64, _lib.F32, None) == 0
    fold = lambda nbytes, n=1, h=64: lib.mvldm_dists_fold(None, nbytes, n, h, 64, None, None, None, None)
    assert fold(0, h=0) == -1 and b"image 0 x 64" in err()
    assert fold(doubles * 8 - 8) == -1 and b"workspace" in err()
    assert fold(doubles * 8) == -1 and b"null" in err()
    assert fold(0, n=0) == 0                                      # nothing to do is no error


def test_the_dists_kernels_use_no_scratch():
    from mv_ldm_amd import _build
    _build.build()
    if not _build.RES.exists():
        _build.build(force=True)
    res = {k: v for k, v in json.loads(_build.RES.read_text()).items() if "dists_" in k}
    for fam, count in (("dists_prep_kernel", 3), ("dists_stats_kernel", 3), ("dists_stats0_kernel", 1), ("dists_l2pool_kernel", 3), ("dists_fold_kernel", 1)):
        assert sum(1 for k in res if fam in k) == count, fam
    bad = {k: (v["scratch"], v.get("vgpr_spill", 0)) for k, v in res.items() if v["scratch"] or v.get("vgpr_spill", 0)}
    assert not bad, bad


# ---- reports: stub networks (the fp64 restatements) on the CPU -- the plumbing, not the kernels ------------------------------------
class _StubDists:
    def __init__(self, weights):
        self.weights, self.calls = weights, 0

    def __call__(self, x, y):
        self.calls += 1
        return R.dists(x, y, self.weights)


class _StubLpips:
    def __init__(self):
        self.weights = lpips_ref.make_weights(lpips_ref.WEIGHT_SEED)

    def __call__(self, in0, in1, normalize=False):
        return lpips_ref.lpips(in0, in1, self.weights, normalize=normalize).view(-1, 1, 1, 1)


def _todays_summarize(per_frame):
    """`metrics.summarize` as it was before it took `names=`: what a run without a DISTS network must still report"""
    mean = lambda v: sum(v) / len(v) if v else float("nan")
    every = [v for f in per_frame.values() for v in f.values()]
    names = ("psnr", "ssim", "lpips") if every and all(len(v) == 3 for v in every) else ("psnr", "ssim")
    means = lambda rows: {k: mean([v[j] for v in rows]) for j, k in enumerate(names)}
    scenes = {s: {**means(list(f.values())), "frames": len(f), "per_frame": f} for s, f in per_frame.items()}
    return {"scenes": scenes, "overall": {**means(every), "frames": len(every)}}


def _same_report(a, b):
    """equal key for key, in the same key order, at every level"""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same_report(a[k], b[k]) for k in a)
    return a == b or (a != a and b != b)


def test_summarize_takes_its_column_names_and_keeps_todays_inference():
    from mv_ldm_amd import metrics as M
    two = {"a": {1: [20.0, 0.5], 2: [30.0, 0.7]}, "b": {1: [40.0, 0.9]}}
    three = {"a": {1: [20.0, 0.5, 0.25], 2: [30.0, 0.7, 0.75]}, "b": {1: [40.0, 0.9, 0.5]}}
    for rows in (two, three, {}):
        assert _same_report(M.summarize(rows), _todays_summarize(rows))
    assert list(M.summarize(three)["overall"]) == ["psnr", "ssim", "lpips", "frames"]
    d3 = M.summarize(three, names=("psnr", "ssim", "dists"))                         # three columns are not always lpips
    assert list(d3["overall"]) == ["psnr", "ssim", "dists", "frames"] and d3["scenes"]["a"]["dists"] == 0.5 and "lpips" not in d3["scenes"]["a"]
    four = {"a": {1: [20.0, 0.5, 0.25, 0.125], 2: [30.0, 0.7, 0.75, 0.375]}}
    d4 = M.summarize(four, names=M.metric_names(lpips=object(), dists=object()))
    assert list(d4["scenes"]["a"]) == ["psnr", "ssim", "lpips", "dists", "frames", "per_frame"] and d4["overall"]["dists"] == 0.25
    assert M.metric_names() == ("psnr", "ssim") and M.metric_names(dists=1) == ("psnr", "ssim", "dists")
    with pytest.raises(ValueError, match="columns"):
        M.summarize(four, names=("psnr", "ssim"))


def test_score_trees_with_and_without_a_network(weights, tmp_path, monkeypatch):
    from mv_ldm_amd import metrics as M
    from mv_ldm_amd.image_io import load_image, save_image
    g = torch.Generator().manual_seed(0)
    for side in ("pred", "gt"):
        for scene, frames in (("a", (1, 2, 3)), ("b", (7,))):
            for f in frames:
                save_image(torch.rand(3, 16, 16, generator=g), tmp_path / side / scene / "color" / f"{f:0>6}.png")
    monkeypatch.setattr(M, "image_metrics", lambda gt, pred: (MR.compute_psnr(gt, pred), MR.compute_ssim(gt, pred)))
    plain = M.score_trees(tmp_path / "pred", tmp_path / "gt", device="cpu", batch=2)
    lp = M.score_trees(tmp_path / "pred", tmp_path / "gt", device="cpu", batch=2, lpips=_StubLpips())
    for rep in (plain, lp):                                       # without dists=: today's report, key for key
        today = _todays_summarize({s: v["per_frame"] for s, v in rep["scenes"].items()})
        today["missing"] = []
        assert _same_report(rep, today) and list(rep) == ["scenes", "overall", "missing"]
    stub = _StubDists(weights)
    rep = M.score_trees(tmp_path / "pred", tmp_path / "gt", device="cpu", batch=2, dists=stub)
    assert stub.calls == 3                                        # scene a in chunks of 2 + 1, scene b
    assert list(rep) == ["scenes", "overall", "columns", "missing"] and rep["columns"] == ["psnr", "ssim", "dists"]
    assert list(rep["overall"]) == ["psnr", "ssim", "dists", "frames"] and list(rep["scenes"]["a"]) == ["psnr", "ssim", "dists", "frames", "per_frame"]
    for s in plain["scenes"]:
        for f, row in plain["scenes"][s]["per_frame"].items():
            got = rep["scenes"][s]["per_frame"][f]
            assert got[:2] == row and len(got) == 3
            p, t = load_image(tmp_path / "pred" / s / "color" / f"{f:0>6}.png")[None], load_image(tmp_path / "gt" / s / "color" / f"{f:0>6}.png")[None]
            want = float(R.dists(t, p, weights))                 # (ground truth, prediction), as the reference calls it
            assert abs(got[2] - want) <= 1e-12 * want
    assert abs(rep["scenes"]["a"]["dists"] - sum(v[2] for v in rep["scenes"]["a"]["per_frame"].values()) / 3) < 1e-12
    both = M.score_trees(tmp_path / "pred", tmp_path / "gt", device="cpu", batch=2, lpips=_StubLpips(), dists=_StubDists(weights))
    assert both["columns"] == ["psnr", "ssim", "lpips", "dists"] and list(both["overall"]) == ["psnr", "ssim", "lpips", "dists", "frames"]
    for s in plain["scenes"]:
        for f in plain["scenes"][s]["per_frame"]:
            assert both["scenes"][s]["per_frame"][f] == [*lp["scenes"][s]["per_frame"][f], rep["scenes"][s]["per_frame"][f][2]]


def test_evaluate_adds_dists_only_when_given_a_network(weights):
    from mv_ldm_amd import generate as G
    from test_metrics_cpu import _examples
    cfg = G.merge_config(G.DEFAULT_CONFIG, {"test": {"sampling_mode": "anchored", "num_anchors_views": 4}, "seed": 7})
    ref = lambda gt, pred: (MR.compute_psnr(gt, pred), MR.compute_ssim(gt, pred))
    ex = _examples([0, 2])
    plain = G.evaluate(cfg, ex, pipe=_StubPipeline(), metric_fn=ref)
    lp = G.evaluate(cfg, ex, pipe=_StubPipeline(), metric_fn=ref, lpips=_StubLpips())
    got = G.evaluate(cfg, ex, pipe=_StubPipeline(), metric_fn=ref, dists=_StubDists(weights))
    both = G.evaluate(cfg, ex, pipe=_StubPipeline(), metric_fn=ref, lpips=_StubLpips(), dists=_StubDists(weights))
    assert sorted(got) == sorted(plain) and sorted(got["metrics"]) == sorted(plain["metrics"]) == ["synthetic0000", "synthetic0002"]
    for i in (0, 2):
        name = ex[i]["scene"][0]
        m, m0 = got["metrics"][name], plain["metrics"][name]
        assert list(m0) == ["psnr", "ssim", "per_frame"] and list(lp["metrics"][name]) == ["psnr", "ssim", "lpips", "per_frame"]     # as today
        assert list(m) == ["psnr", "ssim", "dists", "per_frame"] and list(both["metrics"][name]) == ["psnr", "ssim", "lpips", "dists", "per_frame"]
        assert m["psnr"] == m0["psnr"] and m["ssim"] == m0["ssim"] and isinstance(m["dists"], float)
        for j, f in enumerate(range(1, 8)):
            want = float(R.dists(ex[i]["target"]["image"][0, j:j + 1], got["frames"][name][f][None], weights))
            assert m["per_frame"][f][:2] == m0["per_frame"][f] and len(m["per_frame"][f]) == 3
            assert abs(m["per_frame"][f][2] - want) <= 1e-12 * want           # (the stub scores the scene's frames as one batch)
            assert both["metrics"][name]["per_frame"][f] == [*lp["metrics"][name]["per_frame"][f], m["per_frame"][f][2]]
        assert abs(m["dists"] - sum(v[2] for v in m["per_frame"].values()) / 7) < 1e-12
