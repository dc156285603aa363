"""CPU: the parts of the LPIPS work that need no GPU -- the weight-file layouts `LPIPS.load_weights` takes, properties of the fp64
restatement the GPU tests compare against (tests/lpips_ref.py), the host-side refusals of the library's entry points, the refusal of
CPU tensors, and the shape of the reports of `metrics.summarize` / `score_trees` / `generate.evaluate` with and without a network."""
import json

import pytest
import torch

import lpips_ref as R
import metrics_ref as MR
from conftest import GOLDEN
from test_dist_gloo import _StubPipeline


@pytest.fixture(scope="module")
def weights():
    return R.make_weights(R.WEIGHT_SEED)


def _params(m):
    return {k: v.clone() for k, v in m.state_dict().items()}


def test_both_weight_file_layouts_load_into_the_same_parameters(weights, tmp_path):
    from mv_ldm_amd.lpips import LPIPS
    full = LPIPS(weights=weights)
    want = _params(full)
    assert sorted(want) == sorted(weights) and all(torch.equal(want[k], weights[k]) for k in weights)
    assert len([k for k in want if k.endswith(".weight") and k.startswith("net.")]) == 13
    assert want["lin3.model.1.weight"].shape == (1, 512, 1, 1) and want["net.slice1.0.weight"].shape == (64, 3, 3, 3)
    # the package's ModuleList keeps every lin layer a second time under lins.{k}: accepted, ignored
    dup = dict(weights)
    for k in range(5):
        dup[f"lins.{k}.model.1.weight"] = weights[f"lin{k}.model.1.weight"]
    got = _params(LPIPS(weights=dup))
    assert all(torch.equal(got[k], want[k]) for k in want)
    # torchvision's VGG-16 (features.* and its classifier) + the package's vgg.pth, as files read with weights_only=True
    vgg, lin = R.split_weights(weights)
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    got = _params(LPIPS(weights=tmp_path / "vgg16.pth", lin=str(tmp_path / "vgg.pth")))
    assert all(torch.equal(got[k], want[k]) for k in want)
    torch.save(dup, tmp_path / "full.pth")
    m = LPIPS(allow_random_init=True)
    assert not torch.equal(m.state_dict()["net.slice1.0.weight"], want["net.slice1.0.weight"])
    assert m.load_weights(tmp_path / "full.pth") is m and all(torch.equal(v, want[k]) for k, v in m.state_dict().items())


def test_missing_and_unexpected_keys_are_named(weights):
    from mv_ldm_amd.lpips import LPIPS
    m = LPIPS(allow_random_init=True)
    short = {k: v for k, v in weights.items() if k not in ("net.slice3.12.bias", "lin4.model.1.weight")}
    with pytest.raises(KeyError, match=r"missing keys \['lin4.model.1.weight', 'net.slice3.12.bias'\]"):
        m.load_weights(short)
    with pytest.raises(KeyError, match=r"unexpected keys \['net.slice9.0.weight'\]"):
        m.load_weights({**weights, "net.slice9.0.weight": torch.zeros(1)})
    vgg, lin = R.split_weights(weights)
    with pytest.raises(KeyError, match="lin"):
        m.load_weights(vgg)                                       # a torchvision file alone has no lin layers
    with pytest.raises(KeyError, match=r"unexpected keys \['features.3.weight'\]"):
        m.load_weights({**vgg, "features.3.weight": torch.zeros(1)}, lin)
    with pytest.raises(ValueError, match="net.slice1.0.weight has shape"):
        m.load_weights({**weights, "net.slice1.0.weight": torch.zeros(64, 3, 1, 1)})
    with pytest.raises(ValueError, match="ScalingLayer"):
        m.load_weights({**weights, "scaling_layer.shift": torch.zeros(1, 3, 1, 1)})
    with pytest.raises(NotImplementedError):
        LPIPS(net="alex")
    with pytest.warns(UserWarning, match="RANDOM initial weights"):
        LPIPS()


def test_restatement_properties(weights):
    gt, pred = R.make_pair("noise05", 2, 24, 19, seed=3)
    stats = {}
    ab = R.lpips(gt, pred, weights, normalize=True, stats=stats)
    ba = R.lpips(pred, gt, weights, normalize=True)
    assert ab.dtype == torch.float64 and ab.shape == (2,) and bool((ab > 0).all()) and stats["min_norm"] > 0
    assert float((ab - ba).abs().max()) <= 1e-15 * float(ab.max())                   # symmetric
    same, _ = R.make_pair("identical", 2, 24, 19, seed=4)
    assert torch.equal(R.lpips(same, same.clone(), weights, normalize=True), torch.zeros(2, dtype=torch.float64))
    raw = R.lpips(2 * gt.double() - 1, 2 * pred.double() - 1, weights, normalize=False)
    assert float((raw - ab).abs().max()) <= 1e-12 * float(ab.max())                  # normalize = the 2x - 1 in front
    # more noise, more distance; a pixel whose channels are all <= 0 in both images contributes 0, never NaN
    far = R.lpips(gt, gt + 0.2 * (pred - gt) / 0.05, weights, normalize=True)
    assert bool((far > ab).all())
    fa = -torch.rand(1, 64, 2, 2, dtype=torch.float64)
    assert torch.equal(R.tap_distance(fa, fa - 1, torch.ones(64, dtype=torch.float64)), torch.zeros(1, dtype=torch.float64))


def test_the_committed_bounds_are_those_of_the_restatement_on_the_tests_inputs(weights):
    """tests/golden/lpips_cpu_emulation.json is what tests/golden/make_lpips_bounds.py writes: spot-check one case against a fresh run"""
    g = json.loads((GOLDEN / "lpips_cpu_emulation.json").read_text())
    assert g["weights_seed"] == R.WEIGHT_SEED and [tuple(c) for c in g["cases"]] == R.CASES
    assert sorted(g["worst_rel_err"]) == ["bfloat16", "float16", "float32"]
    assert sorted(g["worst_rel_err"]["float32"]) == ["noise002", "noise05", "random"]
    assert sorted(g["worst_rel_err"]["float16"]) == sorted(g["worst_rel_err"]["bfloat16"]) == ["noise05", "random"]
    n, h, w = 3, 16, 16
    for kind in ("random", "noise002"):
        gt, pred = R.make_pair(kind, n, h, w, seed=R.case_seed(n, h, w))
        want = R.lpips(gt, pred, weights, normalize=True)
        assert torch.allclose(want, torch.tensor(g["want"][R.case_key(kind, n, h, w)], dtype=torch.float64), rtol=1e-12, atol=0)
        e = float(((R.lpips(gt, pred, weights, normalize=True, dtype=torch.float32).double() - want).abs() / want).max())
        assert e <= g["worst_rel_err"]["float32"][kind]
    assert g["min_norm"] >= 1.0


def test_the_library_exports_the_lpips_entry_points_and_refuses_on_the_host():
    from mv_ldm_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.mvldm_abi_version() == 7
    # workgroups per image: 64 quads each at C = 64, 32 at 128, 16 at 256, 8 at 512
    assert lib.mvldm_lpips_tap_slots(64, 64, 64) == 16 and lib.mvldm_lpips_tap_slots(32, 32, 128) == 8
    assert lib.mvldm_lpips_tap_slots(5, 7, 512) == 2 and lib.mvldm_lpips_tap_slots(1, 1, 256) == 1
    assert lib.mvldm_lpips_tap_slots(8, 8, 96) == 0 and lib.mvldm_lpips_tap_slots(8, 8, 576) == 0 and lib.mvldm_lpips_tap_slots(0, 8, 64) == 0
    slots = 16 + 8 + 4 + 2 + 1                                # 64 x 64: 1024, 256, 64, 16, 4 quads
    assert lib.mvldm_lpips_workspace_bytes(3, 64, 64) == 3 * slots * 8
    assert lib.mvldm_lpips_workspace_bytes(1, 15, 64) == 0 and lib.mvldm_lpips_workspace_bytes(1, 64, 15) == 0 and lib.mvldm_lpips_workspace_bytes(0, 64, 64) == 0
    # refusals are decided on the host, before any launch: they can be checked without a device
    err = lambda: lib.mvldm_last_error()
    assert lib.mvldm_lpips_prep(None, None, None, 1, 15, 64, 4, _lib.F32, 1, None) == -1 and b"pool" in err()
    assert lib.mvldm_lpips_prep(None, None, None, 1, 64, 15, 8, _lib.F16, 1, None) == -1 and b"pool" in err()
    assert lib.mvldm_lpips_prep(None, None, None, 1, 64, 64, 8, _lib.F32, 1, None) == -1 and b"c_pad" in err()
    assert lib.mvldm_lpips_prep(None, None, None, 1, 64, 64, 4, _lib.F32, 1, None) == -1 and b"null" in err()
    assert lib.mvldm_lpips_relu(None, 6, _lib.F32, None) == -1 and b"chunk" in err()
    assert lib.mvldm_lpips_relu(None, 64, _lib.F32, None) == -1 and b"null" in err()
    tap = lambda c, nbytes, slot0=0, n=8: lib.mvldm_lpips_tap(None, None, None, 2, 8, 8, c, _lib.F32, None, nbytes, slot0, n, None)
    assert lib.mvldm_lpips_tap_slots(8, 8, 64) == 1
    assert tap(96, 1 << 20) == -1 and b"multiples of 64" in err()
    assert tap(576, 1 << 20) == -1 and b"multiples of 64" in err()
    assert tap(64, 2 * 8 * 8 - 8) == -1 and b"workspace" in err()
    assert tap(64, 1 << 20, slot0=8) == -1 and b"partials" in err()
    assert tap(64, 2 * 8 * 8) == -1 and b"null" in err()
    assert lib.mvldm_lpips_fold(None, 0, 1, 15, 64, None, None) == -1 and b"pool" in err()
    assert lib.mvldm_lpips_fold(None, slots * 8 - 8, 1, 64, 64, None, None) == -1 and b"workspace" in err()
    assert lib.mvldm_lpips_fold(None, slots * 8, 1, 64, 64, None, None) == -1 and b"null" in err()
    assert lib.mvldm_lpips_fold(None, 0, 0, 64, 64, None, None) == 0            # nothing to do is no error


def test_cpu_tensors_raise(weights):
    from mv_ldm_amd import metrics as M
    from mv_ldm_amd.lpips import LPIPS
    m = LPIPS(weights=weights)
    a = torch.rand(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.compute_lpips(a, a, m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.compute_lpips(a.view(1, 2, 3, 16, 16), a.view(1, 2, 3, 16, 16), m)
    with pytest.raises(ValueError):
        M.compute_lpips(a, a[:1], m)


# ---- reports: a stub network (the fp64 restatement) on the CPU -- the plumbing, not the kernels --------------------------------
class _StubLpips:
    def __init__(self, weights):
        self.weights, self.calls = weights, 0

    def __call__(self, in0, in1, normalize=False):
        self.calls += 1
        return R.lpips(in0, in1, self.weights, normalize=normalize).view(-1, 1, 1, 1)


def test_summarize_carries_the_third_column_only_when_it_is_there():
    from mv_ldm_amd import metrics as M
    two = M.summarize({"a": {1: [20.0, 0.5], 2: [30.0, 0.7]}, "b": {1: [40.0, 0.9]}})
    assert sorted(two["overall"]) == ["frames", "psnr", "ssim"] and sorted(two["scenes"]["a"]) == ["frames", "per_frame", "psnr", "ssim"]
    assert two["scenes"]["a"]["psnr"] == 25.0 and abs(two["overall"]["ssim"] - 0.7) < 1e-12
    assert list(two["scenes"]["a"]) == ["psnr", "ssim", "frames", "per_frame"] and list(two["overall"]) == ["psnr", "ssim", "frames"]
    three = M.summarize({"a": {1: [20.0, 0.5, 0.25], 2: [30.0, 0.7, 0.75]}, "b": {1: [40.0, 0.9, 0.5]}})
    assert three["scenes"]["a"]["lpips"] == 0.5 and three["scenes"]["b"]["lpips"] == 0.5 and abs(three["overall"]["lpips"] - 0.5) < 1e-12
    assert three["scenes"]["a"]["psnr"] == two["scenes"]["a"]["psnr"] and three["overall"]["frames"] == 3
    empty = M.summarize({})
    assert sorted(empty["overall"]) == ["frames", "psnr", "ssim"] and empty["overall"]["frames"] == 0


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
    assert sorted(plain) == ["missing", "overall", "scenes"] and sorted(plain["overall"]) == ["frames", "psnr", "ssim"]
    assert all(len(v) == 2 for s in plain["scenes"].values() for v in s["per_frame"].values())
    stub = _StubLpips(weights)
    rep = M.score_trees(tmp_path / "pred", tmp_path / "gt", device="cpu", batch=2, lpips=stub)
    assert stub.calls == 3                                        # scene a in chunks of 2 + 1, scene b
    assert sorted(rep["overall"]) == ["frames", "lpips", "psnr", "ssim"] and sorted(rep["scenes"]["a"]) == ["frames", "lpips", "per_frame", "psnr", "ssim"]
    for s in plain["scenes"]:
        for f, row in plain["scenes"][s]["per_frame"].items():
            got = rep["scenes"][s]["per_frame"][f]
            assert got[:2] == row and len(got) == 3
            p, t = load_image(tmp_path / "pred" / s / "color" / f"{f:0>6}.png")[None], load_image(tmp_path / "gt" / s / "color" / f"{f:0>6}.png")[None]
            want = float(R.lpips(t, p, weights, normalize=True))                 # (ground truth, prediction), normalize=True, as the reference calls it
            assert abs(got[2] - want) <= 1e-12 * want
    assert abs(rep["scenes"]["a"]["lpips"] - sum(v[2] for v in rep["scenes"]["a"]["per_frame"].values()) / 3) < 1e-12


def test_evaluate_adds_lpips_only_when_given_a_network(weights):
    from mv_ldm_amd import generate as G
    from test_metrics_cpu import _examples
    cfg = G.merge_config(G.DEFAULT_CONFIG, {"test": {"sampling_mode": "anchored", "num_anchors_views": 4}, "seed": 7})
    ref = lambda gt, pred: (MR.compute_psnr(gt, pred), MR.compute_ssim(gt, pred))
    ex = _examples([0, 2])
    plain = G.evaluate(cfg, ex, pipe=_StubPipeline(), metric_fn=ref)
    got = G.evaluate(cfg, ex, pipe=_StubPipeline(), metric_fn=ref, lpips=_StubLpips(weights))
    assert sorted(got) == sorted(plain) and sorted(got["metrics"]) == sorted(plain["metrics"]) == ["synthetic0000", "synthetic0002"]
    for i in (0, 2):
        name = ex[i]["scene"][0]
        m, m0 = got["metrics"][name], plain["metrics"][name]
        assert sorted(m0) == ["per_frame", "psnr", "ssim"] and sorted(m) == ["lpips", "per_frame", "psnr", "ssim"]
        assert m["psnr"] == m0["psnr"] and m["ssim"] == m0["ssim"] and isinstance(m["lpips"], float)
        for j, f in enumerate(range(1, 8)):
            want = float(R.lpips(ex[i]["target"]["image"][0, j:j + 1], got["frames"][name][f][None], weights, normalize=True))
            assert m["per_frame"][f][:2] == m0["per_frame"][f] and len(m["per_frame"][f]) == 3
            assert abs(m["per_frame"][f][2] - want) <= 1e-12 * want           # (the stub scores the scene's frames as one batch)
        assert abs(m["lpips"] - sum(v[2] for v in m["per_frame"].values()) / 7) < 1e-12
