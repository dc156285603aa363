"""CPU: the parts of the image-metric work that need no GPU -- the fp64 restatement the GPU tests compare against
(tests/metrics_ref.py) pinned to scipy's Gaussian filter, the PNG-tree pairing of `python -m mv_ldm_amd.metrics`, the shape of
`generate.evaluate`'s result with and without ground truth, and the refusal of CPU tensors."""
import pytest
import torch

import metrics_ref as R
from test_dist_gloo import _StubPipeline


@pytest.mark.parametrize("use_sample_covariance", [True, False])
def test_restatement_agrees_with_scipy_gaussian_filter_plus_crop(use_sample_covariance):
    """skimage's recipe literally: scipy.ndimage.gaussian_filter(sigma=1.5, truncate=3.5, mode="reflect") of the full image, S on the
    full map, crop 5 per side, mean.  The valid-convolution restatement must agree to 1e-10."""
    ndi = pytest.importorskip("scipy.ndimage")
    import numpy as np
    f = lambda a: ndi.gaussian_filter(a, sigma=1.5, truncate=3.5, mode="reflect")
    n = 121 / 120 if use_sample_covariance else 1.0
    worst = 0.0
    for kind in R.KINDS:
        for h, w in ((11, 11), (12, 19), (37, 45), (64, 64)):
            gt, pred = R.make_pair(kind, 2, 3, h, w, seed=h + w)
            got = R.compute_ssim(gt, pred, use_sample_covariance)
            for i in range(2):
                per_channel = []
                for ch in range(3):
                    x, y = gt[i, ch].double().numpy(), pred[i, ch].double().numpy()
                    ux, uy = f(x), f(y)
                    vx, vy, vxy = n * (f(x * x) - ux * ux), n * (f(y * y) - uy * uy), n * (f(x * y) - ux * uy)
                    s = ((2 * ux * uy + R.C1) * (2 * vxy + R.C2)) / ((ux * ux + uy * uy + R.C1) * (vx + vy + R.C2))
                    per_channel.append(s[5:h - 5, 5:w - 5].mean())
                worst = max(worst, abs(float(got[i]) - float(np.mean(per_channel))))
    assert worst <= 1e-10, worst


def test_restatement_basics():
    gt, pred = R.make_pair("identical", 2, 3, 20, 20)
    assert torch.equal(R.compute_ssim(gt, pred), torch.ones(2, dtype=torch.float64)) and bool(torch.isposinf(R.compute_psnr(gt, pred)).all())
    assert abs(float(R.gaussian_taps().sum()) - 1.0) < 1e-15 and R.gaussian_taps().numel() == 11
    gt, pred = R.make_pair("out_of_range", 1, 1, 16, 16)
    assert torch.equal(R.compute_psnr(gt, pred), R.compute_psnr(gt.clip(0, 1), pred.clip(0, 1)))
    assert not torch.equal(R.compute_ssim(gt, pred), R.compute_ssim(gt.clip(0, 1), pred.clip(0, 1)))
    gt, pred = R.make_pair("noise002", 4, 3, 64, 64)
    assert 0.998 < float(R.compute_ssim(gt, pred).mean()) < 0.9999


def _tree(root, layout):
    from mv_ldm_amd.image_io import save_image
    for scene, names in layout.items():
        for k, name in enumerate(names):
            save_image(torch.full((3, 4, 4), (k + 1) / 10), root / scene / "color" / name)


def test_png_trees_are_paired_by_scene_and_frame_index(tmp_path):
    from mv_ldm_amd import metrics as M
    from mv_ldm_amd.image_io import load_image
    _tree(tmp_path / "pred", {"a": ["000001.png", "000002.png", "000010.png"], "b": ["000001.png"], "only_pred": ["000001.png"]})
    _tree(tmp_path / "gt", {"a": ["1.png", "000002.png", "000003.png"], "b": ["000001.png"], "only_gt": ["000005.png"]})
    (tmp_path / "gt" / "a" / "color" / "notes.png").write_bytes(b"")              # no integer stem: ignored
    (tmp_path / "gt" / "stray").mkdir()                                           # no color/ directory: no scene
    pred, gt = M.scan_tree(tmp_path / "pred"), M.scan_tree(tmp_path / "gt")
    assert sorted(pred) == ["a", "b", "only_pred"] and sorted(pred["a"]) == [1, 2, 10]
    assert sorted(gt) == ["a", "b", "only_gt"] and sorted(gt["a"]) == [1, 2, 3]   # "1.png" and "000001.png" are both frame 1
    pairs, missing = M.pair_trees(pred, gt)
    assert sorted(pairs) == ["a", "b"] and [i for i, _, _ in pairs["a"]] == [1, 2] and [i for i, _, _ in pairs["b"]] == [1]
    assert pairs["a"][0][1].name == "000001.png" and pairs["a"][0][2].name == "1.png"
    assert missing == [("frame", "a", 3, "pred"), ("frame", "a", 10, "gt"), ("scene", "only_gt", None, "pred"), ("scene", "only_pred", None, "gt")]
    assert M.pair_trees({}, {}) == ({}, []) and M.scan_tree(tmp_path / "nowhere") == {}
    assert M.pair_trees({"s": {1: "p"}}, {"s": {2: "g"}}) == ({}, [("frame", "s", 1, "gt"), ("frame", "s", 2, "pred")])
    im = load_image(pairs["a"][1][1])
    assert im.shape == (3, 4, 4) and im.dtype == torch.float32 and torch.equal(im, torch.full((3, 4, 4), 51 / 255))      # 0.2 * 255 truncated
    rep = M.summarize({"a": {1: [20.0, 0.5], 2: [30.0, 0.7]}, "b": {1: [40.0, 0.9]}})
    assert rep["scenes"]["a"]["psnr"] == 25.0 and rep["scenes"]["a"]["frames"] == 2 and rep["overall"]["frames"] == 3
    assert abs(rep["overall"]["psnr"] - 30.0) < 1e-12 and abs(rep["overall"]["ssim"] - 0.7) < 1e-12


def _examples(with_gt):
    from mv_ldm_amd import generate as G
    ex = [G.synthetic_example(i, 7, 32, 7) for i in range(3)]
    for i in with_gt:
        ex[i]["target"]["image"] = torch.rand(1, 7, 3, 32, 32, generator=torch.Generator().manual_seed(i))
    return ex


def test_evaluate_reports_metrics_only_where_there_is_ground_truth():
    """the stub pipeline of the harness tests (CPU) and the fp64 restatement as `metric_fn`: the plumbing, not the kernel"""
    from mv_ldm_amd import generate as G
    cfg = G.merge_config(G.DEFAULT_CONFIG, {"test": {"sampling_mode": "anchored", "num_anchors_views": 4}, "seed": 7})
    ref = lambda gt, pred: (R.compute_psnr(gt, pred), R.compute_ssim(gt, pred))
    plain = G.evaluate(cfg, _examples([]), pipe=_StubPipeline())
    assert sorted(plain) == ["frames", "leaf_batch", "owned", "sample_calls", "seconds", "views", "views_per_rank"]      # exactly as before
    ex = _examples([0, 2])
    got = G.evaluate(cfg, ex, pipe=_StubPipeline(), metric_fn=ref)
    assert sorted(got) == sorted([*plain, "metrics"]) and sorted(got["metrics"]) == ["synthetic0000", "synthetic0002"]
    for name in plain["frames"]:                                     # scoring changes no frame
        assert all(torch.equal(got["frames"][name][f], im) for f, im in plain["frames"][name].items())
    for i in (0, 2):
        name = ex[i]["scene"][0]
        m = got["metrics"][name]
        assert sorted(m) == ["per_frame", "psnr", "ssim"] and sorted(m["per_frame"]) == list(range(1, 8))
        assert isinstance(m["psnr"], float) and isinstance(m["ssim"], float)
        for j, f in enumerate(range(1, 8)):                          # frame f is scored against target view j, whose index is f
            p, s = ref(ex[i]["target"]["image"][0, j:j + 1], got["frames"][name][f][None])
            assert m["per_frame"][f] == [float(p), float(s)]
        assert abs(m["psnr"] - sum(v[0] for v in m["per_frame"].values()) / 7) < 1e-12
    # a frame limit: only the generated frames are scored
    cfg["test"]["limit_frames"] = 4
    few = G.evaluate(cfg, ex, pipe=_StubPipeline(), metric_fn=ref)
    assert all(sorted(m["per_frame"]) == sorted(few["frames"][n]) and len(m["per_frame"]) < 7 for n, m in few["metrics"].items())
    # without metric_fn the device kernel is the scorer, and CPU frames are refused like everywhere else
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.evaluate(cfg, ex, pipe=_StubPipeline())


def test_ground_truth_from_a_png_tree(tmp_path):
    from mv_ldm_amd import generate as G
    from mv_ldm_amd.image_io import save_image
    ex = _examples([])
    truth = torch.rand(7, 3, 32, 32, generator=torch.Generator().manual_seed(5))
    for j in range(7):
        save_image(truth[j], tmp_path / "synthetic0001" / "color" / f"{j + 1:0>6}.png")
    for j in range(3):                                               # scene 2: incomplete
        save_image(truth[j], tmp_path / "synthetic0002" / "color" / f"{j + 1:0>6}.png")
    assert G.attach_ground_truth(ex, tmp_path) == ["synthetic0000", "synthetic0002"]
    assert ex[0]["target"]["image"] is None and ex[2]["target"]["image"] is None
    got = ex[1]["target"]["image"]
    assert got.shape == (1, 7, 3, 32, 32) and torch.equal(got[0], (truth * 255).to(torch.uint8).float() / 255)


def test_cpu_tensors_raise():
    from mv_ldm_amd import metrics as M, ops
    a = torch.rand(2, 3, 16, 16)
    for fn in (M.compute_psnr, M.compute_ssim, M.image_metrics, ops.image_metrics):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.image_metrics(a.view(1, 2, 3, 16, 16), a.view(1, 2, 3, 16, 16))
    with pytest.raises(ValueError):
        M.image_metrics(a, a[:1])


def test_the_library_exports_the_metric_entry_points():
    from mv_ldm_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.mvldm_abi_version() == 7
    assert lib.mvldm_image_metrics_workspace_bytes(2, 3, 64, 64) == 2 * 3 * 4 * 16
    assert lib.mvldm_image_metrics_workspace_bytes(2, 3, 10, 64) == 0 and lib.mvldm_image_metrics_workspace_bytes(2, 0, 64, 64) == 0
    # refusals are decided on the host, before any launch: they can be checked without a device
    assert lib.mvldm_image_metrics(None, None, 1, 3, 10, 64, 1, None, None, None, 0, None) == -1 and b"window" in lib.mvldm_last_error()
    assert lib.mvldm_image_metrics(None, None, 1, 3, 64, 64, 1, None, None, None, 0, None) == -1 and b"null" in lib.mvldm_last_error()
