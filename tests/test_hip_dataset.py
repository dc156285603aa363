"""GPU: the RE10K reader end to end (mv_ldm_amd/dataset.py over tests/re10k_fixture.py's tree): the images a scene arrives with are the
golden path's (decoded bytes -> PIL's LANCZOS resize -> crop -> / 255, as tests/cropshim_ref.py restates it and tests/test_cropshim_cpu.py
pins it to PIL), `generate.evaluate` scores such scenes without a ground-truth tree, and the CLI reads them."""
import copy
import json

import numpy as np
import pytest
import torch

import cropshim_ref as R
import re10k_fixture as F
from mv_ldm_amd import dataset as D
from mv_ldm_amd import generate as G

pytestmark = pytest.mark.gpu
GRAD_ENABLED = False      # tests/conftest.py::_grad_mode
SHAPE = (32, 32)
# a 4-level UNet over a 2-level VAE: 32 x 32 images are 16 x 16 latents (the shapes of __graft_entry__.smoke)
SMALL = {"denoiser": dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4)),
         "autoencoder": dict(block_out_channels=(32, 64), layers_per_block=1)}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("re10k")
    return root, F.build(root)


def test_scenes_arrive_with_the_golden_path_images(tree):
    root, index = tree
    examples = list(D.RE10KScenes(root, index=index, image_shape=SHAPE))
    assert [e["scene"][0] for e in examples] == ["a_one", "c_two", "d_close", "h_one"]
    for e in examples:
        name = e["scene"][0]
        raw = F.frames(name)
        h_s, w_s, _, _ = R.geometry(*raw.shape[1:3], SHAPE)
        for g in (e["context"], e["target"]):
            idx = g["index"][0].tolist()
            assert g["image"].is_cuda and g["image"].dtype == torch.float32 and tuple(g["image"].shape) == (1, len(idx), 3, *SHAPE)
            assert torch.equal(g["image"][0].cpu(), torch.from_numpy(R.crop_shim(raw[idx], SHAPE))), name
            k = torch.tensor([[F.SCENES[name][2], 0, 0.5], [0, F.SCENES[name][2], 0.5], [0, 0, 1]]).repeat(len(idx), 1, 1)
            assert torch.equal(g["intrinsics"][0], torch.from_numpy(R.scale_intrinsics(k.numpy(), h_s, w_s, SHAPE)))
    assert R.geometry(48, 64, SHAPE) == (32, 43, 0, 5)                # c_two is resized AND cropped; the 64 x 64 scenes only resized
    # the drop-in for a loader that already has float images: the reference's call shapes, CPU tensors in, device tensors out
    raw = F.frames("c_two")
    views = {"image": torch.from_numpy(R.to_float(raw))[None], "intrinsics": torch.eye(3).repeat(1, 5, 1, 1), "index": torch.arange(5)[None]}
    out = D.apply_crop_shim({"context": views, "target": {**views, "image": None}, "scene": ["x"]}, SHAPE)
    assert out["context"]["image"].is_cuda and tuple(out["context"]["image"].shape) == (1, 5, 3, *SHAPE) and out["target"]["image"] is None
    assert torch.equal(out["context"]["image"][0].cpu(), torch.from_numpy(R.crop_shim(R.to_float(raw), SHAPE)))
    assert float(out["context"]["intrinsics"][0, 0, 0, 0]) == np.float32(43 / 32) and float(views["intrinsics"][0, 0, 0, 0]) == 1.0


def _small_cfg():
    cfg = copy.deepcopy(G.DEFAULT_CONFIG)
    cfg["model"]["denoiser"]["autoencoder"]["block_out_channels"] = [64, 128, 256, 256]
    cfg["model"]["scheduler"]["num_inference_steps"] = 2
    cfg["test"]["sampling_mode"] = "autoregressive"                  # three target frames: one call (the anchored walk wants 4 anchors)
    cfg["seed"] = 4
    return cfg


def test_evaluate_scores_dataset_scenes_without_a_ground_truth_tree(tree):
    """two 64 x 64 scenes through the crop shim to 32 x 32, 2 DDIM steps, random-init weights: finite PSNR / SSIM for both"""
    import mv_ldm_amd
    root, index = tree
    cfg = _small_cfg()
    pipe, _ = G.build_pipeline(cfg, device="cuda", allow_random_init=True, overrides=SMALL)
    g = torch.Generator(device="cuda").manual_seed(0)
    for m in (pipe.denoiser, pipe.autoencoder):
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g, device="cuda") * 0.05)
    examples = list(D.RE10KScenes(root, index=index, image_shape=SHAPE, scenes=["a_one", "h_one"]))
    assert [e["scene"][0] for e in examples] == ["a_one", "h_one"]
    with mv_ldm_amd.compute_dtype(torch.float32):
        res = G.evaluate(cfg, examples, pipe=pipe, batch_scenes=2)
    assert sorted(res["frames"]) == sorted(res["metrics"]) == ["a_one", "h_one"]
    for name, want in (("a_one", [1, 2, 3]), ("h_one", [0, 2, 4])):
        m = res["metrics"][name]
        assert sorted(res["frames"][name]) == sorted(m["per_frame"]) == want
        assert np.isfinite(m["psnr"]) and np.isfinite(m["ssim"]) and all(np.isfinite(v).all() for v in m["per_frame"].values())
        for im in res["frames"][name].values():
            assert tuple(im.shape) == (3, *SHAPE) and torch.isfinite(im).all()


def test_cli_reads_a_dataset(tmp_path, capsys):
    """`python -m mv_ldm_amd.generate --dataset ROOT --index INDEX`: the released topology (random init) at --res 64, the smallest frame its
    8 x VAE and four UNet levels take (8 x 8 latents; at --res 32 the decoder's up path meets 1 x 1 skips with a 2 x 2 map), so this
    test's tree has 80 x 96 frames: scaled to 64 x 77, 6 columns cropped from each side"""
    index = F.build(tmp_path, frame_hw=(80, 96))
    rc = G.main(["model.scheduler.num_inference_steps=2", "test.sampling_mode=autoregressive", "seed=1", "--dataset", str(tmp_path), "--index", str(index), "--res", "64", "--scene", "a_one",
                 "--scene", "h_one", "--dtype", "bf16", "--allow-random-init", "--out", str(tmp_path / "frames")])
    assert rc == 0
    text = capsys.readouterr().out
    out = json.loads([l for l in text.splitlines() if l.startswith("{")][-1])
    assert str(tmp_path) in out["data"] and "synthetic" not in out["data"] and out["scenes"] == 2 and out["frames_per_scene"] == 3 and out["views"] == 6 and out["mode"] == "autoregressive"
    assert "a_one: psnr" in text and "h_one: psnr" in text                     # scored without --gt
    assert (tmp_path / "frames" / "h_one" / "color" / "000004.png").exists()
