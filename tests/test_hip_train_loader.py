"""GPU: the training loader end to end (mv_ldm_amd/dataset.py `RE10KTrainLoader` over tests/train_fixture.py's tree): the batches carry the
reference's examples (tests/golden/train_loader.json) with the images made on the device -- one flagged crop-shim call per batch, mirrored
examples and unmirrored ones together -- `MVLDMTrainer` trains on them, and `python -m mv_ldm_amd.train` runs, saves and resumes."""
import json

import numpy as np
import pytest
import torch

import cropshim_ref as R
import train_fixture as F
from mv_ldm_amd import dataset as D
from test_hip_dataset import SMALL
from test_train_loader_cpu import GOLD

pytestmark = pytest.mark.gpu
GRAD_ENABLED = False      # tests/conftest.py::_grad_mode
WIDTHS = "model.denoiser.autoencoder.block_out_channels=[64, 128, 256, 256]"


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return F.build(tmp_path_factory.mktemp("re10k_train"))


def _loader(root, **kw):
    kw = {**dict(view_sampler=D.get_view_sampler("bounded", **F.SAMPLER), image_shape=F.SHAPE, batch_size=2, augment=True), **kw}
    return D.RE10KTrainLoader(root, **kw)


def test_batches_carry_the_reference_examples_with_device_images(root, monkeypatch):
    from mv_ldm_amd import ops
    calls = []
    real = ops.crop_shim

    def counted(images, shape, ws=None, flip=None):
        calls.append((tuple(images.shape), None if flip is None else flip.tolist()))
        return real(images, shape, ws, flip)
    monkeypatch.setattr(ops, "crop_shim", counted)
    torch.manual_seed(GOLD["seed"])
    loader = _loader(root, drop_last=False)
    mixed = 0
    for want in GOLD["epochs"]:
        batches = list(loader)
        assert [b["scene"] for b in batches] == [[e["scene"] for e in want[:2]], [want[2]["scene"]]]
        for b, examples in zip(batches, (want[:2], want[2:])):
            mixed += len({e["flip"] for e in examples}) == 2
            for view, v in (("context", 2), ("target", 3)):
                g = b[view]
                assert g["image"].is_cuda and g["image"].dtype == torch.float32 and tuple(g["image"].shape) == (len(examples), v, 3, *F.SHAPE)
                for i, e in enumerate(examples):
                    for name in ("extrinsics", "intrinsics", "near", "far"):
                        assert not g[name].is_cuda and torch.equal(g[name][i], torch.tensor(e[view][name], dtype=torch.float32)), (e["scene"], view, name)
                    assert g["index"][i].tolist() == e[view]["index"]
                    frames = F.frames(e["scene"])[e[view]["index"]]
                    image = g["image"][i].cpu()
                    assert torch.equal(image, torch.from_numpy(R.crop_shim(frames[:, :, ::-1] if e["flip"] else frames, F.SHAPE))), (e["scene"], view)
                    pixels = (image * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
                    assert R.digest(pixels) == e[view]["sha256"]
    # one call per batch, all 5 views of every example in it, the flag of an example on each of its frames
    flat = [e for want in GOLD["epochs"] for e in want]
    assert [c[0] for c in calls] == [(10, F.H, F.W, 3), (5, F.H, F.W, 3)] * 2
    assert [c[1] for c in calls] == [[int(e["flip"]) for e in flat[a:b] for _ in range(5)] for a, b in ((0, 2), (2, 3), (3, 5), (5, 6))]
    assert mixed >= 1                                                       # a batch with a mirrored and an unmirrored example went through one call


def test_decode_threads_give_the_same_batches(root):
    got = []
    for workers in (0, 4):
        torch.manual_seed(11)
        got.append(list(_loader(root, drop_last=False, decode_workers=workers)))
        state = torch.get_rng_state()
        got[-1].append(state)
    assert torch.equal(got[0].pop(), got[1].pop()) and len(got[0]) == len(got[1]) == 2
    for a, b in zip(*got):
        assert a["scene"] == b["scene"]
        for view in ("context", "target"):
            for name, t in a[view].items():
                assert torch.equal(t, b[view][name]), (view, name)


def test_the_drop_in_shim_mirrors_on_the_coin():
    """`apply_augmentation_and_crop_shim` on a reference-shaped example (float images, CPU): the reference's coin from the generator, then
    for a mirrored example reflected extrinsics, untouched-but-rescaled intrinsics and the images of the reversed frames"""
    raw = R.make_images("drop_in", 45, 80, "noise", n=5)
    k = torch.eye(3).repeat(5, 1, 1)
    e = torch.randn(5, 4, 4, generator=torch.Generator().manual_seed(2))
    example = {"scene": "x", "context": {"image": torch.from_numpy(R.to_float(raw[:2])), "intrinsics": k[:2], "extrinsics": e[:2]},
               "target": {"image": torch.from_numpy(R.to_float(raw[2:])), "intrinsics": k[2:], "extrinsics": e[2:]}}
    seen = set()
    for seed in range(8):
        flip = not bool(torch.rand(tuple(), generator=torch.Generator().manual_seed(seed)) < 0.5)
        out = D.apply_augmentation_and_crop_shim(example, F.SHAPE, generator=torch.Generator().manual_seed(seed))
        for view, part in (("context", raw[:2]), ("target", raw[2:])):
            g = out[view]
            assert torch.equal(g["image"].cpu(), torch.from_numpy(R.crop_shim(part[:, :, ::-1] if flip else part, F.SHAPE)))
            assert torch.equal(g["extrinsics"], D.reflect_extrinsics(example[view]["extrinsics"]) if flip else example[view]["extrinsics"])
            assert torch.equal(g["intrinsics"], torch.from_numpy(R.scale_intrinsics(example[view]["intrinsics"].numpy(), 32, 57, F.SHAPE)))
        seen.add(flip)
    assert seen == {True, False} and out["scene"] == "x" and float(example["context"]["intrinsics"][0, 0, 0]) == 1.0


def _small_cfg():
    import copy

    from mv_ldm_amd import generate as G
    cfg = copy.deepcopy(G.DEFAULT_CONFIG)
    cfg["model"]["denoiser"]["autoencoder"]["block_out_channels"] = [64, 128, 256, 256]
    return cfg


def test_the_trainer_takes_the_batches(root):
    """one `training_step` per batch on the reduced models of tests/test_hip_dataset.py, f32: a finite loss and gradients that moved"""
    import mv_ldm_amd
    from mv_ldm_amd import generate as G
    from mv_ldm_amd.train import MVLDMTrainer
    mv_ldm_amd.set_compute_dtype(torch.float32)
    pipe, _ = G.build_pipeline(_small_cfg(), device="cuda", allow_random_init=True, overrides=SMALL)
    g = torch.Generator(device="cuda").manual_seed(0)
    for m in (pipe.denoiser, pipe.autoencoder):
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g, device="cuda") * 0.05)
    tr = MVLDMTrainer(pipe.denoiser, pipe.autoencoder, pipe.scheduler, dtype=torch.float32, rays=pipe.rays)
    torch.manual_seed(GOLD["seed"])
    np.random.seed(GOLD["seed"])
    loader = _loader(root)
    batches = [b for _ in range(2) for b in loader]
    assert len(batches) == 2 and all(len(b["scene"]) == 2 for b in batches)
    for b in batches:
        loss = float(tr.training_step(b))
        torch.cuda.synchronize()
        assert np.isfinite(loss) and loss > 0
        assert float(tr.flat.grad.abs().max()) > 0 and torch.isfinite(tr.flat.grad).all()
    assert tr.global_step == 1


def test_the_entry_point_trains_saves_and_resumes(root, tmp_path, capsys):
    from mv_ldm_amd import train as T
    ckpt = tmp_path / "last.ckpt"
    common = [WIDTHS, "trainer.precision=32", "dataset.augment=true", "dataset.view_sampler.min_distance_between_context_views=2",
              "dataset.view_sampler.max_distance_between_context_views=4", "--dataset", str(root), "--batch", "2", "--res", "32", "--log-every", "1"]
    lines = lambda: [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert T.main(common + ["--steps", "2", "--seed", "5", "--save", str(ckpt), "--allow-random-init"], overrides=SMALL) == 0
    first = lines()
    assert [l["step"] for l in first] == [1, 2] and first[-1]["final"] and first[-1]["steps"] == 2 and ckpt.exists()
    assert T.main(common + ["--steps", "1", "--seed", "6", "--resume", str(ckpt)], overrides=SMALL) == 0
    second = lines()
    assert [l["step"] for l in second] == [3] and second[-1]["final"] and second[-1]["steps"] == 1 and second[-1]["weights"] == "checkpoint"
    for l in first + second:
        assert np.isfinite(l["loss"]) and l["loss"] > 0 and l["lr"] > 0 and l["views_per_s"] > 0
    assert second[0]["lr"] > first[-1]["lr"] > first[0]["lr"]               # the LinearLR warm-up went on where it stopped
    assert first[-1]["data"].startswith(str(root)) and first[-1]["dtype"] == "float32"
