"""Writes tests/golden/train_loader.json: what the reference's own training data path gives (run where the reference tree and Pillow are;
the tests need only the file).

The reference's classes are imported through `ref_import` (its stubbed `torchvision.transforms.ToTensor` gets a real body here: bytes
/ 255 in float32, channels first) and called directly, without a `DataLoader`:
  (a) `samplers`: `ViewSamplerBounded.sample` / `ViewSamplerArbitrary.sample` under `torch.manual_seed(seed)` -- cfg, stage, flags, step,
      seed, number of views and the indices drawn, or "ValueError";
  (b) `epochs`: two consecutive passes of `DatasetRE10k(stage="train")` over tests/train_fixture.py's tree under ONE `torch.manual_seed`,
      bounded sampler, `augment`, image shape 32 x 32, and one pass of `stage="val"` after them: per example the scene, the indices, the
      cameras and bounds as float lists (a float32 survives JSON's double) and, per view group, the SHA-256 of the cropped image's
      bytes `[v, h, w, 3]`.  The image is checked to be exactly bytes / 255, and to be `cropshim_ref.crop_shim` of the raw frames either
      as they are or mirrored along w -- which of the two is recorded as "flip".

    python tests/golden/make_train_loader_golden.py"""
import json
import sys
import tempfile
import types
from dataclasses import asdict
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))
import cropshim_ref as R  # noqa: E402
import ref_import  # noqa: E402
import train_fixture as F  # noqa: E402

EPOCH_SEED = 3
BASELINE = dict(num_context_views=2, num_target_views=3, min_distance_between_context_views=50, max_distance_between_context_views=180)
WARM_UP = dict(num_context_views=2, num_target_views=1, min_distance_between_context_views=50, max_distance_between_context_views=180,
               max_distance_to_context_views=10, context_gap_warm_up_steps=100, target_gap_warm_up_steps=100,
               initial_min_distance_between_context_views=10, initial_max_distance_between_context_views=20,
               initial_max_distance_to_context_views=0)
WRAP = dict(F.SAMPLER, max_distance_to_context_views=2)
ARBITRARY = dict(num_context_views=2, num_target_views=3)
FIXED = dict(ARBITRARY, context_views=[1, 5], target_views=[0, 2, 4])
SEEDS = (0, 1, 2)


def sampler_cases():
    """(kind, cfg, stage, overfit, circular, step, num_views)"""
    cases = [("bounded", BASELINE, "train", False, False, 0, n) for n in (40, 51, 52, 120, 300)]
    cases += [("bounded", F.SAMPLER, "train", False, False, 0, n) for n in (2, 6, 7, 8)]
    cases += [("bounded", WARM_UP, "train", False, False, step, 300) for step in (0, 50, 100, 1000)]
    cases += [("bounded", BASELINE, "test", False, False, 0, n) for n in (120, 300)]
    cases += [("bounded", WARM_UP, "test", False, False, 50, 300)]
    cases += [("bounded", BASELINE, "train", True, False, 0, n) for n in (120, 300)]
    cases += [("bounded", WRAP, "train", False, True, 0, 8), ("bounded", BASELINE, "train", False, True, 0, 120)]
    cases += [("arbitrary", ARBITRARY, "train", False, False, 0, 10), ("arbitrary", FIXED, "train", False, False, 0, 10)]
    return cases


def main():
    import PIL
    ref_import.install()
    import torchvision.transforms as tf
    tf.ToTensor = lambda: (lambda pic: torch.from_numpy(np.array(pic)).permute(2, 0, 1).contiguous().float().div(255))
    bounded = ref_import.ref("src.dataset.view_sampler.view_sampler_bounded")
    arbitrary = ref_import.ref("src.dataset.view_sampler.view_sampler_arbitrary")
    re10k = ref_import.ref("src.dataset.dataset_re10k")

    def make_sampler(kind, cfg, stage, overfit, circular, step):
        tracker = types.SimpleNamespace(get_step=lambda: step)      # (the reference's StepTracker starts a Manager process)
        if kind == "bounded":
            return bounded.ViewSamplerBounded(bounded.ViewSamplerBoundedCfg(name="bounded", **cfg), stage, overfit, circular, tracker)
        return arbitrary.ViewSamplerArbitrary(arbitrary.ViewSamplerArbitraryCfg(name="arbitrary", **cfg), stage, overfit, circular, tracker)

    samplers = []
    for kind, cfg, stage, overfit, circular, step, num_views in sampler_cases():
        for seed in SEEDS:
            torch.manual_seed(seed)
            try:
                (view_index,) = make_sampler(kind, cfg, stage, overfit, circular, step).sample("scene", num_views)
                result = {k: v.tolist() for k, v in asdict(view_index).items()}
            except ValueError:
                result = "ValueError"
            samplers.append({"kind": kind, "cfg": cfg, "stage": stage, "overfit": overfit, "circular": circular, "step": step,
                             "num_views": num_views, "seed": seed, "result": result})

    raw = {s: F.frames(s) for s in F.SCENES}

    def record(example):
        out = {"scene": example["scene"]}
        flips = set()
        for view in ("context", "target"):
            g = example[view]
            image = g["image"].numpy()
            pixels = np.ascontiguousarray(np.moveaxis(np.rint(image * 255).astype(np.uint8), -3, -1))
            assert np.array_equal(image, R.to_float(pixels))
            frames = raw[example["scene"]][g["index"].tolist()]
            plain, mirrored = R.crop_shim(frames, F.SHAPE), R.crop_shim(frames[:, :, ::-1], F.SHAPE)
            assert not np.array_equal(plain, mirrored)
            assert np.array_equal(image, plain) or np.array_equal(image, mirrored), "cropshim_ref does not reproduce the reference's image"
            flips.add(bool(np.array_equal(image, mirrored)))
            out[view] = {"index": g["index"].tolist(), "extrinsics": g["extrinsics"].tolist(), "intrinsics": g["intrinsics"].tolist(),
                         "near": g["near"].tolist(), "far": g["far"].tolist(), "sha256": R.digest(pixels)}
        (out["flip"],) = flips
        return out

    with tempfile.TemporaryDirectory() as tmp:
        root = F.build(Path(tmp) / "re10k")

        def dataset(stage):
            cfg = re10k.DatasetRE10kCfg(image_shape=list(F.SHAPE), background_color=[0.0, 0.0, 0.0], cameras_are_circular=False, overfit_to_scene=None,
                                        view_sampler=None, scene=None, augment=True, random_transform_extrinsics=False, name="re10k", root=root,
                                        baseline_epsilon=1e-3, max_fov=100.0, make_baseline_1=True)
            return re10k.DatasetRE10k(cfg, stage, make_sampler("bounded", F.SAMPLER, stage, False, False, 0))
        torch.manual_seed(EPOCH_SEED)
        train = dataset("train")
        epochs = [[record(e) for e in train] for _ in range(2)]
        val = [record(e) for e in dataset("val")]
    for epoch in epochs + [val]:
        assert sorted(e["scene"] for e in epoch) == sorted(F.YIELDED), [e["scene"] for e in epoch]
    flips = [e["flip"] for epoch in epochs for e in epoch]
    assert any(flips) and not all(flips), "the recorded epochs need a mirrored and an unmirrored example: pick another EPOCH_SEED"
    assert not any(e["flip"] for e in val)
    path = HERE / "train_loader.json"
    path.write_text(json.dumps({"pil_version": PIL.__version__, "seed": EPOCH_SEED, "shape": list(F.SHAPE), "sampler": F.SAMPLER,
                                "samplers": samplers, "epochs": epochs, "val": val}))
    print(f"{path}: {path.stat().st_size} bytes, PIL {PIL.__version__}, {len(samplers)} sampler cases, orders "
          f"{[[e['scene'] for e in epoch] for epoch in epochs + [val]]}, flips {flips}")


if __name__ == "__main__":
    main()
