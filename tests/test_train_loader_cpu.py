"""CPU: the training data path of mv_ldm_amd/dataset.py against the reference's own (tests/golden/train_loader.json, written by
tests/golden/make_train_loader_golden.py from the reference's classes): both view samplers draw for draw, the step tracker, the
reflection, and `RE10KTrainLoader.examples()` over tests/train_fixture.py's tree -- the order of two consecutive epochs and a validation
pass under one seed, indices, cameras bit for bit, which examples are mirrored.  The images are pinned without a device: the golden's
digests equal `cropshim_ref.crop_shim` of the raw frames, mirrored where flagged -- the expectation the GPU tests hold the device to."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import cropshim_ref as R
import train_fixture as F
from mv_ldm_amd import dataset as D

GOLD = json.loads((Path(__file__).resolve().parent / "golden" / "train_loader.json").read_text())


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return F.build(tmp_path_factory.mktemp("re10k_train"))


@pytest.fixture(scope="module")
def passes(root):
    """what the golden recorded, replayed: one seed, two epochs of ONE train loader, then a validation loader's pass"""
    torch.manual_seed(GOLD["seed"])
    kw = dict(image_shape=F.SHAPE, augment=True, crop=False)
    train = D.RE10KTrainLoader(root, "train", view_sampler=D.get_view_sampler("bounded", stage="train", **F.SAMPLER), **kw)
    epochs = [list(train.examples()) for _ in range(2)]
    val = list(D.RE10KTrainLoader(root, "val", view_sampler=D.get_view_sampler("bounded", stage="val", **F.SAMPLER), **kw).examples())
    return epochs, val


def _case_id(c):
    return f"{c['kind']}-{c['stage']}-n{c['num_views']}-step{c['step']}-o{int(c['overfit'])}c{int(c['circular'])}-{len(c['cfg'])}-s{c['seed']}"


@pytest.mark.parametrize("case", GOLD["samplers"], ids=_case_id)
def test_samplers_draw_what_the_reference_draws(case):
    tracker = D.StepTracker()
    tracker.set_step(case["step"])
    sampler = D.get_view_sampler(case["kind"], stage=case["stage"], overfit=case["overfit"], cameras_are_circular=case["circular"],
                                 step_tracker=tracker, **case["cfg"])
    torch.manual_seed(case["seed"])
    if case["result"] == "ValueError":
        before = torch.get_rng_state()
        with pytest.raises(ValueError):
            sampler.sample("scene", case["num_views"])
        assert torch.equal(torch.get_rng_state(), before)              # refused before any draw
        return
    (got,) = sampler.sample("scene", case["num_views"])
    assert got.context.dtype == torch.int64 and got.context.tolist() == case["result"]["context"]
    assert got.target.dtype == torch.int64 and got.target.tolist() == case["result"]["target"]
    assert sampler.num_context_views == case["cfg"]["num_context_views"] and sampler.num_target_views == case["cfg"]["num_target_views"]


def test_the_golden_holds_every_kind_of_sampler_case():
    cases = GOLD["samplers"]
    assert any(c["result"] == "ValueError" and c["num_views"] == 40 for c in cases) and any(c["stage"] == "test" for c in cases)
    assert any(c["overfit"] for c in cases) and any(c["circular"] for c in cases) and {c["kind"] for c in cases} == {"bounded", "arbitrary"}
    warm = [c for c in cases if c["cfg"].get("context_gap_warm_up_steps") and c["stage"] == "train"]
    assert sorted({c["step"] for c in warm}) == [0, 50, 100, 1000]
    gap = lambda c: c["result"]["context"][1] - c["result"]["context"][0]
    assert all(10 <= gap(c) <= 20 for c in warm if c["step"] == 0) and all(50 <= gap(c) <= 180 for c in warm if c["step"] >= 100)


def test_a_window_of_fewer_frames_than_targets_is_not_caught():
    """2 frames between context views 1 apart, 3 targets without replacement: torch.multinomial's error propagates, as in the reference"""
    sampler = D.ViewSamplerBounded(num_context_views=2, num_target_views=3, min_distance_between_context_views=1, max_distance_between_context_views=1)
    with pytest.raises(RuntimeError):
        sampler.sample("scene", 5)


def test_get_view_sampler_names(tmp_path):
    for name in ("all", "random"):
        with pytest.raises(NotImplementedError):
            D.get_view_sampler(name)
    with pytest.raises(KeyError):
        D.get_view_sampler("nearest")
    ev = D.get_view_sampler("evaluation", stage="test", index={"a": [{"context": (0,), "target": (1, 2)}], "b": None})
    assert [(c.tolist(), t.tolist()) for c, t in ev.sample("a", 3)] == [([0], [1, 2])] and ev.total_samples == 1
    with pytest.raises(ValueError):
        ev.sample("b", 3)


def test_step_tracker():
    t = D.StepTracker()
    assert t.get_step() == 0
    t.set_step(7)
    assert t.get_step() == 7
    t = D.StepTracker(offset=100)
    assert t.get_step() == 100
    t.set_step(5)
    assert t.get_step() == 105
    s = D.ViewSamplerBounded(step_tracker=t)
    assert s.global_step == 105 and D.ViewSamplerBounded().global_step == 0
    assert s.schedule(10, 50, 210) == 30 and s.schedule(10, 50, 100) == 50 and s.schedule(0, 7, 210) == 3


def test_reflect_extrinsics():
    e = torch.randn(2, 3, 4, 4, generator=torch.Generator().manual_seed(1))
    m = torch.diag(torch.tensor([-1.0, 1.0, 1.0, 1.0]))
    got = D.reflect_extrinsics(e)
    assert torch.equal(got, m @ e @ m) and torch.equal(D.reflect_extrinsics(got), e)
    sign = torch.tensor([[1, -1, -1, -1], [-1, 1, 1, 1], [-1, 1, 1, 1], [-1, 1, 1, 1.0]])
    assert torch.equal(got, e * sign)


def _check_example(got, want):
    assert got["scene"] == want["scene"] and got["flip"] == want["flip"]
    for view in ("context", "target"):
        g, w = got[view], want[view]
        assert g["index"].tolist() == w["index"]
        for name in ("extrinsics", "intrinsics", "near", "far"):
            assert g[name].dtype == torch.float32 and torch.equal(g[name], torch.tensor(w[name], dtype=torch.float32)), (want["scene"], view, name)
        assert g["frames"].dtype == np.uint8 and g["frames"].shape == (len(w["index"]), F.H, F.W, 3)
        assert np.array_equal(g["frames"], F.frames(want["scene"])[w["index"]])          # decoded, not mirrored


def test_examples_follow_the_reference_over_two_epochs_and_a_validation_pass(passes):
    epochs, val = passes
    for got, want in zip(epochs + [val], GOLD["epochs"] + [GOLD["val"]]):
        assert [e["scene"] for e in got] == [e["scene"] for e in want]
        assert sorted(e["scene"] for e in got) == sorted(F.YIELDED)                        # 3 of 6 scenes
        for g, w in zip(got, want):
            _check_example(g, w)
    flips = [e["flip"] for epoch in epochs for e in epoch]
    assert any(flips) and not all(flips) and not any(e["flip"] for e in val)              # only stage "train" augments
    assert [e["scene"] for e in epochs[0]] != [e["scene"] for e in epochs[1]] or [e["scene"] for e in epochs[0]] != [e["scene"] for e in val]
    mirrored = next(e for epoch in epochs for e in epoch if e["flip"])
    assert float(mirrored["context"]["extrinsics"][1, 0, 3]) < 0 < float(mirrored["context"]["near"][0])      # the baseline points along -x


def test_each_skip_rule_is_hit(root, capsys):
    """the three scenes that never arrive leave for three different reasons, and each draws what the reference draws on its way out"""
    fov = lambda s: float(D.get_fov(D.convert_poses(F.cameras(s))[1]).rad2deg().max())
    assert fov("s_wide") > 100.0 > max(fov(s) for s in F.SCENES if s != "s_wide")
    sampler = D.get_view_sampler("bounded", **F.SAMPLER)
    torch.manual_seed(0)
    before = torch.get_rng_state()
    with pytest.raises(ValueError):
        sampler.sample("s_short", F.SCENES["s_short"][0])
    assert torch.equal(torch.get_rng_state(), before)
    loader = D.RE10KTrainLoader(root, view_sampler=sampler, image_shape=F.SHAPE, scenes=["s_close"], crop=False)
    assert list(loader.examples()) == [] and "Skipped s_close because of insufficient baseline" in capsys.readouterr().out
    assert not torch.equal(torch.get_rng_state(), before)                                  # skipped AFTER the sampler's draws
    for s in ("s_wide", "s_short"):
        loader = D.RE10KTrainLoader(root, view_sampler=sampler, image_shape=F.SHAPE, scenes=[s], crop=False)
        torch.manual_seed(0)
        torch.randperm(1), torch.randperm(1)                                               # the chunk list's and the chunk's shuffles
        state = torch.get_rng_state()
        torch.manual_seed(0)
        assert list(loader.examples()) == [] and torch.equal(torch.get_rng_state(), state), s


def test_golden_digests_are_the_numpy_shim_of_the_frames_mirrored_where_flagged():
    n = {True: 0, False: 0}
    for epoch in GOLD["epochs"] + [GOLD["val"]]:
        for e in epoch:
            raw = F.frames(e["scene"])
            for view in ("context", "target"):
                frames = raw[e[view]["index"]]
                want = R.resize_crop_u8(frames[:, :, ::-1] if e["flip"] else frames, F.SHAPE)
                other = R.resize_crop_u8(frames if e["flip"] else frames[:, :, ::-1], F.SHAPE)
                assert R.digest(want) == e[view]["sha256"] != R.digest(other), (e["scene"], view)
                # resize-then-flip is not the reference's image: PIL's tables are not mirror-symmetric
                assert not e["flip"] or R.digest(np.ascontiguousarray(R.resize_crop_u8(frames, F.SHAPE)[:, :, ::-1])) != e[view]["sha256"]
            n[e["flip"]] += 1
    assert n[True] and n[False]


def test_batches_and_drop_last(root):
    kw = dict(view_sampler=D.get_view_sampler("bounded", **F.SAMPLER), image_shape=F.SHAPE, augment=True, crop=False)
    torch.manual_seed(GOLD["seed"])
    batches = list(D.RE10KTrainLoader(root, batch_size=2, **kw))
    assert len(batches) == 1                                                               # 3 examples: the last one is dropped
    (b,) = batches
    want = GOLD["epochs"][0][:2]
    assert b["scene"] == [e["scene"] for e in want] and b["flip"].tolist() == [e["flip"] for e in want]
    for view, v in (("context", 2), ("target", 3)):
        g = b[view]
        assert g["image"].dtype == torch.uint8 and tuple(g["image"].shape) == (2, v, F.H, F.W, 3)
        assert tuple(g["extrinsics"].shape) == (2, v, 4, 4) and tuple(g["intrinsics"].shape) == (2, v, 3, 3)
        assert tuple(g["near"].shape) == tuple(g["far"].shape) == tuple(g["index"].shape) == (2, v)
        for i, e in enumerate(want):
            assert g["index"][i].tolist() == e[view]["index"] and torch.equal(g["extrinsics"][i], torch.tensor(e[view]["extrinsics"]))
            assert np.array_equal(g["image"][i].numpy(), F.frames(e["scene"])[e[view]["index"]])
    torch.manual_seed(GOLD["seed"])
    kept = list(D.RE10KTrainLoader(root, batch_size=2, drop_last=False, decode_workers=3, **kw))
    assert [len(x["scene"]) for x in kept] == [2, 1] and kept[1]["scene"] == [GOLD["epochs"][0][2]["scene"]]
    assert torch.equal(kept[0]["target"]["image"], b["target"]["image"])                   # threads decode the same frames in the same order
    assert D.RE10KTrainLoader(root, decode_workers=99, **kw).decode_workers == 16


def test_what_is_not_built_says_so(root):
    with pytest.raises(NotImplementedError):
        D.RE10KTrainLoader(root, random_transform_extrinsics=True)
    with pytest.raises(ValueError):
        D.RE10KTrainLoader(root, stage="test")
