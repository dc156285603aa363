"""CPU: the RE10K reader's host side (mv_ldm_amd/dataset.py) on a small tree in the dataset's format (tests/re10k_fixture.py): poses,
field of view, the evaluation index, which scenes and entries are skipped, the world rescale, indices and bounds, the order, decoding.
`crop=False` keeps the device out of it: the view groups then carry the decoded frames; the cropped pixels are tests/test_hip_dataset.py's."""
import math

import numpy as np
import pytest
import torch

import re10k_fixture as F
from mv_ldm_amd import dataset as D


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("re10k")
    return root, F.build(root)


@pytest.fixture(scope="module")
def examples(tree):
    root, index = tree
    return list(D.RE10KScenes(root, index=index, image_shape=(32, 32), crop=False))


def test_convert_poses_against_a_hand_inverted_matrix():
    extrinsics, intrinsics = D.convert_poses(F.cameras("c_two"))
    assert extrinsics.dtype == intrinsics.dtype == torch.float32 and extrinsics.shape == (5, 4, 4) and intrinsics.shape == (5, 3, 3)
    assert (extrinsics.double() - F.camera_to_world("c_two")).abs().max() < 1e-6        # fp32 inverse of a rigid motion
    assert torch.equal(intrinsics[3], torch.tensor([[0.8, 0, 0.5], [0, 0.8, 0.5], [0, 0, 1.0]]))


def test_get_fov():
    k = torch.eye(3).repeat(2, 1, 1)
    k[:, 0, 2] = k[:, 1, 2] = 0.5
    k[0, 0, 0], k[0, 1, 1], k[1, 0, 0], k[1, 1, 1] = 0.5, 1.0, 0.3, 0.9
    want = torch.tensor([[2 * math.atan(1.0), 2 * math.atan(0.5)], [2 * math.atan(0.5 / 0.3), 2 * math.atan(0.5 / 0.9)]])
    assert (D.get_fov(k) - want).abs().max() < 1e-5
    assert D.get_fov(k).rad2deg()[1, 0] > 100 > D.get_fov(k).rad2deg()[0, 0]


def test_load_index_drops_scenes_without_entries(tree):
    index = D.load_index(tree[1])
    assert sorted(index) == ["a_one", "b_wide", "c_two", "d_close", "h_one", "z_absent"]
    assert index["c_two"] == [{"context": (0, 4), "target": (1, 2, 3)}] and len(index["d_close"]) == 2


def test_scene_order_and_skips(examples):
    """files in sorted order, scenes in chunk order, entries in index order; b_wide (field of view), e_missing and f_null (no entry),
    d_close's first entry (baseline below epsilon) are left out"""
    assert [e["scene"] for e in examples] == [["a_one"], ["c_two"], ["d_close"], ["h_one"]]
    assert examples[2]["context"]["index"].tolist() == [[2]] and examples[2]["target"]["index"].tolist() == [[3, 4]]


def test_thresholds_decide_the_skips(tree):
    root, index = tree
    names = lambda **kw: [e["scene"][0] for e in D.RE10KScenes(root, index=index, image_shape=(32, 32), crop=False, **kw)]
    assert names(max_fov=120.0) == ["a_one", "b_wide", "c_two", "d_close", "h_one"]
    assert names(max_fov=55.0) == ["h_one"]                                            # fx = 1.1: 49 degrees; 0.9: 58; 0.8: 64
    wide = list(D.RE10KScenes(root, index=index, image_shape=(32, 32), crop=False, baseline_epsilon=1e-4))
    assert [e["scene"][0] for e in wide] == ["a_one", "c_two", "d_close", "d_close", "h_one"]
    assert [e["scene"][0] for e in D.RE10KScenes(root, index=index, image_shape=(32, 32), crop=False, make_baseline_1=False)] \
        == ["a_one", "c_two", "d_close", "d_close", "h_one"]


def test_view_groups_have_the_batched_example_schema(examples):
    a = examples[0]
    c, t = a["context"], a["target"]
    assert c["index"].tolist() == [[0]] and t["index"].tolist() == [[1, 2, 3]] and t["index"].dtype == torch.int64
    assert c["extrinsics"].shape == (1, 1, 4, 4) and t["extrinsics"].shape == (1, 3, 4, 4) and t["intrinsics"].shape == (1, 3, 3, 3)
    assert t["near"].shape == t["far"].shape == (1, 3) and torch.equal(t["near"], torch.full((1, 3), 0.1)) and torch.equal(t["far"], torch.full((1, 3), 1000.0))
    assert (t["extrinsics"][0].double() - F.camera_to_world("a_one")[1:4]).abs().max() < 1e-6
    assert set(c) == set(t) == {"extrinsics", "intrinsics", "image", "near", "far", "index"}
    h = examples[3]
    assert h["context"]["index"].tolist() == [[1]] and h["target"]["index"].tolist() == [[0, 2, 4]]
    assert torch.equal(h["target"]["intrinsics"][0, 1], torch.tensor([[1.1, 0, 0.5], [0, 1.1, 0.5], [0, 0, 1.0]]))


def test_two_context_views_rescale_the_world(examples, tree):
    c = examples[1]
    assert c["context"]["index"].tolist() == [[0, 4]]
    a, b = c["context"]["extrinsics"][0, :, :3, 3]
    assert abs(float((a - b).norm()) - 1.0) < 1e-6
    want = F.camera_to_world("c_two")
    want[:, :3, 3] /= 2.0
    assert (c["target"]["extrinsics"][0].double() - want[1:4]).abs().max() < 1e-6      # positions scaled, rotations kept
    for g in (c["context"], c["target"]):
        assert torch.allclose(g["near"], torch.full_like(g["near"], 0.1 / 2.0), rtol=1e-6) and torch.allclose(g["far"], torch.full_like(g["far"], 1000.0 / 2.0), rtol=1e-6)
    root, index = tree
    plain = [e for e in D.RE10KScenes(root, index=index, image_shape=(32, 32), crop=False, make_baseline_1=False) if e["scene"] == ["c_two"]][0]
    assert (plain["target"]["extrinsics"][0].double() - F.camera_to_world("c_two")[1:4]).abs().max() < 1e-6
    assert torch.equal(plain["target"]["near"], torch.full((1, 3), 0.1))


def test_frames_decode_to_the_stored_bytes(examples):
    """pixel values that need no device: the decoded frames of each group, and a source that is not 360 x 640"""
    for e in examples:
        raw = F.frames(e["scene"][0])
        for g in (e["context"], e["target"]):
            assert g["image"].dtype == torch.uint8 and np.array_equal(g["image"][0].numpy(), raw[g["index"][0].tolist()])
    assert examples[1]["target"]["image"].shape == (1, 3, 48, 64, 3)


def test_scene_selection_goes_through_the_chunk_index(tree):
    root, index = tree
    got = list(D.RE10KScenes(root, index=index, image_shape=(32, 32), crop=False, scenes=["h_one", "a_one"]))
    assert [e["scene"] for e in got] == [["h_one"], ["a_one"]]
    with pytest.raises(ValueError):
        D.RE10KScenes(root)
    with pytest.raises(KeyError):
        D.RE10KScenes(root, index=index, scenes=["nowhere"])


def test_frames_smaller_than_the_image_shape_are_skipped(tree, capsys):
    root, index = tree
    names = [e["scene"][0] for e in D.RE10KScenes(root, index=index, image_shape=(56, 56), crop=False)]
    assert names == ["a_one", "d_close", "h_one"] and "c_two" in capsys.readouterr().out        # c_two's frames are 48 x 64


def test_jpeg_frames_go_through_pillow(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from io import BytesIO
    index = F.build(tmp_path, jpeg_scenes=("a_one",))
    first = next(iter(D.RE10KScenes(tmp_path, index=index, image_shape=(32, 32), crop=False)))
    chunk = torch.load(tmp_path / "test" / "000000.torch", weights_only=True)
    data = [chunk[0]["images"][i].numpy().tobytes() for i in (1, 2, 3)]
    assert data[0][:2] == b"\xff\xd8" and first["scene"] == ["a_one"]
    want = np.stack([np.asarray(Image.open(BytesIO(d)).convert("RGB")) for d in data])
    assert np.array_equal(first["target"]["image"][0].numpy(), want)
    assert not np.array_equal(want[0], want[1]) and want.shape == (3, 64, 64, 3)                # frames 1, 2, 3 in that order, not one thrice
    assert np.array_equal(D.decode_image(data[0]), want[0])
