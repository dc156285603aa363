"""A small RE10K-format tree for the dataset tests (tests/test_dataset_cpu.py, tests/test_hip_dataset.py): `<root>/test/*.torch` chunks of
{"key", "cameras" [n, 18], "images": [uint8 byte tensors]}, `<root>/test/index.json` (scene -> chunk file) and an evaluation index
({scene: [{"context": [...], "target": [...]}]}), as `torch.save` and the reference's converter lay them out.  Frames are seeded noise,
PNG-encoded by `image_io` (the real dataset stores JPEG: `jpeg=True` re-encodes one scene through Pillow)."""
import hashlib
import json
import math
from pathlib import Path

import numpy as np
import torch

from mv_ldm_amd.image_io import encode_png

N_FRAMES = 5
# scene -> (frame h, frame w, fx = fy, positions of its cameras along x)
SCENES = {
    "a_one": (64, 64, 0.9, (0.0, 0.1, 0.2, 0.3, 0.4)),
    "b_wide": (64, 64, 0.3, (0.0, 0.1, 0.2, 0.3, 0.4)),              # field of view 2 atan(0.5 / 0.3) = 118 degrees: skipped
    "c_two": (48, 64, 0.8, (0.0, 0.5, 1.0, 1.5, 2.0)),               # two context views 2.0 apart: the world is rescaled
    "d_close": (64, 64, 0.9, (0.0, 0.0002, 0.2, 0.3, 0.4)),          # its first entry's context views are 2e-4 apart: that entry is skipped
    "e_missing": (64, 64, 0.9, (0.0, 0.1, 0.2, 0.3, 0.4)),           # not in the evaluation index: skipped
    "f_null": (64, 64, 0.9, (0.0, 0.1, 0.2, 0.3, 0.4)),              # mapped to null there: skipped
    "h_one": (64, 64, 1.1, (0.0, 0.1, 0.2, 0.3, 0.4)),
}
CHUNKS = {"000000.torch": ("a_one", "b_wide", "c_two", "d_close"), "000001.torch": ("e_missing", "f_null", "h_one")}
INDEX = {
    "a_one": [{"context": [0], "target": [1, 2, 3]}],
    "b_wide": [{"context": [0], "target": [1, 2]}],
    "c_two": [{"context": [0, 4], "target": [1, 2, 3]}],
    "d_close": [{"context": [0, 1], "target": [2, 3]}, {"context": [2], "target": [3, 4]}],
    "f_null": None,
    "h_one": [{"context": [1], "target": [0, 2, 4]}],
    "z_absent": [{"context": [0], "target": [1]}],                   # in the index, in no chunk
}
ANGLE = 0.05                                                         # camera i is turned by i ANGLE about y


def frames(scene: str, frame_hw=None) -> np.ndarray:
    """uint8 [N_FRAMES, h, w, 3], seeded by the scene's name; `frame_hw` replaces the scene's own frame size"""
    h, w = frame_hw or SCENES[scene][:2]
    rng = np.random.default_rng(int.from_bytes(hashlib.sha256(scene.encode()).digest()[:4], "little"))
    return rng.integers(0, 256, (N_FRAMES, h, w, 3), dtype=np.uint8)


def camera_to_world(scene: str) -> torch.Tensor:
    """[N_FRAMES, 4, 4] by hand: rotation by i ANGLE about y, position (x_i, 0, 0)"""
    out = torch.eye(4, dtype=torch.float64).repeat(N_FRAMES, 1, 1)
    for i, x in enumerate(SCENES[scene][3]):
        c, s = math.cos(i * ANGLE), math.sin(i * ANGLE)
        out[i, :3, :3] = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float64)
        out[i, :3, 3] = torch.tensor([x, 0.0, 0.0], dtype=torch.float64)
    return out


def cameras(scene: str) -> torch.Tensor:
    """[N_FRAMES, 18]: fx, fy, cx, cy, two unused, the 3 x 4 world-to-camera matrix [R^T | -R^T t] by rows"""
    c2w = camera_to_world(scene)
    rt = c2w[:, :3, :3].transpose(1, 2)
    w2c = torch.cat([rt, -(rt @ c2w[:, :3, 3:])], dim=2)
    f = SCENES[scene][2]
    head = torch.tensor([f, f, 0.5, 0.5, 0.0, 0.0], dtype=torch.float64).repeat(N_FRAMES, 1)
    return torch.cat([head, w2c.reshape(N_FRAMES, 12)], dim=1).float()


def _encode(pixels: np.ndarray, jpeg: bool) -> torch.Tensor:
    if jpeg:
        from io import BytesIO

        from PIL import Image
        buf = BytesIO()
        Image.fromarray(pixels).save(buf, format="JPEG", quality=90)
        data = buf.getvalue()
    else:
        data = encode_png(pixels)
    return torch.tensor(np.frombuffer(data, dtype=np.uint8).copy())


def build(root: Path, jpeg_scenes=(), frame_hw=None) -> Path:
    """writes the tree under `root`, returns the evaluation index's path"""
    stage = Path(root) / "test"
    stage.mkdir(parents=True)
    where = {}
    for name, scenes in CHUNKS.items():
        torch.save([{"key": s, "cameras": cameras(s), "images": [_encode(f, s in jpeg_scenes) for f in frames(s, frame_hw)]} for s in scenes], stage / name)
        where.update({s: name for s in scenes})
    (stage / "index.json").write_text(json.dumps(where))
    index = Path(root) / "evaluation_index.json"
    index.write_text(json.dumps(INDEX))
    return index
