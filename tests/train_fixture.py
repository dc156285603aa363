"""A small RE10K-format tree for the training-loader tests (tests/test_train_loader_cpu.py, tests/test_hip_train_loader.py) and the maker
of their golden (tests/golden/make_train_loader_golden.py): `<root>/train/*.torch` chunks of {"key", "cameras" [n, 18], "images": [uint8
byte tensors]} with `<root>/train/index.json` (scene -> chunk file), and the same tree under `<root>/test` (what `stage="val"` reads).

Frames are 360 x 640 -- the reference's reader refuses any other size -- of seeded 45 x 80 noise repeated 8 x each way (a PNG of it
encodes and decodes fast), PNG-encoded by `image_io`; `jpeg=True` re-encodes every frame through Pillow.  Three chunks, six scenes;
"fx" is the focal length, "dx" the camera step along x.  Under `SAMPLER` (bounded: 2 context + 3 target views, gaps 2...4) every epoch
yields exactly s_a, s_b and s_c, in a shuffled order, and meets each skip rule of the reader once."""
import hashlib
import json
import shutil
from pathlib import Path

import numpy as np
import torch

from mv_ldm_amd.image_io import encode_png

H, W, REPEAT = 360, 640, 8
# scene -> (frames, fx = fy, dx)
SCENES = {
    "s_a": (8, 0.9, 0.1),
    "s_wide": (8, 0.3, 0.1),                # field of view 2 atan(0.5 / 0.3) = 118 degrees: skipped, nothing drawn
    "s_b": (6, 0.8, 0.2),
    "s_short": (2, 0.9, 0.1),               # the largest gap (1) is below the smallest allowed (2): ValueError before any draw
    "s_c": (7, 1.1, 0.1),
    "s_close": (8, 0.9, 1e-5),              # context views at most 4e-5 apart: skipped AFTER the sampler's three draws
}
CHUNKS = {"000000.torch": ("s_a", "s_wide"), "000001.torch": ("s_b", "s_short"), "000002.torch": ("s_c", "s_close")}
YIELDED = ("s_a", "s_b", "s_c")
SAMPLER = dict(num_context_views=2, num_target_views=3, min_distance_between_context_views=2, max_distance_between_context_views=4)
SHAPE = (32, 32)
# camera i is turned by i quarter turns about y: (cos, sin).  Every rotation entry is 0 or +-1, so the fp32 inverse `convert_poses` takes
# of the world-to-camera matrix is exact whatever the host's LAPACK does in which order, and the cameras the golden recorded on one
# machine can be compared bit for bit on another
QUARTER_TURNS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))


def frames(scene: str) -> np.ndarray:
    """uint8 [n, 360, 640, 3], seeded by the scene's name"""
    n = SCENES[scene][0]
    rng = np.random.default_rng(int.from_bytes(hashlib.sha256(scene.encode()).digest()[:4], "little"))
    small = rng.integers(0, 256, (n, H // REPEAT, W // REPEAT, 3), dtype=np.uint8)
    return np.ascontiguousarray(small.repeat(REPEAT, axis=1).repeat(REPEAT, axis=2))


def cameras(scene: str) -> torch.Tensor:
    """[n, 18]: fx, fy, cx, cy, two unused, the 3 x 4 world-to-camera matrix [R^T | -R^T t] by rows; camera i stands at (i dx, 0, 0)"""
    n, f, dx = SCENES[scene]
    c2w = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    for i in range(n):
        c, s = QUARTER_TURNS[i % 4]
        c2w[i, :3, :3] = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float64)
        c2w[i, 0, 3] = i * dx
    rt = c2w[:, :3, :3].transpose(1, 2)
    w2c = torch.cat([rt, -(rt @ c2w[:, :3, 3:])], dim=2)
    head = torch.tensor([f, f, 0.5, 0.5, 0.0, 0.0], dtype=torch.float64).repeat(n, 1)
    return torch.cat([head, w2c.reshape(n, 12)], dim=1).float()


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


def build(root: Path, jpeg: bool = False) -> Path:
    """writes `<root>/train` and the same files under `<root>/test`; returns `root`"""
    root = Path(root)
    stage = root / "train"
    stage.mkdir(parents=True)
    where = {}
    for name, scenes in CHUNKS.items():
        torch.save([{"key": s, "cameras": cameras(s), "images": [_encode(f, jpeg) for f in frames(s)]} for s in scenes], stage / name)
        where.update({s: name for s in scenes})
    (stage / "index.json").write_text(json.dumps(where))
    shutil.copytree(stage, root / "test")
    return root
