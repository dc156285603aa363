"""Real scenes in: the RE10K chunk reader and the crop shim, the counterpart of `src/dataset/dataset_re10k.py`, `src/dataset/shims/crop_shim.py`
and the `evaluation` view sampler (`src/dataset/view_sampler/view_sampler_evaluation.py`) for the generation harness.

    scenes = RE10KScenes("re10k", stage="test", index=load_index("assets/evaluation_index/re10k_video.json"), image_shape=(256, 256))
    for example in scenes: ...          # the dict `generate.synthetic_example` returns, with target["image"]

The images take the reference's path bit for bit -- 8-bit decode, PIL's LANCZOS resize of the 8-bit image, centre crop, / 255 -- but the
resize, crop and division run on the device (`ops.crop_shim`, csrc/cropshim.hip); only the container decode (JPEG through Pillow, PNG
through `image_io`) stays on the host.  Cameras follow the reference's host arithmetic.  `rescale_and_crop`, `apply_crop_shim_to_views`
and `apply_crop_shim` are drop-ins for a loader that already produces the reference's `BatchedExample` dicts.

Out of scope: the `bounded` / `arbitrary` training view samplers and the step tracker, the augmentation and random-transform shims, the
re10kv2 / CO3D / Objaverse readers, JPEG decoding on the device, Lightning's DataModule."""
from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

NEAR, FAR = 0.1, 1000.0             # dataset_re10k.py:40-41
_PNG = b"\x89PNG\r\n\x1a\n"


# ------------------------------------------------------------------------------------------ the crop shim
def rescale_and_crop(images: torch.Tensor, intrinsics: torch.Tensor, shape: Tuple[int, int]):
    """crop_shim.py:51-75 + `center_crop`: images `[*batch, 3, h, w]` (fp32 in [0, 1]; or decoded uint8 `[*batch, h, w, 3]`), intrinsics
    `[*batch, 3, 3]` -> (fp32 `[*batch, 3, h_out, w_out]` on the device, intrinsics with fx, fy rescaled).  A CPU tensor is moved to the
    current device; the intrinsics stay where they are and are changed on a clone."""
    from . import ops
    dev = images.device if images.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if images.dtype == torch.uint8:
        *batch, h, w, c = images.shape
        flat = images.reshape(-1, h, w, c)
    else:
        *batch, c, h, w = images.shape
        flat = images.reshape(-1, c, h, w).float()
    assert c == 3, f"the crop shim takes RGB images, got {c} channels"
    out, (h_scaled, w_scaled) = ops.crop_shim(flat.to(dev).contiguous(), shape)
    return out.reshape(*batch, 3, *out.shape[-2:]), crop_intrinsics(intrinsics, (h_scaled, w_scaled), shape)


def crop_intrinsics(intrinsics: torch.Tensor, scaled: Tuple[int, int], shape: Tuple[int, int]) -> torch.Tensor:
    """`center_crop`'s camera update (crop_shim.py:43-46) from the scaled size to `shape`, on a clone: normalised focal lengths grow by the
    share of the image the crop keeps"""
    intrinsics = intrinsics.clone()
    intrinsics[..., 0, 0] *= scaled[1] / shape[1]  # fx
    intrinsics[..., 1, 1] *= scaled[0] / shape[0]  # fy
    return intrinsics


def apply_crop_shim_to_views(views: dict, shape: Tuple[int, int]) -> dict:
    images, intrinsics = rescale_and_crop(views["image"], views["intrinsics"], shape)
    return {**views, "image": images, "intrinsics": intrinsics}


def apply_crop_shim(example: dict, shape: Tuple[int, int]) -> dict:
    """crop every view group of the example that carries images"""
    return {**example, **{view: apply_crop_shim_to_views(example[view], shape) for view in ("context", "target")
                          if view in example and example[view].get("image") is not None}}


# ------------------------------------------------------------------------------------------ cameras
def convert_poses(cameras: torch.Tensor):
    """dataset_re10k.py:173-194: `[n, 18]` rows (fx, fy, cx, cy, 2 unused, a 3 x 4 world-to-camera matrix by rows) -> (camera-to-world
    `[n, 4, 4]`, normalised intrinsics `[n, 3, 3]`), fp32"""
    cameras = cameras.float()
    n = cameras.shape[0]
    intrinsics = torch.eye(3, dtype=torch.float32).repeat(n, 1, 1)
    intrinsics[:, 0, 0], intrinsics[:, 1, 1] = cameras[:, 0], cameras[:, 1]
    intrinsics[:, 0, 2], intrinsics[:, 1, 2] = cameras[:, 2], cameras[:, 3]
    w2c = torch.eye(4, dtype=torch.float32).repeat(n, 1, 1)
    w2c[:, :3] = cameras[:, 6:].reshape(n, 3, 4)
    return w2c.inverse(), intrinsics


def get_fov(intrinsics: torch.Tensor) -> torch.Tensor:
    """projection.py:234-248: `[n, 3, 3]` normalised intrinsics -> `[n, 2]` horizontal and vertical field of view in radians"""
    inv = intrinsics.inverse()

    def ray(v):
        d = torch.einsum("bij,j->bi", inv, torch.tensor(v, dtype=torch.float32, device=intrinsics.device))
        return d / d.norm(dim=-1, keepdim=True)
    fov_x = (ray([0, 0.5, 1]) * ray([1, 0.5, 1])).sum(dim=-1).acos()
    fov_y = (ray([0.5, 0, 1]) * ray([0.5, 1, 1])).sum(dim=-1).acos()
    return torch.stack((fov_x, fov_y), dim=-1)


# ------------------------------------------------------------------------------------------ the evaluation index
def load_index(path: Union[str, Path]) -> Dict[str, List[dict]]:
    """the reference's evaluation index (`assets/evaluation_index/*.json`): {scene: [{"context": [...], "target": [...]}, ...]}.  Scenes
    mapped to null or to an empty list have no views to sample (`ViewSamplerEvaluation.sample` raises, the reader skips them) and are left out."""
    with open(path) as f:
        raw = json.load(f)
    return {k: [{"context": tuple(int(i) for i in e["context"]), "target": tuple(int(i) for i in e["target"])} for e in v]
            for k, v in raw.items() if v}


# ------------------------------------------------------------------------------------------ images
def decode_image(data: bytes) -> np.ndarray:
    """one encoded frame -> uint8 `[h, w, 3]`.  PNG (8-bit RGB / RGBA, as `image_io.encode_png` writes) is decoded here; anything else (the
    dataset's JPEG) goes to Pillow on the host"""
    if data[:8] == _PNG:
        from .image_io import decode_png
        return np.ascontiguousarray(decode_png(data)[..., :3])
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("these frames are not PNG (RE10K stores JPEG): decoding them needs the Pillow package (`PIL`), which is not installed") from e
    from io import BytesIO
    return np.ascontiguousarray(np.asarray(Image.open(BytesIO(data)).convert("RGB")))


def _frame_bytes(frame) -> bytes:
    return frame.numpy().tobytes() if isinstance(frame, torch.Tensor) else bytes(frame)


# ------------------------------------------------------------------------------------------ the reader
class RE10KScenes:
    """Iterable over `BatchedExample`-shaped dicts with b = 1 (the schema of `generate.synthetic_example`, plus `target["image"]`) read
    from `root/<stage>/*.torch` in sorted order: `DatasetRE10k.__iter__` (dataset_re10k.py:79-171) with the `evaluation` view sampler.

    Each chunk is a list of {"key", "cameras" [n, 18], "images": [uint8 byte tensors]}.  `index`: `load_index`'s dict or a path to the
    JSON.  `scenes=[keys]` reads only the chunks `root/<stage>/index.json` names for them (`overfit_to_scene`).  The order is the files',
    then the chunk's, then the index entries': nothing is shuffled.  Skipped, as there: a scene with a field of view above `max_fov`
    degrees, a scene absent from the index, an entry whose two context views are closer than `baseline_epsilon`; also (with a message)
    an entry whose frames disagree in size or are smaller than `image_shape` -- any size from `image_shape` up is taken, not only
    360 x 640.  With exactly two context views and `make_baseline_1` the world is rescaled so that they are 1 apart (in place on the
    scene's poses, as the reference does: a later entry of the same scene starts from the rescaled world); near / far = 0.1 / 1000 over
    that scale.  A view group's frames are decoded on the host, stacked, uploaded as uint8 and go through `ops.crop_shim` in one call.
    `crop=False` leaves out the device: the groups then carry the decoded uint8 frames `[1, v, h, w, 3]` and the unscaled intrinsics
    (inspection, CPU tests)."""

    def __init__(self, root, stage: str = "test", index=None, image_shape: Tuple[int, int] = (256, 256), make_baseline_1: bool = True,
                 baseline_epsilon: float = 1e-3, max_fov: float = 100.0, scenes: Optional[Sequence[str]] = None, crop: bool = True):
        if index is None:
            raise ValueError("RE10KScenes needs an evaluation index (load_index(path), or the path)")
        self.root = Path(root) / stage
        self.index = load_index(index) if isinstance(index, (str, Path)) else {k: v for k, v in index.items() if v}
        self.image_shape = (int(image_shape[0]), int(image_shape[1]))
        self.make_baseline_1, self.baseline_epsilon, self.max_fov = bool(make_baseline_1), float(baseline_epsilon), float(max_fov)
        self.scenes = None if scenes is None else list(scenes)
        self.crop = bool(crop)
        if self.scenes is None:
            self.chunks = sorted(p for p in self.root.iterdir() if p.suffix == ".torch")
        else:
            with open(self.root / "index.json") as f:
                where = json.load(f)
            self.chunks = [self.root / where[name] for name in self.scenes]

    def _views(self, example: dict, indices: Sequence[int], extrinsics, intrinsics, scale) -> Optional[dict]:
        frames = [decode_image(_frame_bytes(example["images"][i])) for i in indices]
        sizes = {f.shape for f in frames}
        h_out, w_out = self.image_shape
        if len(sizes) != 1 or frames[0].shape[0] < h_out or frames[0].shape[1] < w_out:
            print(f"Skipped bad example {example['key']}. Frame shapes were {sorted(sizes)}.")
            return None
        idx = torch.tensor(list(indices), dtype=torch.int64)
        bound = lambda v: (torch.full((len(indices),), v, dtype=torch.float32) / scale)[None]
        views = {"extrinsics": extrinsics[idx][None], "intrinsics": intrinsics[idx][None], "image": torch.from_numpy(np.stack(frames))[None],
                 "near": bound(NEAR), "far": bound(FAR), "index": idx[None]}
        return apply_crop_shim_to_views(views, self.image_shape) if self.crop else views

    def __iter__(self) -> Iterator[dict]:
        for chunk_path in self.chunks:
            chunk = torch.load(chunk_path, weights_only=True)
            if self.scenes is not None:
                chunk = [x for x in chunk if x["key"] in self.scenes]
            for example in chunk:
                extrinsics, intrinsics = convert_poses(example["cameras"])
                scene = example["key"]
                if (get_fov(intrinsics).rad2deg() > self.max_fov).any():
                    continue
                for entry in self.index.get(scene) or ():
                    context_extrinsics = extrinsics[list(entry["context"])]
                    if context_extrinsics.shape[0] == 2 and self.make_baseline_1:
                        a, b = context_extrinsics[:, :3, 3]
                        scale = (a - b).norm()
                        if scale < self.baseline_epsilon:
                            print(f"Skipped {scene} because of insufficient baseline {scale:.6f}")
                            continue
                        extrinsics[:, :3, 3] /= scale
                    else:
                        scale = 1
                    sample = {"scene": [scene]}
                    for view_type in ("context", "target"):
                        sample[view_type] = self._views(example, entry[view_type], extrinsics, intrinsics, scale)
                        if sample[view_type] is None:
                            break
                    else:
                        yield sample
