"""Real scenes in: the RE10K chunk reader and the crop shim, the counterpart of `src/dataset/dataset_re10k.py`, `src/dataset/shims/crop_shim.py`
and the `evaluation` view sampler (`src/dataset/view_sampler/view_sampler_evaluation.py`) for the generation harness.

    scenes = RE10KScenes("re10k", stage="test", index=load_index("assets/evaluation_index/re10k_video.json"), image_shape=(256, 256))
    for example in scenes: ...          # the dict `generate.synthetic_example` returns, with target["image"]

The images take the reference's path bit for bit -- 8-bit decode, PIL's LANCZOS resize of the 8-bit image, centre crop, / 255 -- but the
resize, crop and division run on the device (`ops.crop_shim`, csrc/cropshim.hip).  The container decode (JPEG through Pillow, PNG
through `image_io`) runs on the host by default; with `device_decode=True` a JPEG frame's Huffman scan is decoded by the library's own
host code and everything after it -- dequantisation, inverse DCT, upsampling, colour -- on the device (`ops.jpeg_decode`, csrc/jpeg.hip),
bit for bit with Pillow, so no decoded frame exists on the host; with `device_entropy=True` the Huffman scan is decoded on the device
too (csrc/jpeg_huff.hip).  Cameras follow the reference's host arithmetic.  `rescale_and_crop`, `apply_crop_shim_to_views`
and `apply_crop_shim` are drop-ins for a loader that already produces the reference's `BatchedExample` dicts.

Training reads the same chunks through `RE10KTrainLoader`, `DatasetRE10k.__iter__` for `stage = "train" | "val"`: shuffled chunks and
scenes, the `bounded` / `arbitrary` view samplers (`ViewSamplerBounded`, `ViewSamplerArbitrary`, `get_view_sampler`) under a
`StepTracker`, the augmentation shim's mirror, all with the reference's draws from torch's global stream in the reference's order:

    loader = RE10KTrainLoader("re10k", view_sampler=get_view_sampler("bounded", num_context_views=2, num_target_views=3,
                              min_distance_between_context_views=50, max_distance_between_context_views=180, step_tracker=tracker), augment=True)
    for batch in loader: ...            # [b, v, ...]: images fp32 on the device, cameras on the host -- what MVLDMTrainer takes

The mirror is not a flip of tensors: the flag of each example travels to the crop shim, which reads the flagged images' source rows
reversed (`ops.crop_shim(flip=)`), so a whole micro-batch of mirrored and unmirrored examples is one upload and one launch pair.
`apply_augmentation_and_crop_shim` is the drop-in for the reference's `apply_augmentation_shim` followed by `apply_crop_shim`.

Out of scope: the `all` / `random` view samplers, the random-transform shim (`random_transform_extrinsics`, off in the released config: it
needs an SO(3) sampler), the re10kv2 / CO3D / Objaverse readers, Lightning's DataModule."""
from __future__ import annotations

import json
import threading
from pathlib import Path
from typing import Dict, Iterator, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

NEAR, FAR = 0.1, 1000.0             # dataset_re10k.py:40-41
_PNG = b"\x89PNG\r\n\x1a\n"


# ------------------------------------------------------------------------------------------ the crop shim
def rescale_and_crop(images: torch.Tensor, intrinsics: torch.Tensor, shape: Tuple[int, int], flip: bool = False):
    """crop_shim.py:51-75 + `center_crop`: images `[*batch, 3, h, w]` (fp32 in [0, 1]; or decoded uint8 `[*batch, h, w, 3]`), intrinsics
    `[*batch, 3, 3]` -> (fp32 `[*batch, 3, h_out, w_out]` on the device, intrinsics with fx, fy rescaled).  A CPU tensor is moved to the
    current device; the intrinsics stay where they are and are changed on a clone.  `flip`: the shim reads every image mirrored."""
    from . import ops
    dev = images.device if images.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if images.dtype == torch.uint8:
        *batch, h, w, c = images.shape
        flat = images.reshape(-1, h, w, c)
    else:
        *batch, c, h, w = images.shape
        flat = images.reshape(-1, c, h, w).float()
    assert c == 3, f"the crop shim takes RGB images, got {c} channels"
    flags = torch.full((flat.shape[0],), int(flip), dtype=torch.uint8, device=dev) if flip else None
    out, scaled = ops.crop_shim(flat.to(dev).contiguous(), shape, flip=flags)
    return out.reshape(*batch, 3, *out.shape[-2:]), crop_intrinsics(intrinsics, scaled, shape)


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
class _RE10KReader:
    """what `RE10KScenes` and `RE10KTrainLoader` share: which chunks are read (`root/*.torch` sorted, or those `root/index.json` names
    for `scenes`), how their frames are decoded, and the per-scene steps of `DatasetRE10k.__iter__`.  Nothing here draws a random number."""

    def __init__(self, root, scenes, image_shape, make_baseline_1, baseline_epsilon, max_fov, crop, device_decode, device_entropy, device_restarts=False):
        self.root = Path(root)
        self.scenes = None if scenes is None else list(scenes)
        self.image_shape = (int(image_shape[0]), int(image_shape[1]))
        self.make_baseline_1, self.baseline_epsilon, self.max_fov = bool(make_baseline_1), float(baseline_epsilon), float(max_fov)
        self.crop = bool(crop)
        self.device_restarts = bool(device_restarts) and self.crop         # implies device_entropy: frames with restart intervals too
        self.device_entropy = (bool(device_entropy) or self.device_restarts) and self.crop     # implies device_decode: the Huffman scan is decoded on the device too
        self.device_decode = (bool(device_decode) or self.device_entropy) and self.crop
        self.entropy = "device" if self.device_entropy else "host"         # `ops.jpeg_decode`'s modes
        self.restarts = "device" if self.device_restarts else "host"
        if self.scenes is None:
            self.chunks = sorted(p for p in self.root.iterdir() if p.suffix == ".torch")
        else:
            with open(self.root / "index.json") as f:
                where = json.load(f)
            self.chunks = [self.root / where[name] for name in self.scenes]

    def _scenes(self, chunk_path, order=iter) -> Iterator[tuple]:
        """(example, extrinsics, intrinsics) of the chunk's scenes (those of `scenes`) in `order`, without a field of view above `max_fov`"""
        chunk = torch.load(chunk_path, weights_only=True)
        for example in order(chunk if self.scenes is None else [x for x in chunk if x["key"] in self.scenes]):
            extrinsics, intrinsics = convert_poses(example["cameras"])
            if not (get_fov(intrinsics).rad2deg() > self.max_fov).any():
                yield example, extrinsics, intrinsics

    def _baseline(self, scene: str, extrinsics: torch.Tensor, context):
        """near / far's scale: 1, or with two context views (rows `context`) and `make_baseline_1` their distance, the scene's
        translations divided by it IN PLACE; None (with the message) when it is below `baseline_epsilon`"""
        context_extrinsics = extrinsics[context]
        if context_extrinsics.shape[0] != 2 or not self.make_baseline_1:
            return 1
        a, b = context_extrinsics[:, :3, 3]
        scale = (a - b).norm()
        if scale < self.baseline_epsilon:
            print(f"Skipped {scene} because of insufficient baseline {scale:.6f}")
            return None
        extrinsics[:, :3, 3] /= scale
        return scale

    def _frame_hw(self, scene: str, sizes: set):
        """(h, w) of frames whose shape tuples are `sizes`, or None (with the message): they disagree, or are smaller than `image_shape`"""
        h, w = next(iter(sizes))[:2]
        if len(sizes) != 1 or h < self.image_shape[0] or w < self.image_shape[1]:
            print(f"Skipped bad example {scene}. Frame shapes were {sorted(sizes)}.")
            return None
        return h, w


def _bound(value: float, count: int, scale) -> torch.Tensor:
    """near or far (`NEAR`, `FAR`) of `count` views over the baseline's scale"""
    return torch.full((count,), value, dtype=torch.float32) / scale


class RE10KScenes(_RE10KReader):
    """Iterable over `BatchedExample`-shaped dicts with b = 1 (the schema of `generate.synthetic_example`, plus `target["image"]`) read
    from `root/<stage>/*.torch` in sorted order: `DatasetRE10k.__iter__` (dataset_re10k.py:79-171) with the `evaluation` view sampler.

    Each chunk is a list of {"key", "cameras" [n, 18], "images": [uint8 byte tensors]}.  `index`: `load_index`'s dict or a path to the
    JSON.  `scenes=[keys]` reads only the chunks `root/<stage>/index.json` names for them (`overfit_to_scene`).  The order is the files',
    then the chunk's, then the index entries': nothing is shuffled.  Skipped, as there: a scene with a field of view above `max_fov`
    degrees, a scene absent from the index, an entry whose two context views are closer than `baseline_epsilon`; also (with a message)
    an entry whose frames disagree in size or are smaller than `image_shape` -- any size from `image_shape` up is taken, not only
    360 x 640.  With exactly two context views and `make_baseline_1` the world is rescaled so that they are 1 apart (in place on the
    scene's poses, as the reference does: a later entry of the same scene starts from the rescaled world); near / far = 0.1 / 1000 over
    that scale.  A view group's frames are decoded on the host, stacked, uploaded as uint8 and go through `ops.crop_shim` in one call;
    with `device_decode` (and `crop`) they go through `ops.jpeg_decode` instead -- the scan decoded by the library on the host, the rest
    on the device, PNG frames and frames the library refuses through `decode_image` into their slots -- and its device tensor feeds
    the crop shim: the same bytes.  `device_entropy` (implies `device_decode`): the host only removes the scan's byte stuffing and the
    Huffman decoding runs on the device as well (`ops.jpeg_decode(entropy="device")`): a twelfth of the upload, the same bytes.
    `device_restarts` (implies `device_entropy`): frames with restart intervals are decoded on the device too, interval by interval
    (`ops.jpeg_decode(entropy="device", restarts="device")`), instead of by the host's Huffman pass: the same bytes.
    `crop=False` leaves out the device: the groups then carry the decoded uint8 frames `[1, v, h, w, 3]` and the unscaled intrinsics
    (inspection, CPU tests)."""

    def __init__(self, root, stage: str = "test", index=None, image_shape: Tuple[int, int] = (256, 256), make_baseline_1: bool = True,
                 baseline_epsilon: float = 1e-3, max_fov: float = 100.0, scenes: Optional[Sequence[str]] = None, crop: bool = True,
                 device_decode: bool = False, device_entropy: bool = False, device_restarts: bool = False):
        if index is None:
            raise ValueError("RE10KScenes needs an evaluation index (load_index(path), or the path)")
        super().__init__(Path(root) / stage, scenes, image_shape, make_baseline_1, baseline_epsilon, max_fov, crop, device_decode, device_entropy, device_restarts)
        self.index = load_index(index) if isinstance(index, (str, Path)) else {k: v for k, v in index.items() if v}

    def _views(self, example: dict, indices: Sequence[int], extrinsics, intrinsics, scale) -> Optional[dict]:
        data = [_frame_bytes(example["images"][i]) for i in indices]
        frames = None if self.device_decode else [decode_image(d) for d in data]
        sizes = {(*_frame_size(d, probe=True), 3) for d in data} if frames is None else {f.shape for f in frames}
        if self._frame_hw(example["key"], sizes) is None:
            return None
        if frames is None:
            from . import ops
            images = ops.jpeg_decode(data, entropy=self.entropy, restarts=self.restarts)
        else:
            images = torch.from_numpy(np.stack(frames))
        idx = torch.tensor(list(indices), dtype=torch.int64)
        views = {"extrinsics": extrinsics[idx][None], "intrinsics": intrinsics[idx][None], "image": images[None],
                 "near": _bound(NEAR, len(indices), scale)[None], "far": _bound(FAR, len(indices), scale)[None], "index": idx[None]}
        return apply_crop_shim_to_views(views, self.image_shape) if self.crop else views

    def __iter__(self) -> Iterator[dict]:
        for chunk_path in self.chunks:
            for example, extrinsics, intrinsics in self._scenes(chunk_path):
                scene = example["key"]
                for entry in self.index.get(scene) or ():
                    scale = self._baseline(scene, extrinsics, list(entry["context"]))
                    if scale is None:
                        continue
                    sample = {"scene": [scene]}
                    for view_type in ("context", "target"):
                        sample[view_type] = self._views(example, entry[view_type], extrinsics, intrinsics, scale)
                        if sample[view_type] is None:
                            break
                    else:
                        yield sample


# ------------------------------------------------------------------------------------------ training: step tracker, view samplers
class StepTracker:
    """step_tracker.py: the trainer's global step as the view samplers' warm-up schedules read it.  A lock-guarded int: one process per
    GPU and decode threads only, so no `Manager` process and no shared-memory tensor."""

    def __init__(self, offset: int = 0):
        self.offset = int(offset)
        self._lock = threading.Lock()
        self._step = self.offset

    def set_step(self, step: int) -> None:
        with self._lock:
            self._step = int(step) + self.offset

    def get_step(self) -> int:
        with self._lock:
            return self._step


class ViewIndex(NamedTuple):
    context: torch.Tensor                   # int64 [context views]
    target: Optional[torch.Tensor] = None   # int64 [target views]


class ViewSampler:
    """view_sampler.py: `sample(scene, num_views)` -> a list of `(context, target)` index tensors, one per example the scene gives"""

    def __init__(self, stage: str = "train", is_overfitting: bool = False, cameras_are_circular: bool = False,
                 step_tracker: Optional[StepTracker] = None):
        self.stage, self.is_overfitting, self.cameras_are_circular = stage, bool(is_overfitting), bool(cameras_are_circular)
        self.step_tracker = step_tracker

    @property
    def global_step(self) -> int:
        return 0 if self.step_tracker is None else self.step_tracker.get_step()

    def sample(self, scene: str, num_views: int) -> List[ViewIndex]:
        raise NotImplementedError


class ViewSamplerBounded(ViewSampler):
    """view_sampler_bounded.py: two context views a drawn gap apart, the targets drawn without replacement from the frames between them
    (widened by `max_distance_to_context_views`).  Three draws from torch's global stream, in this order: `randint` (the gap), `randint`
    (the left context view), `multinomial` (the targets; not drawn at `stage == "test"`, which takes the whole window).  The gaps can
    warm up linearly from their `initial_*` values over `*_warm_up_steps` of the step tracker.  `ValueError`: the scene is too short
    for the smallest gap (the reader skips it); what `multinomial` raises for a window of fewer frames than targets is not caught."""

    def __init__(self, num_context_views: int = 2, num_target_views: int = 0, min_distance_between_context_views: int = 0,
                 max_distance_between_context_views: Optional[int] = None, max_distance_to_context_views: int = 0,
                 context_gap_warm_up_steps: int = 0, target_gap_warm_up_steps: int = 0, initial_min_distance_between_context_views: int = 0,
                 initial_max_distance_between_context_views: Optional[int] = None, initial_max_distance_to_context_views: int = 0, **common):
        super().__init__(**common)
        self.num_context_views, self.num_target_views = int(num_context_views), int(num_target_views)
        self.min_distance_between_context_views = int(min_distance_between_context_views)
        self.max_distance_between_context_views = max_distance_between_context_views
        self.max_distance_to_context_views = int(max_distance_to_context_views)
        self.context_gap_warm_up_steps, self.target_gap_warm_up_steps = int(context_gap_warm_up_steps), int(target_gap_warm_up_steps)
        self.initial_min_distance_between_context_views = int(initial_min_distance_between_context_views)
        self.initial_max_distance_between_context_views = initial_max_distance_between_context_views
        self.initial_max_distance_to_context_views = int(initial_max_distance_to_context_views)

    def schedule(self, initial: int, final: int, steps: int) -> int:
        fraction = self.global_step / steps
        return min(initial + int((final - initial) * fraction), final)

    def sample(self, scene: str, num_views: int) -> List[ViewIndex]:
        max_between = self.max_distance_between_context_views or num_views
        initial_max_between = self.initial_max_distance_between_context_views or num_views
        if self.stage == "test":            # always the full gap
            max_context_gap = min_context_gap = max_between
        elif self.context_gap_warm_up_steps > 0:
            max_context_gap = self.schedule(initial_max_between, max_between, self.context_gap_warm_up_steps)
            min_context_gap = self.schedule(self.initial_min_distance_between_context_views, self.min_distance_between_context_views,
                                            self.context_gap_warm_up_steps)
        else:
            max_context_gap, min_context_gap = max_between, self.min_distance_between_context_views
        if not self.cameras_are_circular:
            max_context_gap = min(num_views - 1, max_context_gap)
        if self.stage != "test" and self.target_gap_warm_up_steps > 0:
            max_target_gap = self.schedule(self.initial_max_distance_to_context_views, self.max_distance_to_context_views,
                                           self.target_gap_warm_up_steps)
        else:
            max_target_gap = self.max_distance_to_context_views
        if max_context_gap < min_context_gap:
            raise ValueError("Example does not have enough frames!")
        context_gap = torch.randint(min_context_gap, max_context_gap + 1, size=tuple()).item()
        left = torch.randint(low=0, high=num_views if self.cameras_are_circular else num_views - context_gap, size=tuple()).item()
        if self.stage == "test":
            left = left * 0
        right = left + context_gap
        if self.is_overfitting:
            left, right = 0, max_context_gap
        target = None
        if self.num_target_views > 0:
            target_left, target_right = left - max_target_gap, right + max_target_gap
            if not self.cameras_are_circular:
                target_left, target_right = max(0, target_left), min(num_views - 1, target_right)
            target = torch.arange(target_left, target_right + 1)
            if self.stage != "test":        # when testing, all of them
                picks = torch.multinomial(torch.ones_like(target, dtype=torch.float), num_samples=self.num_target_views, replacement=False)
                target = target[picks.long()]
        if self.cameras_are_circular:
            if target is not None:
                target %= num_views
            right %= num_views
        return [ViewIndex(torch.tensor((left, right)), target)]


class ViewSamplerArbitrary(ViewSampler):
    """view_sampler_arbitrary.py: context and target views drawn anywhere in the scene (`randint`, `randint`; the context draw is made
    even when `context_views` then replaces it, as there), or fixed lists"""

    def __init__(self, num_context_views: int = 2, num_target_views: int = 0, context_views: Optional[Sequence[int]] = None,
                 target_views: Optional[Sequence[int]] = None, **common):
        super().__init__(**common)
        self.num_context_views, self.num_target_views = int(num_context_views), int(num_target_views)
        self.context_views = None if context_views is None else list(context_views)
        self.target_views = None if target_views is None else list(target_views)

    def sample(self, scene: str, num_views: int) -> List[ViewIndex]:
        context = torch.randint(0, num_views, size=(self.num_context_views,))
        if self.context_views is not None:
            assert len(self.context_views) == self.num_context_views
            context = torch.tensor(self.context_views, dtype=torch.int64)
        target = None
        if self.num_target_views > 0:
            if self.target_views is None:
                target = torch.randint(0, num_views, size=(self.num_target_views,))
            else:
                assert len(self.target_views) == self.num_target_views
                target = torch.tensor(self.target_views, dtype=torch.int64)
        return [ViewIndex(context, target)]


class ViewSamplerEvaluation(ViewSampler):
    """view_sampler_evaluation.py: every entry the evaluation index holds for the scene, nothing drawn.  `index`: `load_index`'s dict
    or the JSON's path"""
    num_context_views = num_target_views = 0

    def __init__(self, index=None, index_path=None, **common):
        super().__init__(**common)
        index = index if index is not None else index_path
        if index is None:
            raise ValueError("the evaluation view sampler needs an index (load_index(path), or the path)")
        self.index = load_index(index) if isinstance(index, (str, Path)) else {k: v for k, v in index.items() if v}
        self.total_samples = sum(len(v) for v in self.index.values())

    def sample(self, scene: str, num_views: int) -> List[ViewIndex]:
        entries = self.index.get(scene)
        if not entries:
            raise ValueError(f"No indices available for scene {scene}.")
        return [ViewIndex(torch.tensor(e["context"], dtype=torch.int64), torch.tensor(e["target"], dtype=torch.int64)) for e in entries]


VIEW_SAMPLERS = {"bounded": ViewSamplerBounded, "arbitrary": ViewSamplerArbitrary, "evaluation": ViewSamplerEvaluation}


def get_view_sampler(name: str, stage: str = "train", overfit: bool = False, cameras_are_circular: bool = False,
                     step_tracker: Optional[StepTracker] = None, **cfg) -> ViewSampler:
    """view_sampler/__init__.py: the sampler of the reference's `dataset.view_sampler.name`, its cfg fields as keyword arguments"""
    if name in ("all", "random"):
        raise NotImplementedError(f"the `{name}` view sampler is not built (bounded, arbitrary and evaluation are)")
    if name not in VIEW_SAMPLERS:
        raise KeyError(f"unknown view sampler `{name}`")
    return VIEW_SAMPLERS[name](stage=stage, is_overfitting=overfit, cameras_are_circular=cameras_are_circular, step_tracker=step_tracker, **cfg)


# ------------------------------------------------------------------------------------------ training: the augmentation shim
def reflect_extrinsics(extrinsics: torch.Tensor) -> torch.Tensor:
    """augmentation_shim.py:8-13: the camera-to-world matrices `[*batch, 4, 4]` of the scene mirrored along x, diag(-1, 1, 1, 1) E
    diag(-1, 1, 1, 1)"""
    reflect = torch.eye(4, dtype=torch.float32, device=extrinsics.device)
    reflect[0, 0] = -1
    return reflect @ extrinsics @ reflect


def _crop_views_flagged(views: dict, shape: Tuple[int, int], flip: bool) -> dict:
    """`apply_crop_shim_to_views` of a view group whose images are mirrored first when `flip`: the flag goes to the device shim, the
    extrinsics are reflected here"""
    images, intrinsics = rescale_and_crop(views["image"], views["intrinsics"], shape, flip)
    extrinsics = reflect_extrinsics(views["extrinsics"]) if flip else views["extrinsics"]
    return {**views, "image": images, "extrinsics": extrinsics, "intrinsics": intrinsics}


def apply_augmentation_and_crop_shim(example: dict, shape: Tuple[int, int], generator: Optional[torch.Generator] = None) -> dict:
    """`apply_crop_shim(apply_augmentation_shim(example, generator), shape)` (augmentation_shim.py:24-36, crop_shim.py): the reference's
    coin -- `torch.rand(())`, no mirror when it is below 0.5 -- then, for a mirrored example, the extrinsics of both view groups
    reflected on the host and the images mirrored by the device shim at its source read (no flipped copy of the images is made).
    Intrinsics are untouched by the mirror, as there, and rescaled by the crop."""
    flip = not bool(torch.rand(tuple(), generator=generator) < 0.5)
    return {**example, **{view: _crop_views_flagged(example[view], shape, flip) for view in ("context", "target")
                          if view in example and example[view].get("image") is not None}}


# ------------------------------------------------------------------------------------------ training: the loader
def _frame_size(data: bytes, probe: bool = False) -> Tuple[int, int]:
    """(h, w) of an encoded frame from its header, without decoding it.  `probe`: a JPEG the library decodes is sized by its own marker
    parser (`ops.jpeg_probe`: the frame header's numbers, which are Pillow's `size`); any other goes to Pillow as before"""
    if data[:8] == _PNG:
        return int.from_bytes(data[20:24], "big"), int.from_bytes(data[16:20], "big")
    if probe:
        from .ops import jpeg_probe
        info = jpeg_probe(data)
        if info.supported:
            return info.h, info.w
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("these frames are not PNG (RE10K stores JPEG): reading them needs the Pillow package (`PIL`), which is not installed") from e
    from io import BytesIO
    w, h = Image.open(BytesIO(data)).size
    return h, w


def _shuffle(items: list) -> list:
    return [items[i] for i in torch.randperm(len(items))]


class RE10KTrainLoader(_RE10KReader):
    """`DatasetRE10k.__iter__` (dataset_re10k.py:79-171) for `stage = "train" | "val"` behind the reference's train `DataLoader`
    (data_module.py:87-100: batches of `batch_size`, `drop_last`), one pass over the chunks per `iter()`.

    `examples()` is the host-only pass.  Its draws from torch's global stream are the reference's, in its order: `randperm` over the
    CURRENT chunk order (`self.chunks` stays shuffled between epochs, as there), `randperm` over each chunk, then per scene the field
    of view skip (nothing drawn), the view sampler's draws (`ValueError`: the scene is skipped), the two-context-view baseline rescale
    or skip AFTER those draws, and -- `stage == "train"` with `augment` only -- the augmentation coin.  `stage="val"` reads
    `<root>/test` (and shuffles too); `scenes=[keys]` reads the chunks `<root>/test/index.json` names for them (`overfit_to_scene`).  It
    yields unbatched records {"scene", "flip", "context" / "target": {"extrinsics" [v, 4, 4] (rescaled, reflected when mirrored),
    "intrinsics" [v, 3, 3] (the cropped image's: host arithmetic), "near", "far" [v] over the scale, "index" [v], "frames": decoded
    uint8 [v, h, w, 3], NOT mirrored}}.  Any frame size from `image_shape` up is taken, as in `RE10KScenes`; an example whose frames
    disagree in size or are smaller is skipped with a message before the coin (the reference's shape check sits there).

    Iterating the loader collates `batch_size` records into one `BatchedExample`-shaped dict: every field `[b, v, ...]`, `scene` a list
    of b, images fp32 `[b, v, 3, h_out, w_out]` on the device, cameras on the host -- what `MVLDMTrainer.training_step` /
    `training_window` take.  All b x (v_c + v_t) frames of one frame size go up in ONE pinned upload and through ONE `ops.crop_shim`
    call with the examples' mirror flags, and are then split into context / target; a batch that mixes frame sizes makes one call per
    size.  `decode_workers` > 0: the container decode of a batch's frames runs on that many threads (at most 16, results in order;
    nothing is drawn there, so the order of the draws does not depend on it).  `crop=False` leaves out the device: images are the
    decoded uint8 frames `[b, v, h, w, 3]` (one frame size per batch) and `flip` `[b]` says which the shim would mirror.
    `device_decode` (with `crop`): the batch's encoded frames go to `ops.jpeg_decode` -- the Huffman scans decoded by the library's host
    code on the `decode_workers` threads (no GIL) into one pinned tensor of coefficients, the inverse DCT, upsampling and colour on the
    device -- and its uint8 device tensor feeds the crop shim, so no decoded frame exists on the host; PNG frames and JPEG frames the
    library refuses are decoded as before and uploaded into their slots, so a batch may mix them.  The bytes, and the draws, are the same.
    `device_entropy` (implies `device_decode`): the workers only parse the markers and remove the byte stuffing; the Huffman scans are
    decoded on the device too (`ops.jpeg_decode(entropy="device")`), at the price of one small status read-back per frame size.
    `device_restarts` (implies `device_entropy`): so are the scans of frames with restart intervals (`restarts="device"`), which
    `device_entropy` alone leaves to the host's Huffman pass.

    No rank sharding: like the reference's iterable dataset, every rank walks all chunks, under its own torch seed."""

    MAX_DECODE_WORKERS = 16

    def __init__(self, root, stage: str = "train", view_sampler: Optional[ViewSampler] = None, image_shape: Tuple[int, int] = (256, 256),
                 batch_size: int = 6, drop_last: bool = True, augment: bool = False, make_baseline_1: bool = True, baseline_epsilon: float = 1e-3,
                 max_fov: float = 100.0, scenes: Optional[Sequence[str]] = None, decode_workers: int = 0, crop: bool = True,
                 random_transform_extrinsics: bool = False, device_decode: bool = False, device_entropy: bool = False, device_restarts: bool = False):
        if stage not in ("train", "val"):
            raise ValueError(f"RE10KTrainLoader reads stage train or val, got {stage!r} (RE10KScenes reads test)")
        if random_transform_extrinsics:
            raise NotImplementedError("dataset.random_transform_extrinsics (off in the released config) needs an SO(3) sampler that is not built")
        if view_sampler is None:            # config/experiment/baseline.yaml:16-20
            view_sampler = ViewSamplerBounded(num_context_views=2, num_target_views=3, min_distance_between_context_views=50,
                                              max_distance_between_context_views=180, stage=stage)
        super().__init__(Path(root) / ("test" if stage == "val" or scenes is not None else stage),     # `data_stage`
                         scenes, image_shape, make_baseline_1, baseline_epsilon, max_fov, crop, device_decode, device_entropy, device_restarts)
        self.stage, self.view_sampler = stage, view_sampler
        self.batch_size, self.drop_last, self.augment = int(batch_size), bool(drop_last), bool(augment)
        self.decode_workers = max(0, min(int(decode_workers), self.MAX_DECODE_WORKERS))
        self._pool = None

    # ---- the host-only pass
    def _records(self, decode: bool) -> Iterator[dict]:
        from .ops import crop_geometry
        self.chunks = _shuffle(self.chunks)
        for chunk_path in self.chunks:
            for example, extrinsics, intrinsics in self._scenes(chunk_path, _shuffle):
                scene = example["key"]
                try:
                    view_indices = self.view_sampler.sample(scene, extrinsics.shape[0])
                except ValueError:          # not enough frames
                    continue
                for view_index in view_indices:
                    scale = self._baseline(scene, extrinsics, view_index.context)
                    if scale is None:
                        continue
                    groups = {k: v for k, v in view_index._asdict().items() if v is not None}
                    data = {k: [_frame_bytes(example["images"][i.item()]) for i in v] for k, v in groups.items()}
                    size = self._frame_hw(scene, {_frame_size(d, probe=self.device_decode and not decode) for ds in data.values() for d in ds})
                    if size is None:
                        continue
                    h, w = size
                    flip = False
                    if self.stage == "train" and self.augment:
                        flip = not bool(torch.rand(tuple()) < 0.5)
                    h_s, w_s, _, _ = crop_geometry(h, w, self.image_shape)
                    record = {"scene": scene, "flip": flip}
                    for k, idx in groups.items():
                        ext = extrinsics[idx]
                        record[k] = {"extrinsics": reflect_extrinsics(ext) if flip else ext,
                                     "intrinsics": crop_intrinsics(intrinsics[idx], (h_s, w_s), self.image_shape),
                                     "near": _bound(NEAR, len(idx), scale), "far": _bound(FAR, len(idx), scale), "index": idx, "size": (h, w)}
                        if decode:
                            record[k]["frames"] = np.stack([decode_image(d) for d in data[k]])
                        else:
                            record[k]["data"] = data[k]
                    yield record


    def examples(self) -> Iterator[dict]:
        return self._records(decode=True)

    # ---- batches
    def _workers(self):
        if self.decode_workers == 0:
            return None
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=self.decode_workers, thread_name_prefix="re10k-decode")
        return self._pool

    def _decode(self, blobs: List[bytes]) -> List[np.ndarray]:
        if self.decode_workers == 0 or len(blobs) < 2:
            return [decode_image(d) for d in blobs]
        return list(self._workers().map(decode_image, blobs))     # in the order of `blobs`

    def _collate(self, records: List[dict]) -> dict:
        views = [k for k in ("context", "target") if k in records[0]]
        counts = [records[0][k]["index"].shape[0] for k in views]
        assert all([r[k]["index"].shape[0] for k in views] == counts for r in records), "one view count per batch (the sampler's)"
        v = sum(counts)
        blobs = [d for r in records for k in views for d in r[k]["data"]]
        frames = None if self.device_decode else self._decode(blobs)
        batch = {"scene": [r["scene"] for r in records]}
        by_size: Dict[Tuple[int, int], List[int]] = {}
        for i, r in enumerate(records):
            by_size.setdefault(r[views[0]]["size"], []).append(i)
        flips = torch.tensor([r["flip"] for r in records], dtype=torch.uint8)
        images = None
        if not self.crop:
            assert len(by_size) == 1, "crop=False batches hold one frame size"
            images = torch.from_numpy(np.stack(frames)).reshape(len(records), v, *frames[0].shape)
            batch["flip"] = flips.bool()
        else:
            from . import ops
            dev = torch.device("cuda", torch.cuda.current_device())
            for (h, w), members in by_size.items():
                if self.device_decode:      # coefficients up, frames decoded on the device
                    source = ops.jpeg_decode([blobs[i * v + t] for i in members for t in range(v)], pool=self._workers(), entropy=self.entropy, restarts=self.restarts)
                else:
                    staged = torch.empty(len(members) * v, h, w, 3, dtype=torch.uint8, pin_memory=True)      # one upload per frame size
                    host = staged.numpy()
                    for j, i in enumerate(members):
                        for t in range(v):
                            host[j * v + t] = frames[i * v + t]
                    source = staged.to(dev, non_blocking=True)
                flags = flips[members].repeat_interleave(v).to(dev, non_blocking=True)
                out, _ = ops.crop_shim(source, self.image_shape, flip=flags)
                out = out.reshape(len(members), v, *out.shape[1:])
                if len(by_size) == 1:
                    images = out
                else:
                    if images is None:
                        images = torch.empty(len(records), *out.shape[1:], dtype=out.dtype, device=dev)
                    images[torch.tensor(members, device=dev)] = out
        at = 0
        for k, n in zip(views, counts):
            batch[k] = {name: torch.stack([r[k][name] for r in records]) for name in ("extrinsics", "intrinsics", "near", "far", "index")}
            batch[k]["image"] = images[:, at:at + n]
            at += n
        return batch

    def __iter__(self) -> Iterator[dict]:
        pending: List[dict] = []
        for record in self._records(decode=False):
            pending.append(record)
            if len(pending) == self.batch_size:
                yield self._collate(pending)
                pending = []
        if pending and not self.drop_last:
            yield self._collate(pending)
