"""Clean-FID and Clean-KID on the device: the counterparts of `cleanfid.fid.compute_fid(dir, "gt_images")` and
`cleanfid.fid.compute_kid(dir, "gt_images")` as src/scripts/compute_fid.py:44-47 calls them (`mode="clean"`, `model_name="inception_v3"`):
the `fidclean_*` and `kidclean_*` columns of the reference's evaluation.

    python -m mv_ldm_amd.cleanfid DIR1 DIR2 --weights INCEPTION.pth [--json OUT] [--kid [--kid-seed N] [--kid-subsets S] [--kid-subset-size M]]

Every `*.png` under a folder (recursively, sorted; any PNG Pillow reads -- filtered rows, RGB, RGBA, grey, palette: `ops.png_decode`
unfilters and expands on the device, and what it refuses is decoded by Pillow) goes through the package's "clean" resize -- PIL's antialiased bicubic on float32
planes, no re-quantisation --, `(x - 128) / 128`, the FID variant of Inception-v3 up to its 2048-wide pool, and the fp64 statistics; the
score is the Frechet distance of the two sets.  The resize, the pools, the unfold that turns the 1 x 7 / 7 x 1 / 1 x 3 / 3 x 1 / 5 x 5
convolutions into 1 x 1 ones, the running statistics and the 2048-wide eigen-solves are `csrc/inception.hip`; the 94 convolutions run
through the implicit GEMM (`ops.conv2d`) with BatchNorm folded into weight and bias.  No PyTorch math and no PIL on this path.

No pretrained file ships with this package and none is fetched: `load_weights` takes the user's file (torch-fidelity / pytorch-fid
`pt_inception` key names).  The resize is pinned against PIL's own output (tests/golden/cleanfid_resize.npz); everything behind it is a
restatement of the package's arithmetic ("parity unpinned").  `sum sqrt(eig(Sigma1 Sigma2))` is computed in its symmetric
form, as `csrc/fid.hip` does; the package takes `scipy.linalg.sqrtm` and its real part.

Float images: the package's input is uint8.  A float image in [0, 1] is multiplied by 255 in fp32 and NOT quantised; the command line
always passes the decoded bytes.

KID is the package's `kernel_distance(feats1, feats2, num_subsets=100, max_subset_size=1000)` on the same features: per subset m =
min(n1, n2, max_subset_size) rows a side, the cubic kernel `(x . y / d + 1)^3`, the unbiased estimate, averaged (`csrc/kid.hip`: the Gram
tiles on the fp64 matrix cores, never an m x m matrix in memory).  Two differences to the package, both on purpose: its features are
float32 and its products run in float32, here the features are the fp64 ones and everything is fp64; and it draws the subsets from
numpy's global legacy stream, which the reference never seeds (it seeds torch only), so its own `kidclean` changes from run to run --
here the subsets are an explicit input (`kid_subsets`, in the package's draw order: `np.random.seed(s)` before a `seed=None` call selects
the subsets the package would draw), as noise is everywhere else at this boundary.
"""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import ops
from ._metric_nets import FLOATS, FrechetStats, InceptionStack, check_images, conv, pack_conv      # noqa: F401  (`conv`, `pack_conv`: importable from here)

SIZE = 299                      # the extractor's input edge
FEATURES = 2048
MAPS = ("stem", "Mixed_5d", "Mixed_6a", "Mixed_6e", "Mixed_7a", "Mixed_7c")      # what `features(return_maps=...)` can hand back


def _layers():
    """[(name, c_in, c_out, (kh, kw), stride, (pad_h, pad_w))] of the 94 BasicConv2d of the FID Inception-v3, in forward order"""
    out = []

    def add(name, c_in, c_out, k=(1, 1), stride=1, pad=(0, 0)):
        out.append((name, c_in, c_out, k, stride, pad))

    add("Conv2d_1a_3x3", 3, 32, (3, 3), 2)
    add("Conv2d_2a_3x3", 32, 32, (3, 3))
    add("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1))
    add("Conv2d_3b_1x1", 64, 80)
    add("Conv2d_4a_3x3", 80, 192, (3, 3))
    for name, c_in, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        add(f"{name}.branch1x1", c_in, 64)
        add(f"{name}.branch5x5_1", c_in, 48)
        add(f"{name}.branch5x5_2", 48, 64, (5, 5), 1, (2, 2))
        add(f"{name}.branch3x3dbl_1", c_in, 64)
        add(f"{name}.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1))
        add(f"{name}.branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1))
        add(f"{name}.branch_pool", c_in, pf)
    add("Mixed_6a.branch3x3", 288, 384, (3, 3), 2)
    add("Mixed_6a.branch3x3dbl_1", 288, 64)
    add("Mixed_6a.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1))
    add("Mixed_6a.branch3x3dbl_3", 96, 96, (3, 3), 2)
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        add(f"{name}.branch1x1", 768, 192)
        add(f"{name}.branch7x7_1", 768, c7)
        add(f"{name}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        add(f"{name}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        add(f"{name}.branch7x7dbl_1", 768, c7)
        add(f"{name}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        add(f"{name}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        add(f"{name}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        add(f"{name}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        add(f"{name}.branch_pool", 768, 192)
    add("Mixed_7a.branch3x3_1", 768, 192)
    add("Mixed_7a.branch3x3_2", 192, 320, (3, 3), 2)
    add("Mixed_7a.branch7x7x3_1", 768, 192)
    add("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    add("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    add("Mixed_7a.branch7x7x3_4", 192, 192, (3, 3), 2)
    for name, c_in in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        add(f"{name}.branch1x1", c_in, 320)
        add(f"{name}.branch3x3_1", c_in, 384)
        add(f"{name}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        add(f"{name}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        add(f"{name}.branch3x3dbl_1", c_in, 448)
        add(f"{name}.branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1))
        add(f"{name}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        add(f"{name}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        add(f"{name}.branch_pool", c_in, 192)
    return out


LAYERS = _layers()
# elements per image of the largest operand of a launch: the 5 x 5 window of a 35 x 35 x 48 map, unfolded
_LARGEST = 35 * 35 * 25 * 48


class InceptionPool3(InceptionStack):
    """The FID Inception-v3 up to its 2048-wide pool; fp32 parameters under torch-fidelity's `pt_inception` key names
    (`Mixed_6b.branch7x7_2.conv.weight`, `.bn.{weight,bias,running_mean,running_var}`).  `dtype`: the compute dtype of the activations and
    packed weights (float32 by default: a metric; float16 / bfloat16 are allowed)."""
    LAYERS = LAYERS
    IGNORED = ("AuxLogits.", "fc.")

    def __init__(self, weights=None, dtype: torch.dtype = torch.float32, allow_random_init: bool = False):
        super().__init__(dtype)
        self._init_weights(weights, allow_random_init)

    # ---- the network -----------------------------------------------------------------------------------------------------------
    @staticmethod
    def chunk_images(dtype: torch.dtype, h: int = SIZE, w: int = SIZE) -> int:
        """images per launch: the largest operand (the unfolded 5 x 5 window of a 35 x 35 x 48 map, or the resize's intermediate
        `[n, 3, h, 299]` float32) stays below 2 GiB"""
        per_image = max(_LARGEST * (4 if dtype == torch.float32 else 2), 3 * h * SIZE * 4, 3 * h * w * 4)
        return max(1, ((1 << 31) - 1) // per_image)

    def workspace_bytes(self, n: int, h: int = SIZE, w: int = SIZE, dtype: Optional[torch.dtype] = None) -> int:
        """bytes `features` / `CleanFID.update` need as `ws=` for n images of h x w: the resize's intermediate, then the features"""
        m = min(n, self.chunk_images(self.compute_dtype if dtype is None else dtype, h, w))
        return ops._roundup(ops.inception_workspace_bytes(m, h, SIZE), 16) + m * FEATURES * 8

    def _forward(self, x: torch.Tensor, packs: dict, keep: dict, wanted) -> torch.Tensor:
        """the prepared NHWC input -> the post-ReLU 8 x 8 x 2048 map; every stored map is post-ReLU"""
        spec = {name: (k, stride, pad) for name, _, _, k, stride, pad in LAYERS}

        def cv(name, x, dst=None, off=0):
            k, stride, pad = spec[name]
            y = conv(x, packs[name][0], packs[name][1], k, stride, pad)
            if dst is None:
                return ops.relu_(y)
            return ops.inception_concat(y, dst, off, relu=True)

        def new(x, h, w, c):
            return torch.empty(x.shape[0], h, w, c, dtype=x.dtype, device=x.device)

        def tap(name, x):
            if name in wanted:
                keep[name] = x
            return x

        x = cv("Conv2d_1a_3x3", x)
        x = cv("Conv2d_2a_3x3", x)
        x = cv("Conv2d_2b_3x3", x)
        x = ops.inception_maxpool(x, 2, 0)
        x = cv("Conv2d_3b_1x1", x)
        x = cv("Conv2d_4a_3x3", x)
        x = tap("stem", ops.inception_maxpool(x, 2, 0))
        for name, pf in (("Mixed_5b", 32), ("Mixed_5c", 64), ("Mixed_5d", 64)):
            out = new(x, x.shape[1], x.shape[2], 224 + pf)
            cv(f"{name}.branch1x1", x, out, 0)
            cv(f"{name}.branch5x5_2", cv(f"{name}.branch5x5_1", x), out, 64)
            cv(f"{name}.branch3x3dbl_3", cv(f"{name}.branch3x3dbl_2", cv(f"{name}.branch3x3dbl_1", x)), out, 128)
            cv(f"{name}.branch_pool", ops.inception_avgpool(x), out, 224)
            x = tap(name, out)
        h, w = (x.shape[1] - 3) // 2 + 1, (x.shape[2] - 3) // 2 + 1
        out = new(x, h, w, 768)
        cv("Mixed_6a.branch3x3", x, out, 0)
        cv("Mixed_6a.branch3x3dbl_3", cv("Mixed_6a.branch3x3dbl_2", cv("Mixed_6a.branch3x3dbl_1", x)), out, 384)
        ops.inception_maxpool(x, 2, 0, out, 480)
        x = tap("Mixed_6a", out)
        for name in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            out = new(x, x.shape[1], x.shape[2], 768)
            cv(f"{name}.branch1x1", x, out, 0)
            cv(f"{name}.branch7x7_3", cv(f"{name}.branch7x7_2", cv(f"{name}.branch7x7_1", x)), out, 192)
            y = cv(f"{name}.branch7x7dbl_1", x)
            for j in (2, 3, 4):
                y = cv(f"{name}.branch7x7dbl_{j}", y)
            cv(f"{name}.branch7x7dbl_5", y, out, 384)
            cv(f"{name}.branch_pool", ops.inception_avgpool(x), out, 576)
            x = tap(name, out)
        h, w = (x.shape[1] - 3) // 2 + 1, (x.shape[2] - 3) // 2 + 1
        out = new(x, h, w, 1280)
        cv("Mixed_7a.branch3x3_2", cv("Mixed_7a.branch3x3_1", x), out, 0)
        y = cv("Mixed_7a.branch7x7x3_1", x)
        y = cv("Mixed_7a.branch7x7x3_3", cv("Mixed_7a.branch7x7x3_2", y))
        cv("Mixed_7a.branch7x7x3_4", y, out, 320)
        ops.inception_maxpool(x, 2, 0, out, 512)
        x = tap("Mixed_7a", out)
        for name in ("Mixed_7b", "Mixed_7c"):
            out = new(x, x.shape[1], x.shape[2], 2048)
            cv(f"{name}.branch1x1", x, out, 0)
            y = cv(f"{name}.branch3x3_1", x)
            cv(f"{name}.branch3x3_2a", y, out, 320)
            cv(f"{name}.branch3x3_2b", y, out, 704)
            y = cv(f"{name}.branch3x3dbl_2", cv(f"{name}.branch3x3dbl_1", x))
            cv(f"{name}.branch3x3dbl_3a", y, out, 1088)
            cv(f"{name}.branch3x3dbl_3b", y, out, 1472)
            pooled = ops.inception_avgpool(x) if name == "Mixed_7b" else ops.inception_maxpool(x, 1, 1)
            cv(f"{name}.branch_pool", pooled, out, 1856)
            x = tap(name, out)
        return x

    def _run(self, imgs: torch.Tensor, out: Optional[torch.Tensor], state: Optional[torch.Tensor], dtype, ws, wanted=()):
        imgs = check_images("InceptionPool3", "imgs", imgs, self.Conv2d_1a_3x3.conv.weight.device, (torch.uint8, *FLOATS),
                            "uint8 images, or float images in [0, 1], are scored")
        bad = [m for m in wanted if m not in MAPS]
        if bad:
            raise ValueError(f"InceptionPool3: return_maps {bad}; known: {MAPS}")
        dtype = self.compute_dtype if dtype is None else dtype
        n, _, h, w = imgs.shape
        maps = {m: [] for m in wanted}
        if n == 0:
            return maps
        step = min(n, self.chunk_images(dtype, h, w))
        need = self.workspace_bytes(step, h, w, dtype)
        if ws is None:
            ws = ops.workspace(need, imgs.device, "cleanfid")
        if ws.numel() * ws.element_size() < need:
            raise ValueError(f"InceptionPool3: workspace of {ws.numel() * ws.element_size()} bytes, need {need}")
        prep_bytes = ops._roundup(ops.inception_workspace_bytes(step, h, SIZE), 16)
        ws = ws.view(torch.uint8).view(-1)
        packs = self._packed(dtype)
        for i0 in range(0, n, step):
            m = min(step, n - i0)
            x = ops.inception_prep(imgs[i0:i0 + m], dtype, SIZE, SIZE, ws[:prep_bytes])
            keep: dict = {}
            x = self._forward(x, packs, keep, wanted)
            f = ws[prep_bytes:prep_bytes + m * FEATURES * 8].view(torch.float64).view(m, FEATURES) if out is None else out[i0:i0 + m]
            ops.inception_features(x, f)
            if state is not None:
                ops.frechet_accumulate(f, state)
            for k, v in keep.items():
                maps[k].append(v)
        return maps

    @torch.no_grad()
    def features(self, imgs: torch.Tensor, *, dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
                 ws: Optional[torch.Tensor] = None, return_maps=()):
        """uint8 `[n, 3, h, w]`, or float in [0, 1] -> the fp64 `[n, 2048]` features on the device.  `return_maps`: names out of `MAPS`;
        then `(features, {name: post-ReLU NHWC map})` is returned."""
        n = imgs.shape[0]
        out = torch.empty(n, FEATURES, dtype=torch.float64, device=imgs.device) if out is None else out
        assert out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (n, FEATURES)
        maps = self._run(imgs, out, None, dtype, ws, tuple(return_maps))
        if not return_maps:
            return out
        return out, {k: (v[0] if len(v) == 1 else torch.cat(v)) for k, v in maps.items()}

    def forward(self, *args, **kw):
        raise NotImplementedError("InceptionPool3: call features(imgs)")


class CleanFID(FrechetStats):
    """`update(imgs, real)`, `compute()`, `reset()` around an `InceptionPool3`.  The two running states (count, sum f, sum f^T f; fp64,
    1 + 2048 + 2048^2 doubles each) live on the device; the sample counts are kept on the host too, so `compute()` can refuse without
    a synchronisation.  `compute(out=, ws=)`: `ws` is `ops.frechet_compute`'s workspace."""

    def __init__(self, model: InceptionPool3, keep_features: bool = False):
        super().__init__()
        self.model = model
        self.keep_features = bool(keep_features)
        self._feats = {True: [], False: []}
        self._init_stats(FEATURES, model.Conv2d_1a_3x3.conv.weight.device)

    @torch.no_grad()
    def update(self, imgs: torch.Tensor, real: bool, *, dtype: Optional[torch.dtype] = None, ws: Optional[torch.Tensor] = None) -> None:
        """adds `[n, 3, h, w]` images to the real or the fake side.  `ws` (uint8, at least `model.workspace_bytes(n, h, w)`) lets a captured
        graph own its buffer."""
        if imgs.is_cuda and self.real_state.device != imgs.device:
            raise RuntimeError(f"CleanFID: the states are on {self.real_state.device}, the images on {imgs.device} (no CPU fallback: module.to('cuda'))")
        state = self.real_state if real else self.fake_state
        if self.keep_features and imgs.dim() == 4 and imgs.shape[0] > 0:
            f = torch.empty(imgs.shape[0], FEATURES, dtype=torch.float64, device=imgs.device)
            self.model._run(imgs, f, state, dtype, ws)
            self._feats[bool(real)].append(f)
        else:
            self.model._run(imgs, None, state, dtype, ws)
        self._n[bool(real)] += int(imgs.shape[0])

    def _solve(self, out: torch.Tensor, ws: Optional[torch.Tensor] = None) -> None:
        ops.frechet_compute(self.real_state, self.fake_state, out, self.info, ws)

    def features(self, real: bool) -> torch.Tensor:
        """the kept fp64 `[n, 2048]` features of one side, in the order of the `update` calls (`keep_features=True` only)"""
        if not self.keep_features:
            raise RuntimeError("CleanFID: the features are folded into the moments and dropped; construct with keep_features=True")
        kept = self._feats[bool(real)]
        if not kept:
            return torch.empty(0, FEATURES, dtype=torch.float64, device=self.real_state.device)
        return kept[0] if len(kept) == 1 else torch.cat(kept)

    @torch.no_grad()
    def compute_kid(self, num_subsets: int = 100, max_subset_size: int = 1000, seed=None, **buffers) -> torch.Tensor:
        """the 0-d fp32 KID of the kept features, fake = `feats1`, real = `feats2` (`score_folders`' dir1 / dir2).  `buffers`: what
        `kernel_distance` takes (`subsets=`, `out=`, `info=`, `per_subset=`, `ws=`)."""
        if not self.keep_features:
            raise RuntimeError("CleanFID.compute_kid: KID needs the features themselves; construct with keep_features=True")
        return kernel_distance(self.features(False), self.features(True), num_subsets, max_subset_size, seed, **buffers)

    def reset(self) -> None:
        """both sides empty again (stream-ordered fills of the two states); the kept features are dropped"""
        super().reset()
        self._feats = {True: [], False: []}

    def forward(self, *args, **kw):
        raise NotImplementedError("CleanFID: call update(imgs, real) / compute() / reset()")


# ---- KID ------------------------------------------------------------------------------------------------------------------------------
def kid_subsets(n1: int, n2: int, num_subsets: int = 100, max_subset_size: int = 1000, seed=None):
    """host int32 `(idx1 [S, m], idx2 [S, m])`, m = min(n1, n2, max_subset_size): rows of feats1 and of feats2, drawn in the package's
    order -- per subset `choice(n2, m, replace=False)` first, then `choice(n1, m, replace=False)`.  `seed=None`: numpy's global legacy
    stream (the package's); an int: a private `np.random.RandomState(seed)`; a `RandomState` is used as given."""
    m = min(int(n1), int(n2), int(max_subset_size))
    if m < 2:
        raise ValueError(f"KID needs two images a side: subsets of min(n1 = {n1}, n2 = {n2}, max_subset_size = {max_subset_size}) = {m} "
                         "(the estimate divides by m - 1)")
    if num_subsets < 1:
        raise ValueError(f"KID: num_subsets {num_subsets}")
    rng = np.random if seed is None else seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    idx1 = np.empty((num_subsets, m), dtype=np.int32)
    idx2 = np.empty((num_subsets, m), dtype=np.int32)
    for s in range(num_subsets):
        idx2[s] = rng.choice(n2, m, replace=False)
        idx1[s] = rng.choice(n1, m, replace=False)
    return torch.from_numpy(idx1), torch.from_numpy(idx2)


@torch.no_grad()
def kernel_distance(feats1: torch.Tensor, feats2: torch.Tensor, num_subsets: int = 100, max_subset_size: int = 1000, seed=None, *,
                    subsets=None, out: Optional[torch.Tensor] = None, info: Optional[torch.Tensor] = None,
                    per_subset: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`cleanfid.fid.kernel_distance(feats1, feats2, num_subsets, max_subset_size)` of device fp64 features `[n1, d]`, `[n2, d]`: the 0-d
    fp32 score on the device.  `subsets=(idx1, idx2)` (integer `[S, m]`, rows of feats1 / feats2) replaces the draw of `kid_subsets`;
    the lists are range-checked here, on the host, before they are uploaded.  `info` (fp64 `[ops.KID_INFO]`) receives the record of
    `ops.kid_compute`, `per_subset` (fp64 `[S]`) each subset's value."""
    if not (feats1.is_cuda and feats2.is_cuda):
        raise RuntimeError("mv_ldm_amd.cleanfid.kernel_distance runs only on a HIP device (no CPU fallback): move the features to 'cuda'")
    if feats1.dim() != 2 or feats2.dim() != 2 or feats1.shape[1] != feats2.shape[1]:
        raise ValueError(f"kernel_distance: features {tuple(feats1.shape)} and {tuple(feats2.shape)}; two [n, d] matrices of one width are compared")
    if feats1.dtype != torch.float64 or feats2.dtype != torch.float64:
        raise TypeError(f"kernel_distance: features are {feats1.dtype}, {feats2.dtype}; the fp64 features of InceptionPool3.features are scored")
    n1, n2 = int(feats1.shape[0]), int(feats2.shape[0])
    if subsets is None:
        idx1, idx2 = kid_subsets(n1, n2, num_subsets, max_subset_size, seed)
    else:
        idx1, idx2 = (t.cpu() if isinstance(t, torch.Tensor) else torch.tensor(np.asarray(t)) for t in subsets)
        if idx1.dim() != 2 or idx1.shape != idx2.shape or idx1.shape[0] < 1 or idx1.dtype.is_floating_point or idx2.dtype.is_floating_point:
            raise ValueError(f"kernel_distance: subsets of shapes {tuple(idx1.shape)}, {tuple(idx2.shape)}; two integer [S, m] lists are taken")
        if idx1.shape[1] < 2:
            raise ValueError(f"KID needs two images a side: subsets of {idx1.shape[1]}")
        if idx1.shape[1] > min(n1, n2):
            raise ValueError(f"kernel_distance: subsets of {idx1.shape[1]} rows out of {n1} and {n2} features")
        for name, t, n in (("idx1", idx1, n1), ("idx2", idx2, n2)):
            if int(t.min()) < 0 or int(t.max()) >= n:
                raise IndexError(f"kernel_distance: {name} holds a row outside [0, {n})")
        idx1, idx2 = idx1.to(torch.int32).contiguous(), idx2.to(torch.int32).contiguous()
    dev = feats1.device
    out = torch.empty((), dtype=torch.float32, device=dev) if out is None else out
    info = torch.empty(ops.KID_INFO, dtype=torch.float64, device=dev) if info is None else info
    ops.kid_compute(feats1.contiguous(), feats2.contiguous(), idx1.to(dev), idx2.to(dev), out, info, per_subset, ws)
    return out.view(())


# ---- folders ------------------------------------------------------------------------------------------------------------------------
def list_images(folder) -> list:
    """every `*.png` under `folder`, recursively, in sorted order (the package's `sorted(glob(..., recursive=True))`)"""
    folder = Path(folder)
    if not folder.is_dir():
        raise FileNotFoundError(f"cleanfid: {folder} is not a folder")
    return sorted(p for p in folder.rglob("*.png") if p.is_file())


def iter_batches(folder, batch: int = 32, device="cpu", pool=None, inflate: str = "host"):
    """uint8 `[m, 3, h, w]` tensors on `device` (the host unless one is named) of the folder's images: sorted order, split by image size (sizes in order of first
    appearance), at most `batch` images each.  Any PNG Pillow reads: the host inflates (on `pool`), the device unfilters the rows and
    expands grey, alpha and palette files to RGB (`ops.png_decode`); what that refuses goes through Pillow.  `inflate="device"`: the
    device inflates too (opt-in, the same bytes)."""
    from .image_io import group_by_size, load_images
    paths = list_images(folder)
    for members in group_by_size(paths).values():
        for i in range(0, len(members), batch):
            yield load_images([paths[j] for j in members[i:i + batch]], device, pool, out="uint8", inflate=inflate).permute(0, 3, 1, 2).contiguous()


def score_folders(dir1, dir2, metric: CleanFID, batch: int = 32, dtype: Optional[torch.dtype] = None, kid: Optional[dict] = None, inflate: str = "host") -> dict:
    """{"fidclean", "n1", "n2", "solve": {...}} of two folders, which need not pair up: a distance of two distributions.
    `kid=dict(num_subsets=, max_subset_size=, seed=)` (a `CleanFID(keep_features=True)`) adds "kidclean" and "kid": {"m", "subsets",
    "seed", "fp64", "scale"}.  `inflate`: see `iter_batches`."""
    if kid is not None and not metric.keep_features:
        raise RuntimeError("score_folders(kid=...): KID needs the features themselves; construct the CleanFID with keep_features=True")
    from concurrent.futures import ThreadPoolExecutor
    dev = metric.real_state.device
    metric.reset()
    counts = []
    pool = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))      # the files' inflate; unfiltering and expansion are the device's
    try:
        for folder, real in ((dir1, False), (dir2, True)):
            n = 0
            for imgs in iter_batches(folder, batch, dev, pool, inflate):
                metric.update(imgs, real=real, dtype=dtype)
                n += imgs.shape[0]
            if n == 0:
                raise ValueError(f"cleanfid: no *.png under {folder}")
            counts.append(n)
    finally:
        pool.shutdown()
    score = float(metric.compute())
    info = metric.info.tolist()
    rec = {"fidclean": score, "n1": counts[0], "n2": counts[1],
           "solve": {"sweeps": [int(info[0]), int(info[2])], "residual": [info[1], info[3]], "capped": int(info[4]), "fid_fp64": info[5],
                     "sum_sqrt": info[6], "scale": info[7]}}
    if kid is not None:
        kinfo = torch.empty(ops.KID_INFO, dtype=torch.float64, device=dev)
        num_subsets, seed = int(kid.get("num_subsets", 100)), kid.get("seed")
        rec["kidclean"] = float(metric.compute_kid(num_subsets, int(kid.get("max_subset_size", 1000)), seed, info=kinfo))
        kinfo = kinfo.tolist()
        rec["kid"] = {"m": int(kinfo[2]), "subsets": num_subsets, "seed": seed if seed is None or isinstance(seed, int) else None,
                      "fp64": kinfo[0], "scale": kinfo[1]}
    metric.reset()
    return rec


def _not_empty(*folders) -> None:
    """refuse before any weight is read or any launch is made"""
    for folder in folders:
        if not list_images(folder):
            raise ValueError(f"cleanfid: no *.png under {folder}")


def compute_fid(dir1, dir2, weights, device="cuda", batch: int = 32, dtype: torch.dtype = torch.float32) -> float:
    """`cleanfid.fid.compute_fid(dir1, dir2)` with the Inception-v3 weights of `weights` (a path or a state dict)"""
    _not_empty(dir1, dir2)
    model = weights if isinstance(weights, InceptionPool3) else InceptionPool3(weights=weights, dtype=dtype).to(device)
    return score_folders(dir1, dir2, CleanFID(model), batch, dtype)["fidclean"]


def compute_kid(dir1, dir2, weights, device="cuda", batch: int = 32, dtype: torch.dtype = torch.float32, num_subsets: int = 100,
                max_subset_size: int = 1000, seed=None) -> float:
    """`cleanfid.fid.compute_kid(dir1, dir2)` with the Inception-v3 weights of `weights` (a path, a state dict or an `InceptionPool3`);
    `seed`: see `kid_subsets`"""
    _not_empty(dir1, dir2)
    model = weights if isinstance(weights, InceptionPool3) else InceptionPool3(weights=weights, dtype=dtype).to(device)
    kid = dict(num_subsets=num_subsets, max_subset_size=max_subset_size, seed=seed)
    return score_folders(dir1, dir2, CleanFID(model, keep_features=True), batch, dtype, kid=kid)["kidclean"]


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m mv_ldm_amd.cleanfid", description="clean-fid's compute_fid (and compute_kid) of two PNG folders on the device")
    ap.add_argument("dir1")
    ap.add_argument("dir2")
    ap.add_argument("--weights", required=True, help="pt_inception state dict (torch-fidelity / pytorch-fid key names)")
    ap.add_argument("--json", default=None, help="write the record here too")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="float32", choices=("float32", "float16", "bfloat16"))
    ap.add_argument("--kid", action="store_true", help="also score clean-fid's compute_kid (kidclean)")
    ap.add_argument("--kid-seed", type=int, default=None, help="seed of a private numpy RandomState for the subsets (default: numpy's global stream)")
    ap.add_argument("--kid-subsets", type=int, default=100)
    ap.add_argument("--kid-subset-size", type=int, default=1000)
    ap.add_argument("--device-inflate", action="store_true", help="inflate the files' IDAT on the device as well (the default inflates on the host); the same bytes")
    a = ap.parse_args(argv)
    dtype = getattr(torch, a.dtype)
    _not_empty(a.dir1, a.dir2)
    model = InceptionPool3(weights=a.weights, dtype=dtype).to("cuda")
    kid = dict(num_subsets=a.kid_subsets, max_subset_size=a.kid_subset_size, seed=a.kid_seed) if a.kid else None
    rec = score_folders(a.dir1, a.dir2, CleanFID(model, keep_features=a.kid), a.batch, dtype, kid=kid, inflate="device" if a.device_inflate else "host")
    s = rec["solve"]
    line = (f"fidclean {rec['fidclean']:.6f}  ({rec['n1']} vs {rec['n2']} images; solves: {s['sweeps'][0]} + {s['sweeps'][1]} sweeps, "
            f"residual {s['residual'][0]:.1e}, {s['residual'][1]:.1e}, capped {s['capped']})")
    if a.kid:
        line += f"  kidclean {rec['kidclean']:.6e}  ({rec['kid']['subsets']} subsets of {rec['kid']['m']}, seed {rec['kid']['seed']})"
    print(line)
    if a.json:
        Path(a.json).write_text(json.dumps(rec, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
