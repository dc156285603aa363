"""FID on the device: the counterpart of `torchmetrics.image.fid.FrechetInceptionDistance(feature=64, normalize=True)` as
`src/evaluation/metric_computer.py:22,65-68` uses it (`update(ground_truth, real=True)`, `update(predicted, real=False)`, `compute()`,
`reset()`).

`feature=64` taps Inception-v3 after its first max-pool: three 3x3 convolutions with BatchNorm, which run through the implicit GEMM
(`ops.conv2d`) with BatchNorm folded into the packed weight and a bias.  The byte quantisation with torch-fidelity's TensorFlow-1 bilinear
resize to 299 x 299, the fused ReLU + max-pool + global average, the fp64 running statistics and the Frechet distance (two symmetric
64 x 64 eigen-solves by cyclic Jacobi, one workgroup, matrices in LDS) are `csrc/fid.hip`.

No pretrained file ships with this package and none is fetched: `load_weights` takes the user's file, torch-fidelity's `pt_inception`
state dict or a torchmetrics FID state dict.  The package's arithmetic is restated, not pinned against the package itself (DESIGN.md
§5, "parity unpinned"); `sum sqrt(eig(Sigma1 Sigma2))` is computed in its symmetric form.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from ._metric_nets import BN_EPS, FLOATS, FrechetStats, InceptionStack, check_images, conv      # noqa: F401  (BN_EPS stays importable from here)
from .cleanfid import LAYERS as INCEPTION_LAYERS

LAYERS = INCEPTION_LAYERS[:3]   # Conv2d_1a_3x3, Conv2d_2a_3x3, Conv2d_2b_3x3: rows (name, c_in, c_out, (kh, kw), stride, (pad_h, pad_w))
SIZE = 299                      # the extractor's input edge
MAP = 147                       # the edge of Conv2d_2b_3x3's output: 299 -> 149 -> 147 -> 147
FEATURES = 64


class FrechetInceptionDistance(FrechetStats, InceptionStack):
    """`FrechetInceptionDistance(feature=64, normalize=True)`; fp32 parameters under torch-fidelity's key names
    (`Conv2d_{1a,2a,2b}_3x3.conv.weight`, `.bn.{weight,bias,running_mean,running_var}`).  `normalize=True`: float images in [0, 1];
    `normalize=False`: uint8 images.  `dtype`: the compute dtype of the activations and packed weights (float32 by default: a metric;
    float16 / bfloat16 are allowed).  The two running states (count, sum f, sum f^T f; fp64) live on the device; the sample counts are
    kept on the host too, so `compute()` can refuse without a synchronisation.  `load_weights` ignores the layers of Inception-v3
    behind the tap: their keys are in every published file."""
    LAYERS = LAYERS
    IGNORED = ("Conv2d_3b_1x1.", "Conv2d_4a_3x3.", "Mixed_", "AuxLogits.", "fc.")

    def __init__(self, feature: int = 64, normalize: bool = True, weights=None, dtype: torch.dtype = torch.float32, allow_random_init: bool = False):
        if feature in (192, 768, 2048):
            raise NotImplementedError(f"FrechetInceptionDistance(feature={feature}): only feature=64, the tap the reference scores with "
                                      "(Inception-v3 after its first max-pool), is built")
        if feature != 64:
            raise ValueError(f"FrechetInceptionDistance: feature={feature!r}; torchmetrics knows 64, 192, 768, 2048 and feature=64 is built")
        super().__init__(dtype)
        self.normalize = bool(normalize)
        self._init_stats(FEATURES)
        self._init_weights(weights, allow_random_init)

    # ---- the metric ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def chunk_images(dtype: torch.dtype) -> int:
        """images per launch: the largest operand (n x 147 x 147 x 64 of the compute dtype) stays below 2 GiB"""
        return max(1, ((1 << 31) - 1) // (MAP * MAP * FEATURES * (4 if dtype == torch.float32 else 2)))

    def workspace_bytes(self, n: int, dtype: Optional[torch.dtype] = None) -> int:
        """bytes `update` / `features` need as `ws=` for n images"""
        dtype = self.compute_dtype if dtype is None else dtype
        return ops.fid_workspace_bytes(min(n, self.chunk_images(dtype)), MAP, MAP, FEATURES)

    def _check(self, imgs: torch.Tensor) -> torch.Tensor:
        if self.normalize:
            return check_images("FrechetInceptionDistance(normalize=True)", "imgs", imgs, self.real_state.device, FLOATS,
                                "float32, bfloat16 or float16 images in [0, 1] are scored")
        return check_images("FrechetInceptionDistance(normalize=False)", "imgs", imgs, self.real_state.device, (torch.uint8,), "uint8 images are scored")

    def _run(self, imgs: torch.Tensor, state: Optional[torch.Tensor], out: Optional[torch.Tensor], dtype, ws):
        imgs = self._check(imgs)
        dtype = self.compute_dtype if dtype is None else dtype
        n = imgs.shape[0]
        if n == 0:
            return
        step = min(n, self.chunk_images(dtype))
        need = ops.fid_workspace_bytes(step, MAP, MAP, FEATURES)
        if ws is None:
            ws = ops.workspace(need, imgs.device, "fid")
        packs = self._packed(dtype)
        for i0 in range(0, n, step):
            m = min(step, n - i0)
            f = ops.fid_prep(imgs[i0:i0 + m], dtype, SIZE, SIZE)
            for name, _, _, k, stride, pad in LAYERS:
                f = conv(f, *packs[name], k, stride, pad)
                if name != LAYERS[-1][0]:
                    ops.relu_(f)
            ops.fid_pool(f, ws)                                                 # ReLU on load
            ops.fid_accumulate(ws, m, MAP, MAP, FEATURES, state, None if out is None else out[i0:i0 + m])

    @torch.no_grad()
    def update(self, imgs: torch.Tensor, real: bool, *, dtype: Optional[torch.dtype] = None, ws: Optional[torch.Tensor] = None) -> None:
        """adds `[n, 3, h, w]` images to the real or the fake side.  `ws` (uint8, at least `workspace_bytes(n)`) lets a captured graph
        own its buffer."""
        self._run(imgs, self.real_state if real else self.fake_state, None, dtype, ws)
        self._n[bool(real)] += int(imgs.shape[0])

    @torch.no_grad()
    def features(self, imgs: torch.Tensor, *, dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
                 ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`[n, 3, h, w]` -> the fp64 `[n, 64]` features on the device; the running states are not touched"""
        n = imgs.shape[0]
        out = torch.empty(n, FEATURES, dtype=torch.float64, device=imgs.device) if out is None else out
        assert out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (n, FEATURES)
        self._run(imgs, None, out, dtype, ws)
        return out

    def _solve(self, out: torch.Tensor) -> None:
        ops.fid_compute(self.real_state, self.fake_state, out, self.info)      # the 64-wide solve in LDS: `compute(out=)` takes no workspace

    def forward(self, *args, **kw):
        raise NotImplementedError("FrechetInceptionDistance: call update(imgs, real) / compute() / reset(), as the reference does")
