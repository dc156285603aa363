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

import math
import warnings
from typing import Optional

import torch
from torch import nn

from . import ops
from .lpips import _Conv, _read

LAYERS = (("Conv2d_1a_3x3", 3, 32, 2, 0), ("Conv2d_2a_3x3", 32, 32, 1, 0), ("Conv2d_2b_3x3", 32, 64, 1, 1))     # name, c_in, c_out, stride, pad
BN_EPS = 1e-3
SIZE = 299                      # the extractor's input edge
MAP = 147                       # the edge of Conv2d_2b_3x3's output: 299 -> 149 -> 147 -> 147
FEATURES = 64
# layers of Inception-v3 behind the tap: their keys are in every published file and are not read
_LATER = ("Conv2d_3b_1x1.", "Conv2d_4a_3x3.", "Mixed_", "AuxLogits.", "fc.")


class _BN(nn.Module):
    """parameter holder with nn.BatchNorm2d's names"""

    def __init__(self, c: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(c), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(c), requires_grad=False)
        self.register_buffer("running_mean", torch.empty(c))
        self.register_buffer("running_var", torch.empty(c))


class _BasicConv(nn.Module):
    def __init__(self, c_in: int, c_out: int):
        super().__init__()
        self.conv = _Conv(c_out, c_in, 3, bias=False)
        self.bn = _BN(c_out)


class FrechetInceptionDistance(nn.Module):
    """`FrechetInceptionDistance(feature=64, normalize=True)`; fp32 parameters under torch-fidelity's key names
    (`Conv2d_{1a,2a,2b}_3x3.conv.weight`, `.bn.{weight,bias,running_mean,running_var}`).  `normalize=True`: float images in [0, 1];
    `normalize=False`: uint8 images.  `dtype`: the compute dtype of the activations and packed weights (float32 by default: a metric;
    float16 / bfloat16 are allowed).  The two running states (count, sum f, sum f^T f; fp64) live on the device; the sample counts are
    kept on the host too, so `compute()` can refuse without a synchronisation."""

    def __init__(self, feature: int = 64, normalize: bool = True, weights=None, dtype: torch.dtype = torch.float32, allow_random_init: bool = False):
        super().__init__()
        if feature in (192, 768, 2048):
            raise NotImplementedError(f"FrechetInceptionDistance(feature={feature}): only feature=64, the tap the reference scores with "
                                      "(Inception-v3 after its first max-pool), is built")
        if feature != 64:
            raise ValueError(f"FrechetInceptionDistance: feature={feature!r}; torchmetrics knows 64, 192, 768, 2048 and feature=64 is built")
        if dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"FrechetInceptionDistance: compute dtype {dtype}")
        self.compute_dtype = dtype
        self.normalize = bool(normalize)
        for name, c_in, c_out, _, _ in LAYERS:
            setattr(self, name, _BasicConv(c_in, c_out))
        self.register_buffer("real_state", torch.zeros(ops.FID_STATE, dtype=torch.float64), persistent=False)
        self.register_buffer("fake_state", torch.zeros(ops.FID_STATE, dtype=torch.float64), persistent=False)
        self.register_buffer("info", torch.zeros(ops.FID_INFO, dtype=torch.float64), persistent=False)
        self._n = {True: 0, False: 0}
        self._packs: dict = {}
        self.reset_parameters()
        if weights is not None:
            self.load_weights(weights)
        elif not allow_random_init:
            warnings.warn("FrechetInceptionDistance(): no weight file given -- the module keeps RANDOM initial weights and its scores mean nothing "
                          "(pass weights=... / call load_weights, or allow_random_init=True to silence)", stacklevel=2)

    def reset_parameters(self, seed: Optional[int] = None):
        """Kaiming-normal convs, BatchNorm close to the identity"""
        g = None if seed is None else torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, *_ in LAYERS:
                m = self.get_submodule(name)
                m.conv.weight.copy_(torch.randn(m.conv.weight.shape, generator=g) * math.sqrt(2.0 / (9 * m.conv.weight.shape[1])))
                m.bn.weight.copy_(0.5 + torch.rand(m.bn.weight.shape, generator=g))
                m.bn.bias.copy_(0.1 * torch.randn(m.bn.bias.shape, generator=g))
                m.bn.running_mean.copy_(0.1 * torch.randn(m.bn.running_mean.shape, generator=g))
                m.bn.running_var.copy_(0.5 + torch.rand(m.bn.running_var.shape, generator=g))
        self._packs.clear()

    # ---- weights ---------------------------------------------------------------------------------------------------------------
    def load_weights(self, weights) -> "FrechetInceptionDistance":
        """`weights`: a state dict or the path of one (read with `torch.load(weights_only=True)`): torch-fidelity's `pt_inception`
        (`Conv2d_1a_3x3.conv.weight`, ...) or a torchmetrics FID state dict (the same keys under `inception.`).  Read:
        `Conv2d_{1a,2a,2b}_3x3.conv.weight` and `.bn.{weight,bias,running_mean,running_var}`.  Ignored: `num_batches_tracked` and the
        layers behind the tap (`Conv2d_3b_1x1.*`, `Conv2d_4a_3x3.*`, `Mixed_*`, `AuxLogits.*`, `fc.*`).  Anything else, or a missing
        key, raises a KeyError that names it; a wrong shape or a non-positive `running_var + 1e-3` a ValueError."""
        sd = _read(weights)
        if any(k.startswith("inception.") for k in sd):
            sd = {(k[len("inception."):] if k.startswith("inception.") else k): v for k, v in sd.items()}
        want = dict(self.state_dict())              # the running states are not persistent: the fifteen weight tensors only
        ignored = lambda k: k.endswith("num_batches_tracked") or k.startswith(_LATER)
        missing = sorted(k for k in want if k not in sd)
        unexpected = sorted(k for k in sd if k not in want and not ignored(k))
        if missing or unexpected:
            raise KeyError(f"FrechetInceptionDistance.load_weights: missing keys {missing}, unexpected keys {unexpected}")
        for k, ref in want.items():
            if tuple(sd[k].shape) != tuple(ref.shape):
                raise ValueError(f"FrechetInceptionDistance.load_weights: {k} has shape {tuple(sd[k].shape)}, expected {tuple(ref.shape)}")
            if k.endswith("running_var") and not bool((sd[k].detach().double() + BN_EPS > 0).all()):
                raise ValueError(f"FrechetInceptionDistance.load_weights: {k} + {BN_EPS} is not positive everywhere; BatchNorm divides by its root")
        with torch.no_grad():
            for k, ref in want.items():
                ref.copy_(sd[k].detach().to(torch.float32))
        self._packs.clear()
        return self

    def _apply(self, fn, *args, **kw):
        self._packs.clear()                     # .to(device) / .float(): the packs follow the parameters
        out = super()._apply(fn, *args, **kw)
        for name in ("real_state", "fake_state", "info"):      # the statistics stay fp64 whatever the module is cast to
            if self._buffers[name].dtype != torch.float64:
                self._buffers[name] = self._buffers[name].double()
        return out

    def _packed(self, dtype: torch.dtype):
        """[(packed weight, fp32 bias)] of the three convs with BatchNorm folded in, in fp64 on the host"""
        mods = [self.get_submodule(name) for name, *_ in LAYERS]
        dev = mods[0].conv.weight.device
        key = (dtype, str(dev))
        version = tuple(t._version for m in mods for t in (m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var))
        hit = self._packs.get(key)
        if hit is None or hit[0] != version:
            packs = []
            for m in mods:
                var = m.bn.running_var.detach().double().cpu() + BN_EPS
                if not bool((var > 0).all()):
                    raise ValueError(f"FrechetInceptionDistance: running_var + {BN_EPS} is not positive everywhere")
                g = m.bn.weight.detach().double().cpu() / var.sqrt()
                w = m.conv.weight.detach().double().cpu() * g.view(-1, 1, 1, 1)
                b = m.bn.bias.detach().double().cpu() - m.bn.running_mean.detach().double().cpu() * g
                packs.append((ops.pack_weight(w.float().to(dev), dtype), b.float().to(dev)))
            hit = (version, packs)
            self._packs[key] = hit
        return hit[1]

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
        if not imgs.is_cuda:
            raise RuntimeError("mv_ldm_amd modules run only on a HIP device (no CPU fallback): move the module and its inputs to 'cuda'")
        if imgs.dim() != 4 or imgs.shape[1] != 3:
            raise ValueError(f"FrechetInceptionDistance: imgs must be [n, 3, h, w], got {tuple(imgs.shape)}")
        if self.normalize:
            if imgs.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                raise TypeError(f"FrechetInceptionDistance(normalize=True): imgs is {imgs.dtype}; float32, bfloat16 or float16 images in [0, 1] are scored")
        elif imgs.dtype != torch.uint8:
            raise TypeError(f"FrechetInceptionDistance(normalize=False): imgs is {imgs.dtype}; uint8 images are scored")
        if not imgs.is_contiguous():
            raise ValueError(f"FrechetInceptionDistance: imgs must be contiguous NCHW (got strides {imgs.stride()}); call .contiguous() first")
        if self.real_state.device != imgs.device:
            raise RuntimeError(f"FrechetInceptionDistance: the module is on {self.real_state.device}, the images on {imgs.device} (no CPU fallback: module.to('cuda'))")
        if imgs.shape[2] < 1 or imgs.shape[3] < 1:
            raise ValueError(f"FrechetInceptionDistance: imgs {tuple(imgs.shape)} has an empty edge")
        return imgs if imgs.dtype in (torch.float32, torch.uint8) else ops.convert(imgs, torch.float32)

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
            for k, (_, _, _, stride, pad) in enumerate(LAYERS):
                f = ops.conv2d(f, packs[k][0], packs[k][1], stride=stride, pad=pad)
                if k + 1 < len(LAYERS):
                    ops.lpips_relu(f)
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

    @torch.no_grad()
    def compute(self, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the 0-d fp32 score on the device.  Raises the package's RuntimeError below 2 samples on a side (host counters: no
        synchronisation).  `self.info` then holds the solves' record (`ops.fid_compute`)."""
        if self._n[True] < 2 or self._n[False] < 2:
            raise RuntimeError("More than one sample is required for both the real and fake distributed to compute FID")
        out = torch.empty((), dtype=torch.float32, device=self.real_state.device) if out is None else out
        ops.fid_compute(self.real_state, self.fake_state, out, self.info)
        return out.view(())

    def reset(self) -> None:
        """both sides empty again (stream-ordered fills of the two states)"""
        self.real_state.zero_()
        self.fake_state.zero_()
        self._n = {True: 0, False: 0}

    def forward(self, *args, **kw):
        raise NotImplementedError("FrechetInceptionDistance: call update(imgs, real) / compute() / reset(), as the reference does")
