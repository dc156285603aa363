"""LPIPS(net="vgg") on the device: the counterpart of `lpips.LPIPS(net="vgg")` as `src/evaluation/metrics.py:43-54` uses it
(`get_lpips`, `compute_lpips`: `forward(ground_truth, predicted, normalize=True)[:, 0, 0, 0]`).

The VGG-16 trunk is thirteen 3x3 convolutions, which run through the implicit GEMM (`ops.conv2d`, with their bias); the ScalingLayer,
the ReLUs between convs, the channel-normalised weighted distance at the five taps with the 2x2 max-pool that follows each, and the
fold over layers are `csrc/lpips.hip`.  Both inputs go through every conv as ONE batch of 2n images.

No pretrained file ships with this package and none is fetched: `load_weights` takes the user's file(s), in the `lpips` package's
own key layout or as torchvision's VGG-16 plus the package's `vgg.pth`.  The package's arithmetic is restated, not pinned against the
package itself ("parity unpinned").
"""
from __future__ import annotations

import math
import warnings
from pathlib import Path
from typing import Dict, List, Optional, Union

import torch
from torch import nn

from . import ops

# slice -> torchvision `features` indices of its convs (the ReLUs and pools between them hold no parameters)
VGG_SLICES = {1: (0, 2), 2: (5, 7), 3: (10, 12, 14), 4: (17, 19, 21), 5: (24, 26, 28)}
VGG_WIDTH = {1: 64, 2: 128, 3: 256, 4: 512, 5: 512}
SHIFT = (-0.030, -0.088, -0.188)          # the package's ScalingLayer
SCALE = (0.458, 0.448, 0.450)


class _Conv(nn.Module):
    """parameter holder with nn.Conv2d's names (the convolution itself is `ops.conv2d` on the packed weight)"""

    def __init__(self, c_out: int, c_in: int, k: int, bias: bool = True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(c_out, c_in, k, k), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(c_out), requires_grad=False) if bias else None


class _Lin(nn.Module):
    """`NetLinLayer`: model = [Dropout, Conv2d(C, 1, 1, bias=False)] -- key `model.1.weight`"""

    def __init__(self, c: int):
        super().__init__()
        self.model = nn.ModuleDict({"1": _Conv(1, c, 1, bias=False)})


class _Scaling(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT).view(1, 3, 1, 1))
        self.register_buffer("scale", torch.tensor(SCALE).view(1, 3, 1, 1))


def _conv_names() -> List[str]:
    return [f"net.slice{s}.{i}" for s, idx in VGG_SLICES.items() for i in idx]


def _read(src) -> Dict[str, torch.Tensor]:
    if isinstance(src, (str, Path)):
        src = torch.load(str(src), map_location="cpu", weights_only=True)
    if not isinstance(src, dict):
        raise TypeError(f"expected a state dict or the path of one, got {type(src).__name__}")
    return dict(src)


class LPIPS(nn.Module):
    """`LPIPS(net="vgg")`; fp32 parameters under the package's key names (`net.slice{1..5}.{idx}.weight|bias`,
    `lin{0..4}.model.1.weight`, buffers `scaling_layer.shift|scale`).  `dtype`: the compute dtype of the activations and packed
    weights (float32 by default: a metric; float16 / bfloat16 are allowed).  `weights` / `lin`: see `load_weights`; without them the
    module keeps a random init and says so."""

    def __init__(self, net: str = "vgg", weights=None, lin=None, dtype: torch.dtype = torch.float32, allow_random_init: bool = False):
        super().__init__()
        if net != "vgg":
            raise NotImplementedError(f"LPIPS(net={net!r}): only the VGG-16 variant the reference scores with is built")
        if dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"LPIPS: compute dtype {dtype}")
        self.compute_dtype = dtype
        self.scaling_layer = _Scaling()
        self.net = nn.Module()
        c_in = 3
        for s, idx in VGG_SLICES.items():
            convs = {}
            for i in idx:
                convs[str(i)] = _Conv(VGG_WIDTH[s], c_in, 3)
                c_in = VGG_WIDTH[s]
            setattr(self.net, f"slice{s}", nn.ModuleDict(convs))
        for k in range(5):
            setattr(self, f"lin{k}", _Lin(VGG_WIDTH[k + 1]))
        self._packs: dict = {}
        self.reset_parameters()
        if weights is not None:
            self.load_weights(weights, lin)
        elif not allow_random_init:
            warnings.warn("LPIPS(): no weight file given -- the module keeps RANDOM initial weights and its scores mean nothing "
                          "(pass weights=... / call load_weights, or allow_random_init=True to silence)", stacklevel=2)

    def reset_parameters(self, seed: Optional[int] = None):
        """Kaiming-normal convs, small biases, small non-negative `lin` weights (the published ones are non-negative)"""
        g = None if seed is None else torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name in _conv_names():
                m = self.get_submodule(name)
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / (9 * m.weight.shape[1])))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)
            for k in range(5):
                wt = self.get_submodule(f"lin{k}.model.1").weight
                wt.copy_(torch.rand(wt.shape, generator=g) * 0.02)
        self._packs.clear()

    # ---- weights ---------------------------------------------------------------------------------------------------------------
    def load_weights(self, weights, lin=None) -> "LPIPS":
        """`weights`: a state dict or the path of one (read with `torch.load(weights_only=True)`), either
          * a full `lpips.LPIPS(net="vgg").state_dict()` (`net.slice*`, `lin*`, `scaling_layer.*`; the `lins.{k}.*` duplicates of the
            package's ModuleList are accepted and ignored), or
          * torchvision's VGG-16 (`features.{idx}.weight|bias`; its `classifier.*` is not part of LPIPS and is ignored) together with
            `lin`: the package's `weights/v0.1/vgg.pth` (`lin{k}.model.1.weight`).
        Missing and unexpected keys raise a KeyError that names them."""
        sd = _read(weights)
        if any(k.startswith("features.") for k in sd):
            if lin is None:
                raise KeyError("a torchvision VGG-16 state dict holds no `lin` layers: pass the lpips package's vgg.pth as `lin`")
            mapped = {}
            for k, v in sd.items():
                if k.startswith("classifier."):
                    continue
                parts = k.split(".")
                owner = next((s for s, idx in VGG_SLICES.items() if len(parts) == 3 and parts[1].isdigit() and int(parts[1]) in idx), None)
                mapped[k if owner is None else f"net.slice{owner}.{parts[1]}.{parts[2]}"] = v
            mapped.update(_read(lin))
            sd = mapped
        elif lin is not None:
            sd.update(_read(lin))
        sd = {k: v for k, v in sd.items() if not k.startswith("lins.")}
        want = {k: v for k, v in self.state_dict().items()}
        optional = {"scaling_layer.shift", "scaling_layer.scale"}
        missing = sorted(k for k in want if k not in sd and k not in optional)
        unexpected = sorted(k for k in sd if k not in want)
        if missing or unexpected:
            raise KeyError(f"LPIPS.load_weights: missing keys {missing}, unexpected keys {unexpected}")
        for k, v in sd.items():
            if tuple(v.shape) != tuple(want[k].shape):
                raise ValueError(f"LPIPS.load_weights: {k} has shape {tuple(v.shape)}, expected {tuple(want[k].shape)}")
        for k in optional & sd.keys():          # the kernel carries the package's constants: a file that disagrees is another metric
            if not torch.allclose(sd[k].detach().float().cpu(), want[k].cpu(), rtol=0, atol=1e-6):
                raise ValueError(f"LPIPS.load_weights: {k} = {sd[k].flatten().tolist()} is not the lpips package's ScalingLayer")
        with torch.no_grad():
            for k, v in sd.items():
                if k not in optional:
                    want[k].copy_(v.detach().to(torch.float32))
        self._packs.clear()
        return self

    def _apply(self, fn, *args, **kw):
        self._packs.clear()                     # .to(device) / .float(): the packs follow the parameters
        return super()._apply(fn, *args, **kw)

    def _packed(self, dtype: torch.dtype):
        convs = [self.get_submodule(n) for n in _conv_names()]
        key = (dtype, str(convs[0].weight.device))
        version = tuple(m.weight._version for m in convs)
        hit = self._packs.get(key)
        if hit is None or hit[0] != version:
            hit = (version, [ops.pack_weight(m.weight, dtype) for m in convs])
            self._packs[key] = hit
        return convs, hit[1]

    # ---- forward ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def chunk_pairs(h: int, w: int, dtype: torch.dtype) -> int:
        """pairs per launch so that the largest operand (conv1's output, 2 x pairs x h x w x 64) does not pass 2 GiB: the 32-bit
        buffer-offset rule of the implicit GEMM -- 64 pairs of 256 x 256 in f32"""
        es = 4 if dtype == torch.float32 else 2
        return max(1, (1 << 31) // (2 * h * w * 64 * es))

    @torch.no_grad()
    def forward(self, in0: torch.Tensor, in1: torch.Tensor, normalize: bool = False, *, dtype: Optional[torch.dtype] = None,
                out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`[n, 3, h, w]` x 2 -> `[n, 1, 1, 1]` fp32 on the device.  `normalize`: the inputs are in [0, 1] (mapped to [-1, 1] first).
        `out` (fp32, n elements) and `ws` (uint8, at least `ops.lpips_workspace_bytes` of one chunk) let a captured graph own its buffers."""
        for name, t in (("in0", in0), ("in1", in1)):
            if not t.is_cuda:
                raise RuntimeError("mv_ldm_amd modules run only on a HIP device (no CPU fallback): move the module and its inputs to 'cuda'")
            if t.dim() != 4 or t.shape[1] != 3:
                raise ValueError(f"LPIPS: {name} must be [n, 3, h, w], got {tuple(t.shape)}")
            if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                raise TypeError(f"LPIPS: {name} is {t.dtype}; float32, bfloat16 or float16 images are scored")
            if not t.is_contiguous():
                raise ValueError(f"LPIPS: {name} must be contiguous NCHW (got strides {t.stride()}); call .contiguous() first")
        if in0.shape != in1.shape or in0.device != in1.device:
            raise ValueError(f"LPIPS: in0 {tuple(in0.shape)} on {in0.device} against in1 {tuple(in1.shape)} on {in1.device}")
        if self.scaling_layer.shift.device != in0.device:
            raise RuntimeError(f"LPIPS: the module is on {self.scaling_layer.shift.device}, the images on {in0.device} (no CPU fallback: module.to('cuda'))")
        in0 = in0 if in0.dtype == torch.float32 else ops.convert(in0, torch.float32)
        in1 = in1 if in1.dtype == torch.float32 else ops.convert(in1, torch.float32)
        dtype = self.compute_dtype if dtype is None else dtype
        n, _, h, w = in0.shape
        out = torch.empty(n, 1, 1, 1, dtype=torch.float32, device=in0.device) if out is None else out
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n
        if n == 0:
            return out.view(n, 1, 1, 1)
        step = min(n, self.chunk_pairs(h, w, dtype))
        need = ops.lpips_workspace_bytes(step, h, w)
        if need == 0:
            raise ops.L.MvldmError(f"LPIPS: a {h} x {w} image leaves nothing after four 2x2 pool stages (at least {ops.LPIPS_MIN_EDGE} x {ops.LPIPS_MIN_EDGE})")
        if ws is None:
            ws = ops.workspace(need, in0.device, "lpips")
        convs, packs = self._packed(dtype)
        lins = [self.get_submodule(f"lin{k}.model.1").weight.view(-1) for k in range(5)]
        slots = [ops.lpips_tap_slots(h >> l, w >> l, c) for l, c in enumerate(ops.LPIPS_CHANNELS)]
        flat = out.view(-1)
        for i0 in range(0, n, step):
            m = min(step, n - i0)
            x = ops.lpips_prep(in0[i0:i0 + m], in1[i0:i0 + m], dtype, normalize)
            k, slot0 = 0, 0
            for l, idx in enumerate(VGG_SLICES.values()):
                for j in range(len(idx)):
                    x = ops.conv2d(x, packs[k], convs[k].bias)
                    k += 1
                    if j + 1 < len(idx):
                        ops.lpips_relu(x)
                x = ops.lpips_tap(x, lins[l], ws, slot0, sum(slots), pool=l < 4)
                slot0 += slots[l]
            ops.lpips_fold(ws, m, h, w, flat[i0:i0 + m])
        return out.view(n, 1, 1, 1)
