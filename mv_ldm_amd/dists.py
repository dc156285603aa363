"""DISTS on the device: the counterpart of `DISTS_pytorch.DISTS()` as `src/evaluation/metrics.py:27-40` uses it (`get_dists`,
`compute_dists`: `forward(ground_truth, predicted)`).

The trunk is the thirteen 3x3 convolutions of VGG-16 LPIPS runs too, through the implicit GEMM (`ops.conv2d`, with their bias); the input
normalisation, the L2 pooling that replaces every max-pool, the per-channel sums of each of the six taps (the raw image and the five
stages) and the fold into one score are `csrc/dists.hip`.  Both inputs go through every conv as ONE batch of 2n images.  The sums are
fp64 from the first product on, so the one-pass variances are good far below the package's c2 = 1e-6.

No pretrained file ships with this package and none is fetched: `load_weights` takes the user's file(s), in the `DISTS_pytorch`
package's own key layout or as torchvision's VGG-16 plus the package's `weights.pt`.  The package's arithmetic is restated, not pinned
against the package itself ("parity unpinned").
"""
from __future__ import annotations

import math
import warnings
from typing import List, Optional

import torch
from torch import nn

from . import ops
from .lpips import LPIPS, _Conv, _read

# stage -> torchvision `features` indices of its convs (the ReLUs and L2 pools between them hold no parameters)
VGG_STAGES = {1: (0, 2), 2: (5, 7), 3: (10, 12, 14), 4: (17, 19, 21), 5: (24, 26, 28)}
VGG_WIDTH = {1: 64, 2: 128, 3: 256, 4: 512, 5: 512}
L2POOLS = {2: 4, 3: 9, 4: 16, 5: 23}          # stage -> index of the L2pooling that opens it (its `filter` buffer is a constant here)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
N_CHANNELS = sum(ops.DISTS_CHANNELS)          # 1475


def _conv_names() -> List[str]:
    return [f"stage{s}.{i}" for s, idx in VGG_STAGES.items() for i in idx]


def _constants() -> dict:
    """the package's buffers the kernels carry as constants: optional in a file, and a file that disagrees is another metric"""
    hann = torch.tensor([1.0, 2.0, 1.0])
    g = torch.outer(hann, hann) / 16.0
    out = {"mean": torch.tensor(MEAN).view(1, 3, 1, 1), "std": torch.tensor(STD).view(1, 3, 1, 1)}
    for s, i in L2POOLS.items():
        out[f"stage{s}.{i}.filter"] = g.view(1, 1, 3, 3).repeat(VGG_WIDTH[s - 1], 1, 1, 1)
    return out


class DISTS(nn.Module):
    """`DISTS_pytorch.DISTS()`; fp32 parameters under the package's key names (`stage1.{0,2}`, `stage2.{5,7}`, `stage3.{10,12,14}`,
    `stage4.{17,19,21}`, `stage5.{24,26,28}`, each `.weight|.bias`, and `alpha`, `beta` `[1, 1475, 1, 1]`).  `dtype`: the compute dtype
    of the activations and packed weights (float32 by default: a metric; float16 / bfloat16 are allowed).  `weights` / `alpha_beta`:
    see `load_weights`; without them the module keeps a random init and says so."""

    def __init__(self, weights=None, alpha_beta=None, dtype: torch.dtype = torch.float32, allow_random_init: bool = False):
        super().__init__()
        if dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"DISTS: compute dtype {dtype}")
        self.compute_dtype = dtype
        c_in = 3
        for s, idx in VGG_STAGES.items():
            convs = {}
            for i in idx:
                convs[str(i)] = _Conv(VGG_WIDTH[s], c_in, 3)
                c_in = VGG_WIDTH[s]
            setattr(self, f"stage{s}", nn.ModuleDict(convs))
        self.alpha = nn.Parameter(torch.empty(1, N_CHANNELS, 1, 1), requires_grad=False)
        self.beta = nn.Parameter(torch.empty(1, N_CHANNELS, 1, 1), requires_grad=False)
        self._packs: dict = {}
        self.reset_parameters()
        if weights is not None:
            self.load_weights(weights, alpha_beta)
        elif not allow_random_init:
            warnings.warn("DISTS(): no weight file given -- the module keeps RANDOM initial weights and its scores mean nothing "
                          "(pass weights=... / call load_weights, or allow_random_init=True to silence)", stacklevel=2)

    def reset_parameters(self, seed: Optional[int] = None):
        """Kaiming-normal convs, small biases, alpha and beta |N(0.1, 0.01)| as the package initialises them"""
        g = None if seed is None else torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name in _conv_names():
                m = self.get_submodule(name)
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / (9 * m.weight.shape[1])))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)
            for p in (self.alpha, self.beta):
                p.copy_((0.1 + 0.01 * torch.randn(p.shape, generator=g)).abs())
        self._packs.clear()

    # ---- weights ---------------------------------------------------------------------------------------------------------------
    def load_weights(self, weights, alpha_beta=None) -> "DISTS":
        """`weights`: a state dict or the path of one (read with `torch.load(weights_only=True)`), either
          * a full `DISTS_pytorch.DISTS().state_dict()` (`stage*`, `alpha`, `beta`; its `mean`, `std` and `stage{2..5}.{4,9,16,23}.filter`
            buffers are optional and must equal the package's constants within 1e-6), or
          * torchvision's VGG-16 (`features.{idx}.weight|bias`; its `classifier.*` is not part of DISTS and is ignored) together with
            `alpha_beta`: the package's `weights.pt` (`alpha`, `beta`).
        Missing and unexpected keys raise a KeyError that names them."""
        sd = _read(weights)
        if any(k.startswith("features.") for k in sd):
            if alpha_beta is None:
                raise KeyError("a torchvision VGG-16 state dict holds no `alpha` / `beta`: pass the DISTS_pytorch package's weights.pt as `alpha_beta`")
            mapped = {}
            for k, v in sd.items():
                if k.startswith("classifier."):
                    continue
                parts = k.split(".")
                owner = next((s for s, idx in VGG_STAGES.items() if len(parts) == 3 and parts[1].isdigit() and int(parts[1]) in idx), None)
                mapped[k if owner is None else f"stage{owner}.{parts[1]}.{parts[2]}"] = v
            mapped.update(_read(alpha_beta))
            sd = mapped
        elif alpha_beta is not None:
            sd.update(_read(alpha_beta))
        want = dict(self.state_dict())
        consts = _constants()
        missing = sorted(k for k in want if k not in sd)
        unexpected = sorted(k for k in sd if k not in want and k not in consts)
        if missing or unexpected:
            raise KeyError(f"DISTS.load_weights: missing keys {missing}, unexpected keys {unexpected}")
        for k, v in sd.items():
            ref = want[k] if k in want else consts[k]
            if tuple(v.shape) != tuple(ref.shape):
                raise ValueError(f"DISTS.load_weights: {k} has shape {tuple(v.shape)}, expected {tuple(ref.shape)}")
        for k in consts.keys() & sd.keys():     # the kernels carry the package's constants: a file that disagrees is another metric
            if not torch.allclose(sd[k].detach().float().cpu(), consts[k], rtol=0, atol=1e-6):
                raise ValueError(f"DISTS.load_weights: {k} is not the DISTS_pytorch package's constant (mean / std of ImageNet, the 3x3 Hann filter)")
        wsum = float(sd["alpha"].detach().double().sum() + sd["beta"].detach().double().sum())
        if not wsum > 0:
            raise ValueError(f"DISTS.load_weights: sum(alpha) + sum(beta) = {wsum}; the score divides by it")
        with torch.no_grad():
            for k, v in sd.items():
                if k in want:
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
    chunk_pairs = staticmethod(LPIPS.chunk_pairs)       # the same largest operand: conv1's output, 2 x pairs x h x w x 64

    @torch.no_grad()
    def forward(self, x: torch.Tensor, y: torch.Tensor, require_grad: bool = False, batch_average: bool = False, *,
                dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`[n, 3, h, w]` x 2 in [0, 1] -> `[n]` fp32 on the device, always 1-d (the package squeezes n = 1 to 0-d, which the reference's
        `compute_dists` undoes).  `out` (fp32, n elements) and `ws` (uint8, at least `ops.dists_workspace_bytes` of one chunk) let a
        captured graph own its buffers."""
        if require_grad:
            raise NotImplementedError("DISTS: no backward pass is built (require_grad=True)")
        if batch_average:
            raise NotImplementedError("DISTS: batch_average=True is not built; take .mean() of the per-pair scores")
        for name, t in (("x", x), ("y", y)):
            if not t.is_cuda:
                raise RuntimeError("mv_ldm_amd modules run only on a HIP device (no CPU fallback): move the module and its inputs to 'cuda'")
            if t.dim() != 4 or t.shape[1] != 3:
                raise ValueError(f"DISTS: {name} must be [n, 3, h, w], got {tuple(t.shape)}")
            if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                raise TypeError(f"DISTS: {name} is {t.dtype}; float32, bfloat16 or float16 images are scored")
            if not t.is_contiguous():
                raise ValueError(f"DISTS: {name} must be contiguous NCHW (got strides {t.stride()}); call .contiguous() first")
        if x.shape != y.shape or x.device != y.device:
            raise ValueError(f"DISTS: x {tuple(x.shape)} on {x.device} against y {tuple(y.shape)} on {y.device}")
        if self.alpha.device != x.device:
            raise RuntimeError(f"DISTS: the module is on {self.alpha.device}, the images on {x.device} (no CPU fallback: module.to('cuda'))")
        x = x if x.dtype == torch.float32 else ops.convert(x, torch.float32)
        y = y if y.dtype == torch.float32 else ops.convert(y, torch.float32)
        dtype = self.compute_dtype if dtype is None else dtype
        n, _, h, w = x.shape
        out = torch.empty(n, dtype=torch.float32, device=x.device) if out is None else out
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n
        if n == 0:
            return out.view(n)
        step = min(n, self.chunk_pairs(h, w, dtype))
        need = ops.dists_workspace_bytes(step, h, w)
        if need == 0:
            raise ops.L.MvldmError(f"DISTS: a {h} x {w} image is refused (an edge below 1, or too large)")
        if ws is None:
            ws = ops.workspace(need, x.device, "dists")
        convs, packs = self._packed(dtype)
        taps, stride = ops.dists_layout(h, w)
        alpha, beta = self.alpha.view(-1), self.beta.view(-1)
        flat = out.view(-1)
        for i0 in range(0, n, step):
            m = min(step, n - i0)
            xa, ya = x[i0:i0 + m], y[i0:i0 + m]
            ops.dists_stats(xa, ws, taps[0][3], stride, feat_b=ya)          # tap 0: the raw fp32 images
            f = ops.dists_prep(xa, ya, dtype)
            k = 0
            for l, idx in enumerate(VGG_STAGES.values()):
                for j in range(len(idx)):
                    f = ops.conv2d(f, packs[k], convs[k].bias)
                    k += 1
                    if j + 1 < len(idx):
                        ops.lpips_relu(f)
                ops.dists_stats(f, ws, taps[l + 1][3], stride)              # ReLU on load
                if l < 4:
                    f = ops.dists_l2pool(f)
            ops.dists_fold(ws, m, h, w, alpha, beta, flat[i0:i0 + m])
        return out.view(n)
