"""What the metric networks share (lpips.py, dists.py, fid.py, cleanfid.py), each piece once: the state-dict reader and loader, the
parameter holders, the pack cache, the BatchNorm fold, the image check, the VGG-16 trunk of LPIPS and DISTS, the Inception conv stack of
FID and Clean-FID, and the fp64 running statistics of the two Frechet distances.  Private: the four modules are the interface.
"""
from __future__ import annotations

import math
import warnings
from pathlib import Path
from typing import Dict, Optional

import torch
from torch import nn

from . import ops

FLOATS = (torch.float32, torch.float16, torch.bfloat16)
BN_EPS = 1e-3


def read_state(src) -> Dict[str, torch.Tensor]:
    if isinstance(src, (str, Path)):
        src = torch.load(str(src), map_location="cpu", weights_only=True)
    if not isinstance(src, dict):
        raise TypeError(f"expected a state dict or the path of one, got {type(src).__name__}")
    return dict(src)


# ---- parameter holders -------------------------------------------------------------------------------------------------------------
class Conv(nn.Module):
    """parameter holder with nn.Conv2d's names (the convolution itself is `ops.conv2d` on the packed weight); the kernel may be oblong"""

    def __init__(self, c_out: int, c_in: int, kh: int, kw: int, bias: bool = True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(c_out, c_in, kh, kw), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(c_out), requires_grad=False) if bias else None


class BatchNorm(nn.Module):
    """parameter holder with nn.BatchNorm2d's names"""

    def __init__(self, c: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(c), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(c), requires_grad=False)
        self.register_buffer("running_mean", torch.empty(c))
        self.register_buffer("running_var", torch.empty(c))


class BasicConv(nn.Module):
    def __init__(self, c_in: int, c_out: int, k):
        super().__init__()
        self.conv = Conv(c_out, c_in, *k, bias=False)
        self.bn = BatchNorm(c_out)


def add_submodule(root: nn.Module, name: str, leaf: nn.Module) -> None:
    """`leaf` under the dotted `name`, with plain containers on the way"""
    *path, last = name.split(".")
    for p in path:
        if not hasattr(root, p):
            setattr(root, p, nn.Module())
        root = getattr(root, p)
    setattr(root, last, leaf)


# ---- checks and loading --------------------------------------------------------------------------------------------------------------
def check_images(who: str, name: str, t: torch.Tensor, module_device, dtypes=FLOATS, scored: str = "float32, bfloat16 or float16 images are scored") -> torch.Tensor:
    """the one check of an `[n, 3, h, w]` input; returns it as the kernels read it (fp32, or uint8 where `dtypes` allows it)"""
    if not t.is_cuda:
        raise RuntimeError("mv_ldm_amd modules run only on a HIP device (no CPU fallback): move the module and its inputs to 'cuda'")
    if t.dim() != 4 or t.shape[1] != 3:
        raise ValueError(f"{who}: {name} must be [n, 3, h, w], got {tuple(t.shape)}")
    if t.dtype not in dtypes:
        raise TypeError(f"{who}: {name} is {t.dtype}; {scored}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous NCHW (got strides {t.stride()}); call .contiguous() first")
    if module_device != t.device:
        raise RuntimeError(f"{who}: the module is on {module_device}, the images on {t.device} (no CPU fallback: module.to('cuda'))")
    if t.shape[2] < 1 or t.shape[3] < 1:
        raise ValueError(f"{who}: {name} {tuple(t.shape)} has an empty edge")
    return t if t.dtype in (torch.float32, torch.uint8) else ops.convert(t, torch.float32)


def load_state(module: nn.Module, sd: dict, ignored=lambda k: False, constants: Optional[dict] = None, source: str = "", check=None) -> None:
    """copies `sd` into `module`'s fp32 state.  `ignored(key)`: keys of a published file that are not read.  `constants`: key -> the value
    the kernels carry; optional in a file, never copied, and a file that disagrees (1e-6) is another metric (`source` names theirs).
    `check(sd)`: the module's own refusals.  Missing and unexpected keys raise a KeyError that names them, a wrong shape a ValueError;
    every check runs before the first copy, so a refused file changes nothing."""
    who = f"{type(module).__name__}.load_weights"
    want, constants = dict(module.state_dict()), constants or {}
    missing = sorted(k for k in want if k not in sd and k not in constants)
    unexpected = sorted(k for k in sd if k not in want and k not in constants and not ignored(k))
    if missing or unexpected:
        raise KeyError(f"{who}: missing keys {missing}, unexpected keys {unexpected}")
    read = {k: v for k, v in sd.items() if k in want or k in constants}
    for k, v in read.items():
        ref = constants[k] if k in constants else want[k]
        if tuple(v.shape) != tuple(ref.shape):
            raise ValueError(f"{who}: {k} has shape {tuple(v.shape)}, expected {tuple(ref.shape)}")
        if k in constants and not torch.allclose(v.detach().float().cpu(), ref, rtol=0, atol=1e-6):
            raise ValueError(f"{who}: {k} is not {source}")
    if check is not None:
        check(read)
    with torch.no_grad():
        for k, v in read.items():
            if k not in constants:
                want[k].copy_(v.detach().to(torch.float32))


def fold_batchnorm(conv: Conv, bn: BatchNorm, eps: float = BN_EPS, name: str = "bn"):
    """fp32 (weight, bias) on the host of the convolution with its BatchNorm folded in, computed in fp64:
    w' = w g, b' = beta - mean g, g = gamma / sqrt(var + eps)"""
    var = bn.running_var.detach().double().cpu() + eps
    if not bool((var > 0).all()):
        raise ValueError(f"{name}.running_var + {eps} is not positive everywhere")
    g = bn.weight.detach().double().cpu() / var.sqrt()
    w = conv.weight.detach().double().cpu() * g.view(-1, 1, 1, 1)
    b = bn.bias.detach().double().cpu() - bn.running_mean.detach().double().cpu() * g
    return w.float(), b.float()


class PackedNet(nn.Module):
    """a network whose convolutions read packed copies of its fp32 weights: the compute dtype, the pack cache and the end of every
    constructor (random init, then the user's file or a warning)"""

    def __init__(self, dtype: torch.dtype):
        super().__init__()
        if dtype not in FLOATS:
            raise TypeError(f"{type(self).__name__}: compute dtype {dtype}")
        self.compute_dtype = dtype
        self._packs: dict = {}

    def _init_weights(self, weights, allow_random_init: bool, *more) -> None:
        self.reset_parameters()
        if weights is not None:
            self.load_weights(weights, *more)
        elif not allow_random_init:
            warnings.warn(f"{type(self).__name__}(): no weight file given -- the module keeps RANDOM initial weights and its scores mean nothing "
                          "(pass weights=... / call load_weights, or allow_random_init=True to silence)", stacklevel=3)

    def _apply(self, fn, *args, **kw):
        self._packs.clear()                     # .to(device) / .float(): the packs follow the parameters
        return super()._apply(fn, *args, **kw)

    def _cached(self, dtype: torch.dtype, sources, build):
        """`build()` per (dtype, device), again whenever one of the `sources` tensors was written to"""
        key = (dtype, str(sources[0].device))
        version = tuple(t._version for t in sources)
        hit = self._packs.get(key)
        if hit is None or hit[0] != version:
            hit = (version, build())
            self._packs[key] = hit
        return hit[1]


# ---- the VGG-16 trunk of LPIPS and DISTS ---------------------------------------------------------------------------------------------
# slice (stage) -> torchvision `features` indices of its convs (the ReLUs and pools between them hold no parameters)
VGG_SLICES = {1: (0, 2), 2: (5, 7), 3: (10, 12, 14), 4: (17, 19, 21), 5: (24, 26, 28)}
VGG_WIDTH = {1: 64, 2: 128, 3: 256, 4: 512, 5: 512}


class VGGTrunk(PackedNet):
    """the thirteen 3 x 3 convolutions under the subclass's key template `KEY` (`{s}`: slice, `{i}`: torchvision index)"""
    KEY = ""

    def _conv_names(self):
        return [self.KEY.format(s=s, i=i) for s, idx in VGG_SLICES.items() for i in idx]

    def _add_convs(self) -> None:
        c_in = 3
        for s, idx in VGG_SLICES.items():
            for i in idx:
                add_submodule(self, self.KEY.format(s=s, i=i), Conv(VGG_WIDTH[s], c_in, 3, 3))
                c_in = VGG_WIDTH[s]

    def _reset_convs(self, g) -> None:
        """Kaiming-normal weights, small biases"""
        for name in self._conv_names():
            m = self.get_submodule(name)
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / (9 * m.weight.shape[1])))
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)

    def _read_weights(self, weights, extra, no_extra: str) -> dict:
        """the state dict of `weights` merged with `extra`'s; torchvision's VGG-16 (`features.{idx}.weight|bias`, its `classifier.*`
        dropped) is renamed to the own keys and needs `extra`"""
        sd = read_state(weights)
        if any(k.startswith("features.") for k in sd):
            if extra is None:
                raise KeyError(no_extra)
            mapped = {}
            for k, v in sd.items():
                if k.startswith("classifier."):
                    continue
                parts = k.split(".")
                owner = next((s for s, idx in VGG_SLICES.items() if len(parts) == 3 and parts[1].isdigit() and int(parts[1]) in idx), None)
                mapped[k if owner is None else f"{self.KEY.format(s=owner, i=parts[1])}.{parts[2]}"] = v
            sd = mapped
        if extra is not None:
            sd.update(read_state(extra))
        return sd

    def _packed(self, dtype: torch.dtype):
        convs = [self.get_submodule(n) for n in self._conv_names()]
        return convs, self._cached(dtype, [m.weight for m in convs], lambda: [ops.pack_weight(m.weight, dtype) for m in convs])

    @staticmethod
    def chunk_pairs(h: int, w: int, dtype: torch.dtype) -> int:
        """pairs per launch so that the largest operand (conv1's output, 2 x pairs x h x w x 64) does not pass 2 GiB: the 32-bit
        buffer-offset rule of the implicit GEMM -- 64 pairs of 256 x 256 in f32"""
        es = 4 if dtype == torch.float32 else 2
        return max(1, (1 << 31) // (2 * h * w * 64 * es))

    def _check_pair(self, names, a: torch.Tensor, b: torch.Tensor):
        who, dev = type(self).__name__, self.get_submodule(self._conv_names()[0]).weight.device
        a32, b32 = check_images(who, names[0], a, dev), check_images(who, names[1], b, dev)
        if a.shape != b.shape:
            raise ValueError(f"{who}: {names[0]} {tuple(a.shape)} against {names[1]} {tuple(b.shape)}")
        return a32, b32

    @staticmethod
    def _stage(x: torch.Tensor, l: int, convs, packs) -> torch.Tensor:
        """stage l (from 0): its convs with the ReLU between them; the last output stays pre-activation (the tap kernels apply the ReLU on load)"""
        sizes = [len(idx) for idx in VGG_SLICES.values()]
        k0, k1 = sum(sizes[:l]), sum(sizes[:l + 1])
        for k in range(k0, k1):
            x = ops.conv2d(x, packs[k], convs[k].bias)
            if k + 1 < k1:
                ops.relu_(x)
        return x


# ---- the Inception conv stack of FID and Clean-FID ---------------------------------------------------------------------------------
def pack_conv(w: torch.Tensor, dtype: torch.dtype) -> ops.PackedWeight:
    """fp32 `[n_out, c_in, kh, kw]` on the device -> the packed weight `conv` reads: a 1 x 1 or 3 x 3 kernel as the implicit GEMM takes
    it, any other as the 1 x 1 weight `[n_out, kh kw c_in]` over the unfolded map (tap-major, then channel)"""
    kh, kw = w.shape[2:]
    if kh == kw and kh in (1, 3):
        return ops.pack_weight(w, dtype)
    return ops.pack_weight(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous(), dtype)


def conv(x: torch.Tensor, pw: ops.PackedWeight, bias, k, stride: int = 1, pad=(0, 0)) -> torch.Tensor:
    """the pre-activation convolution of NHWC `x`: 1 x 1 and 3 x 3 straight through `ops.conv2d`, every other kernel (stride 1, padding
    that keeps the size) as `ops.inception_unfold` and a 1 x 1 convolution"""
    kh, kw = k
    if kh == kw and kh in (1, 3):
        return ops.conv2d(x, pw, bias, stride=stride, pad=pad[0])
    assert stride == 1 and tuple(pad) == (kh // 2, kw // 2)
    return ops.conv2d(ops.inception_unfold(x, kh, kw), pw, bias, pad=0)


class InceptionStack(PackedNet):
    """BasicConv2d layers (conv without bias + BatchNorm) under torch-fidelity's `pt_inception` key names, from the subclass's table
    `LAYERS`: rows `(name, c_in, c_out, (kh, kw), stride, (pad_h, pad_w))`.  `IGNORED`: key prefixes of a published file that are not read."""
    LAYERS = ()
    IGNORED = ()

    def __init__(self, dtype: torch.dtype):
        super().__init__(dtype)
        for name, c_in, c_out, k, _, _ in self.LAYERS:
            add_submodule(self, name, BasicConv(c_in, c_out, k))

    def _layers(self):
        return [(row[0], self.get_submodule(row[0])) for row in self.LAYERS]

    def reset_parameters(self, seed: Optional[int] = None):
        """Kaiming-normal convs, BatchNorm close to the identity"""
        g = None if seed is None else torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for _, m in self._layers():
                w = m.conv.weight
                w.copy_(torch.randn(w.shape, generator=g) * math.sqrt(2.0 / (w.shape[1] * w.shape[2] * w.shape[3])))
                m.bn.weight.copy_(0.5 + torch.rand(m.bn.weight.shape, generator=g))
                m.bn.bias.copy_(0.1 * torch.randn(m.bn.bias.shape, generator=g))
                m.bn.running_mean.copy_(0.1 * torch.randn(m.bn.running_mean.shape, generator=g))
                m.bn.running_var.copy_(0.5 + torch.rand(m.bn.running_var.shape, generator=g))
        self._packs.clear()

    def load_weights(self, weights):
        """`weights`: a state dict or the path of one (read with `torch.load(weights_only=True)`): torch-fidelity's `pt_inception`
        (`Conv2d_1a_3x3.conv.weight`, `.bn.{weight,bias,running_mean,running_var}`, ...) or the same keys under `inception.`, as a
        torchmetrics FID state dict has them.  Ignored: `num_batches_tracked` and the `IGNORED` prefixes.  Anything else, or a missing key,
        raises a KeyError that names it; a wrong shape or a non-positive `running_var + 1e-3` a ValueError.  A refused file changes nothing."""
        sd = read_state(weights)
        if any(k.startswith("inception.") for k in sd):
            sd = {(k[len("inception."):] if k.startswith("inception.") else k): v for k, v in sd.items()}

        def check(read):
            for k, v in read.items():
                if k.endswith("running_var") and not bool((v.detach().double() + BN_EPS > 0).all()):
                    raise ValueError(f"{type(self).__name__}.load_weights: {k} + {BN_EPS} is not positive everywhere; BatchNorm divides by its root")

        load_state(self, sd, ignored=lambda k: k.endswith("num_batches_tracked") or k.startswith(self.IGNORED), check=check)
        self._packs.clear()
        return self

    def _packed(self, dtype: torch.dtype) -> dict:
        """name -> (packed weight, fp32 bias) with BatchNorm folded in, in fp64 on the host"""
        layers = self._layers()
        dev = layers[0][1].conv.weight.device

        def build():
            folded = {name: fold_batchnorm(m.conv, m.bn, BN_EPS, f"{type(self).__name__}: {name}.bn") for name, m in layers}
            return {name: (pack_conv(w.to(dev), dtype), b.to(dev)) for name, (w, b) in folded.items()}

        sources = [t for _, m in layers for t in (m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var)]
        return self._cached(dtype, sources, build)


# ---- the running statistics of a Frechet distance -----------------------------------------------------------------------------------
class FrechetStats(nn.Module):
    """the two running states (count, sum f, sum f^T f; fp64) and the solves' record `info` on the device, the sample counts on the host
    too, so `compute()` can refuse without a synchronisation.  The subclass brings `_solve(out, ...)`."""

    def _init_stats(self, width: int, device=None) -> None:
        for name, size in (("real_state", ops.frechet_state_size(width)), ("fake_state", ops.frechet_state_size(width)), ("info", ops.FID_INFO)):
            self.register_buffer(name, torch.zeros(size, dtype=torch.float64, device=device), persistent=False)
        self._n = {True: 0, False: 0}

    def _apply(self, fn, *args, **kw):
        out = super()._apply(fn, *args, **kw)
        for name in ("real_state", "fake_state", "info"):      # the statistics stay fp64 whatever the module is cast to
            if self._buffers[name].dtype != torch.float64:
                self._buffers[name] = self._buffers[name].double()
        return out

    @torch.no_grad()
    def compute(self, *, out: Optional[torch.Tensor] = None, **buffers) -> torch.Tensor:
        """the 0-d fp32 score on the device.  Raises the package's RuntimeError below 2 samples on a side (host counters: no
        synchronisation).  `self.info` then holds the solves' record."""
        if self._n[True] < 2 or self._n[False] < 2:
            raise RuntimeError("More than one sample is required for both the real and fake distributed to compute FID")
        out = torch.empty((), dtype=torch.float32, device=self.real_state.device) if out is None else out
        self._solve(out, **buffers)
        return out.view(())

    def reset(self) -> None:
        """both sides empty again (stream-ordered fills of the two states)"""
        self.real_state.zero_()
        self.fake_state.zero_()
        self._n = {True: 0, False: 0}
