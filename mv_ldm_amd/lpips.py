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

from typing import Optional

import torch
from torch import nn

from . import ops
from ._metric_nets import VGG_SLICES, VGG_WIDTH, Conv, VGGTrunk, load_state      # noqa: F401  (the slice table and widths stay importable from here)

SHIFT = (-0.030, -0.088, -0.188)          # the package's ScalingLayer
SCALE = (0.458, 0.448, 0.450)


class _Lin(nn.Module):
    """`NetLinLayer`: model = [Dropout, Conv2d(C, 1, 1, bias=False)] -- key `model.1.weight`"""

    def __init__(self, c: int):
        super().__init__()
        self.model = nn.ModuleDict({"1": Conv(1, c, 1, 1, bias=False)})


class _Scaling(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT).view(1, 3, 1, 1))
        self.register_buffer("scale", torch.tensor(SCALE).view(1, 3, 1, 1))


class LPIPS(VGGTrunk):
    """`LPIPS(net="vgg")`; fp32 parameters under the package's key names (`net.slice{1..5}.{idx}.weight|bias`,
    `lin{0..4}.model.1.weight`, buffers `scaling_layer.shift|scale`).  `dtype`: the compute dtype of the activations and packed
    weights (float32 by default: a metric; float16 / bfloat16 are allowed).  `weights` / `lin`: see `load_weights`; without them the
    module keeps a random init and says so."""
    KEY = "net.slice{s}.{i}"

    def __init__(self, net: str = "vgg", weights=None, lin=None, dtype: torch.dtype = torch.float32, allow_random_init: bool = False):
        if net != "vgg":
            raise NotImplementedError(f"LPIPS(net={net!r}): only the VGG-16 variant the reference scores with is built")
        super().__init__(dtype)
        self.scaling_layer = _Scaling()
        self._add_convs()
        for k in range(5):
            setattr(self, f"lin{k}", _Lin(VGG_WIDTH[k + 1]))
        self._init_weights(weights, allow_random_init, lin)

    def reset_parameters(self, seed: Optional[int] = None):
        """Kaiming-normal convs, small biases, small non-negative `lin` weights (the published ones are non-negative)"""
        g = None if seed is None else torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self._reset_convs(g)
            for k in range(5):
                wt = self.get_submodule(f"lin{k}.model.1").weight
                wt.copy_(torch.rand(wt.shape, generator=g) * 0.02)
        self._packs.clear()

    def load_weights(self, weights, lin=None) -> "LPIPS":
        """`weights`: a state dict or the path of one (read with `torch.load(weights_only=True)`), either
          * a full `lpips.LPIPS(net="vgg").state_dict()` (`net.slice*`, `lin*`, `scaling_layer.*`; the `lins.{k}.*` duplicates of the
            package's ModuleList are accepted and ignored), or
          * torchvision's VGG-16 (`features.{idx}.weight|bias`; its `classifier.*` is not part of LPIPS and is ignored) together with
            `lin`: the package's `weights/v0.1/vgg.pth` (`lin{k}.model.1.weight`).
        Missing and unexpected keys raise a KeyError that names them.  `scaling_layer.*` is optional, and a file whose values are not
        the package's is refused: the kernel carries them."""
        sd = self._read_weights(weights, lin, "a torchvision VGG-16 state dict holds no `lin` layers: pass the lpips package's vgg.pth as `lin`")
        constants = {"scaling_layer.shift": torch.tensor(SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(SCALE).view(1, 3, 1, 1)}
        load_state(self, sd, ignored=lambda k: k.startswith("lins."), constants=constants, source="the lpips package's ScalingLayer")
        self._packs.clear()
        return self

    @torch.no_grad()
    def forward(self, in0: torch.Tensor, in1: torch.Tensor, normalize: bool = False, *, dtype: Optional[torch.dtype] = None,
                out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`[n, 3, h, w]` x 2 -> `[n, 1, 1, 1]` fp32 on the device.  `normalize`: the inputs are in [0, 1] (mapped to [-1, 1] first).
        `out` (fp32, n elements) and `ws` (uint8, at least `ops.lpips_workspace_bytes` of one chunk) let a captured graph own its buffers."""
        in0, in1 = self._check_pair(("in0", "in1"), in0, in1)
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
            slot0 = 0
            for l in range(5):
                x = ops.lpips_tap(self._stage(x, l, convs, packs), lins[l], ws, slot0, sum(slots), pool=l < 4)
                slot0 += slots[l]
            ops.lpips_fold(ws, m, h, w, flat[i0:i0 + m])
        return out.view(n, 1, 1, 1)
