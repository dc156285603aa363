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

from typing import Optional

import torch
from torch import nn

from . import ops
from ._metric_nets import VGG_SLICES as VGG_STAGES, VGG_WIDTH, VGGTrunk, load_state      # noqa: F401  (the stage table stays importable from here)

L2POOLS = {2: 4, 3: 9, 4: 16, 5: 23}          # stage -> index of the L2pooling that opens it (its `filter` buffer is a constant here)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
N_CHANNELS = sum(ops.DISTS_CHANNELS)          # 1475


def _constants() -> dict:
    """the package's buffers the kernels carry as constants: optional in a file, and a file that disagrees is another metric"""
    hann = torch.tensor([1.0, 2.0, 1.0])
    g = torch.outer(hann, hann) / 16.0
    out = {"mean": torch.tensor(MEAN).view(1, 3, 1, 1), "std": torch.tensor(STD).view(1, 3, 1, 1)}
    for s, i in L2POOLS.items():
        out[f"stage{s}.{i}.filter"] = g.view(1, 1, 3, 3).repeat(VGG_WIDTH[s - 1], 1, 1, 1)
    return out


class DISTS(VGGTrunk):
    """`DISTS_pytorch.DISTS()`; fp32 parameters under the package's key names (`stage1.{0,2}`, `stage2.{5,7}`, `stage3.{10,12,14}`,
    `stage4.{17,19,21}`, `stage5.{24,26,28}`, each `.weight|.bias`, and `alpha`, `beta` `[1, 1475, 1, 1]`).  `dtype`: the compute dtype
    of the activations and packed weights (float32 by default: a metric; float16 / bfloat16 are allowed).  `weights` / `alpha_beta`:
    see `load_weights`; without them the module keeps a random init and says so."""
    KEY = "stage{s}.{i}"

    def __init__(self, weights=None, alpha_beta=None, dtype: torch.dtype = torch.float32, allow_random_init: bool = False):
        super().__init__(dtype)
        self._add_convs()
        self.alpha = nn.Parameter(torch.empty(1, N_CHANNELS, 1, 1), requires_grad=False)
        self.beta = nn.Parameter(torch.empty(1, N_CHANNELS, 1, 1), requires_grad=False)
        self._init_weights(weights, allow_random_init, alpha_beta)

    def reset_parameters(self, seed: Optional[int] = None):
        """Kaiming-normal convs, small biases, alpha and beta |N(0.1, 0.01)| as the package initialises them"""
        g = None if seed is None else torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self._reset_convs(g)
            for p in (self.alpha, self.beta):
                p.copy_((0.1 + 0.01 * torch.randn(p.shape, generator=g)).abs())
        self._packs.clear()

    def load_weights(self, weights, alpha_beta=None) -> "DISTS":
        """`weights`: a state dict or the path of one (read with `torch.load(weights_only=True)`), either
          * a full `DISTS_pytorch.DISTS().state_dict()` (`stage*`, `alpha`, `beta`; its `mean`, `std` and `stage{2..5}.{4,9,16,23}.filter`
            buffers are optional and must equal the package's constants within 1e-6), or
          * torchvision's VGG-16 (`features.{idx}.weight|bias`; its `classifier.*` is not part of DISTS and is ignored) together with
            `alpha_beta`: the package's `weights.pt` (`alpha`, `beta`).
        Missing and unexpected keys raise a KeyError that names them."""
        sd = self._read_weights(weights, alpha_beta,
                                "a torchvision VGG-16 state dict holds no `alpha` / `beta`: pass the DISTS_pytorch package's weights.pt as `alpha_beta`")

        def check(read):
            wsum = float(read["alpha"].detach().double().sum() + read["beta"].detach().double().sum())
            if not wsum > 0:
                raise ValueError(f"DISTS.load_weights: sum(alpha) + sum(beta) = {wsum}; the score divides by it")

        load_state(self, sd, constants=_constants(), check=check,
                   source="the DISTS_pytorch package's constant (mean / std of ImageNet, the 3x3 Hann filter)")
        self._packs.clear()
        return self

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
        x, y = self._check_pair(("x", "y"), x, y)
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
            for l in range(5):
                f = self._stage(f, l, convs, packs)
                ops.dists_stats(f, ws, taps[l + 1][3], stride)              # ReLU on load
                if l < 4:
                    f = ops.dists_l2pool(f)
            ops.dists_fold(ws, m, h, w, alpha, beta, flat[i0:i0 + m])
        return out.view(n)
