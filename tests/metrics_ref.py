"""The expectation of the image-metric tests: compute_psnr / compute_ssim (src/evaluation/metrics.py:17-24, 58-73) restated in fp64
torch.  A helper module like tests/torch_optimizer_ops.py: imported by tests/test_metrics_cpu.py (which pins it against
scipy.ndimage.gaussian_filter) and tests/test_hip_metrics.py (which holds the kernel to it).

SSIM is skimage.metrics.structural_similarity(win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0): per channel a
Gaussian filter f (sigma 1.5, truncate 3.5 -> radius 5, 11 normalised taps, separable), ux = f(x), vx = n (f(x^2) - ux^2), ...,
S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), mean over the map cropped by 5 pixels per side, mean over
channels.  The crop removes every output the filter's border mode touches, so f is a VALID 11 x 11 convolution here."""
import math

import torch
import torch.nn.functional as F

WIN, SIGMA, C1, C2 = 11, 1.5, 1e-4, 9e-4


def gaussian_taps(dtype=torch.float64) -> torch.Tensor:
    r = WIN // 2
    g = torch.tensor([math.exp(-0.5 * (k - r) ** 2 / SIGMA ** 2) for k in range(WIN)], dtype=torch.float64)
    return (g / g.sum()).to(dtype)


def _filter(x: torch.Tensor) -> torch.Tensor:
    """valid separable Gaussian of [n, 1, h, w]"""
    g = gaussian_taps(x.dtype).to(x.device)
    return F.conv2d(F.conv2d(x, g.view(1, 1, 1, WIN)), g.view(1, 1, WIN, 1))


def ssim_map(gt: torch.Tensor, pred: torch.Tensor, use_sample_covariance: bool = True) -> torch.Tensor:
    """[b, c, h, w] -> S on the cropped map, [b, c, h - 10, w - 10], fp64"""
    b, c, h, w = gt.shape
    x = gt.double().reshape(b * c, 1, h, w)
    y = pred.double().reshape(b * c, 1, h, w)
    n = WIN * WIN / (WIN * WIN - 1.0) if use_sample_covariance else 1.0
    ux, uy = _filter(x), _filter(y)
    vx, vy, vxy = n * (_filter(x * x) - ux * ux), n * (_filter(y * y) - uy * uy), n * (_filter(x * y) - ux * uy)
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return s.reshape(b, c, h - WIN + 1, w - WIN + 1)


def compute_ssim(gt: torch.Tensor, pred: torch.Tensor, use_sample_covariance: bool = True) -> torch.Tensor:
    return ssim_map(gt, pred, use_sample_covariance).mean(dim=(2, 3)).mean(dim=1)


def compute_psnr(gt: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
    d = gt.double().clip(0, 1) - pred.double().clip(0, 1)
    return -10 * (d * d).mean(dim=(1, 2, 3)).log10()


# ---- inputs of the parity tests (seeded, built on the CPU) ---------------------------------------------------------
def smooth(n, c, h, w, g) -> torch.Tensor:
    """a low-frequency image in [0.2, 0.8]: bilinear upsampling of a coarse random grid"""
    coarse = torch.rand(n, c, max(2, h // 8 + 1), max(2, w // 8 + 1), generator=g, dtype=torch.float64)
    return 0.2 + 0.6 * F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True)


def make_pair(kind: str, n: int, c: int, h: int, w: int, seed: int = 0):
    """(gt, pred) float32 [n, c, h, w] of the kinds the parity test names"""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda: torch.rand(n, c, h, w, generator=g, dtype=torch.float64)
    if kind == "random":
        a, b = rnd(), rnd()
    elif kind in ("noise05", "noise002"):
        a = smooth(n, c, h, w, g)
        b = a + torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * (0.05 if kind == "noise05" else 0.002)
    elif kind == "zeros_ones":
        a, b = torch.zeros(n, c, h, w, dtype=torch.float64), torch.ones(n, c, h, w, dtype=torch.float64)
    elif kind == "out_of_range":                 # values in [-0.5, 1.5]: the PSNR clips them, the SSIM does not
        a, b = rnd() * 2 - 0.5, rnd() * 2 - 0.5
    elif kind == "identical":
        a = rnd()
        b = a.clone()
    else:
        raise KeyError(kind)
    return a.float(), b.float()


KINDS = ("random", "noise05", "noise002", "zeros_ones", "out_of_range", "identical")
