"""The expectation of the LPIPS tests: `lpips.LPIPS(net="vgg").forward(in0, in1, normalize)` (what src/evaluation/metrics.py:43-54
calls) restated in fp64 torch with F.conv2d / F.max_pool2d.  A helper module like tests/metrics_ref.py: imported by
tests/test_lpips_cpu.py, tests/test_hip_lpips.py and tests/golden/make_lpips_bounds.py.

The package's arithmetic, from knowledge of the package ("parity unpinned"): ScalingLayer (x - shift) / scale after the
optional 2x - 1; torchvision's vgg16.features cut after relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (a 2x2 max-pool opens slices
2..5); per tap normalize_tensor f / (sqrt(sum_c f^2) + 1e-10), the squared difference, a 1x1 `lin` conv without bias, the spatial
mean; the five taps summed.

No pretrained weights exist offline: `make_weights` draws a seeded set of the right shapes (Kaiming-normal convs, small biases,
non-negative `lin` weights as the published ones are).  `emulate=<16-bit dtype>` rounds the weights and every stored activation (the
ScalingLayer's output, each conv's output) to that type and computes in fp32: the CPU model of the 16-bit device path."""
import math

import torch
import torch.nn.functional as F

SLICES = {1: (0, 2), 2: (5, 7), 3: (10, 12, 14), 4: (17, 19, 21), 5: (24, 26, 28)}
WIDTH = {1: 64, 2: 128, 3: 256, 4: 512, 5: 512}
SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
EPS = 1e-10
KINDS = ("random", "noise05", "noise002", "identical")
KINDS_16BIT = ("random", "noise05")          # noise002 scores ~1e-6: a bf16 emulation is off by ~100 % there, no 16-bit case


def make_weights(seed: int = 1234) -> dict:
    """a full LPIPS state dict (fp32, the package's key layout) of seeded random weights"""
    g = torch.Generator().manual_seed(seed)
    sd, c_in = {}, 3
    for s, idx in SLICES.items():
        for i in idx:
            sd[f"net.slice{s}.{i}.weight"] = (torch.randn(WIDTH[s], c_in, 3, 3, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (9 * c_in))).float()
            sd[f"net.slice{s}.{i}.bias"] = (0.05 * torch.randn(WIDTH[s], generator=g, dtype=torch.float64)).float()
            c_in = WIDTH[s]
    for k in range(5):
        sd[f"lin{k}.model.1.weight"] = (0.02 * torch.rand(1, WIDTH[k + 1], 1, 1, generator=g, dtype=torch.float64)).float()
    sd["scaling_layer.shift"] = torch.tensor(SHIFT).view(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(SCALE).view(1, 3, 1, 1)
    return sd


def split_weights(sd: dict):
    """the same weights as the two published files: (torchvision VGG-16 `features.*` + `classifier.*`, the package's vgg.pth `lin*`)"""
    vgg = {f"features.{k.split('.')[2]}.{k.split('.')[3]}": v for k, v in sd.items() if k.startswith("net.")}
    vgg["classifier.0.weight"], vgg["classifier.0.bias"] = torch.zeros(4, 4), torch.zeros(4)
    lin = {k: v for k, v in sd.items() if k.startswith("lin")}
    return vgg, lin


def tap_distance(fa: torch.Tensor, fb: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """pre-activation NCHW maps [n, C, h, w] x 2, lin weight [C] -> per-image SUM over pixels of the distance, in the maps' dtype"""
    a, b = fa.relu(), fb.relu()
    na = a.pow(2).sum(dim=1, keepdim=True).sqrt()
    nb = b.pow(2).sum(dim=1, keepdim=True).sqrt()
    d = (a / (na + EPS) - b / (nb + EPS)).pow(2) * w.view(1, -1, 1, 1).to(a.dtype)
    return d.sum(dim=(1, 2, 3))


def lpips(in0: torch.Tensor, in1: torch.Tensor, sd: dict, normalize: bool = False, dtype=torch.float64, emulate=None, stats=None) -> torch.Tensor:
    """[n, 3, h, w] x 2 -> [n] in `dtype` (fp64: the reference; fp32: the summation-order emulation).  `stats`: a dict that
    receives "min_norm", the smallest channel norm at any tap pixel of either image (the conditioning of the normalisation)."""
    if emulate is not None:
        dtype = torch.float32
    rnd = (lambda t: t.to(emulate).to(dtype)) if emulate is not None else (lambda t: t)
    n = in0.shape[0]
    x = torch.cat([in0, in1]).to(dtype)
    if normalize:
        x = 2 * x - 1
    x = rnd((x - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1))
    total = torch.zeros(n, dtype=dtype)
    min_norm = float("inf")
    for l, (s, idx) in enumerate(SLICES.items()):
        if l:
            x = F.max_pool2d(x, 2)
        for j, i in enumerate(idx):
            if j:
                x = x.relu()
            x = rnd(F.conv2d(x, rnd(sd[f"net.slice{s}.{i}.weight"].to(dtype)), sd[f"net.slice{s}.{i}.bias"].to(dtype), padding=1))
        total = total + tap_distance(x[:n], x[n:], sd[f"lin{l}.model.1.weight"].to(dtype).view(-1)) / (x.shape[2] * x.shape[3])
        min_norm = min(min_norm, float(x.relu().pow(2).sum(dim=1).sqrt().min()))
        x = x.relu()
    if stats is not None:
        stats["min_norm"] = min(min_norm, stats.get("min_norm", float("inf")))
    return total


def make_pair(kind: str, n: int, h: int, w: int, seed: int = 0):
    """(gt, pred) float32 [n, 3, h, w] in (about) [0, 1]: uniform ground truth; the prediction independent, or the truth plus noise"""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda: torch.rand(n, 3, h, w, generator=g, dtype=torch.float64)
    if kind == "random":
        a, b = rnd(), rnd()
    elif kind in ("noise05", "noise002"):
        a = rnd()                # (a smooth ground truth has grey pixels whose 64 first-tap channels nearly vanish: badly conditioned)
        b = a + torch.randn(n, 3, h, w, generator=g, dtype=torch.float64) * (0.05 if kind == "noise05" else 0.002)
    elif kind == "identical":
        a = rnd()
        b = a.clone()
    else:
        raise KeyError(kind)
    return a.float(), b.float()


# ---- the cases of the whole-metric parity test (tests/test_hip_lpips.py) and of the CPU bounds (tests/golden/make_lpips_bounds.py) ----
# 16 x 16: 1 x 1 at conv5; 37 x 45: odd at every level (18 x 22, 9 x 11, 4 x 5, 2 x 2); 256 x 256: the sampler's resolution
CASES = [(n, h, w) for (h, w) in ((16, 16), (37, 45), (64, 64)) for n in (1, 3)] + [(2, 256, 256)]
WEIGHT_SEED = 1234


def case_seed(n: int, h: int, w: int) -> int:
    return h * 1000 + w + 7 * n


def case_key(kind: str, n: int, h: int, w: int) -> str:
    return f"{kind}/{n}x3x{h}x{w}"
