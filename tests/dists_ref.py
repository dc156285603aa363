"""The expectation of the DISTS tests: `DISTS_pytorch.DISTS().forward(x, y)` (what src/evaluation/metrics.py:27-40 calls) restated in
fp64 torch with F.conv2d.  A helper module like tests/lpips_ref.py: imported by tests/test_dists_cpu.py, tests/test_hip_dists.py and
tests/golden/make_dists_bounds.py.

The package's arithmetic, from knowledge of the package ("parity unpinned"): the trunk input (x - mean) / std;
torchvision's vgg16.features cut after relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 with an L2pooling (sqrt(conv2d(f^2, g, stride 2,
padding 1, groups C) + 1e-12), g = outer((1,2,1),(1,2,1)) / 16) in place of every max-pool; six taps (the RAW x, then the five stages);
per channel S1 = (2 mx my + c1) / (mx^2 + my^2 + c1), S2 = (2 cov + c2) / (vx + vy + c2), c1 = c2 = 1e-6; score = 1 - sum_c (alpha_c S1_c
+ beta_c S2_c) / (sum alpha + sum beta).  `form="direct"` is the algebraically equal sum_c (alpha_c (1 - S1_c) + beta_c (1 - S2_c)) / W
the device computes, 1 - S1 = (mx - my)^2 / (mx^2 + my^2 + c1), 1 - S2 = (vx + vy - 2 cov) / (vx + vy + c2): exactly 0 for equal inputs.

No pretrained weights exist offline: `make_weights` draws a seeded set of the right shapes.  `dtype=torch.float32` runs the trunk in
fp32 and the statistics and the fold in fp64 from those maps; `emulate=<16-bit dtype>` also rounds the weights and every stored
activation (the trunk input, each conv's output, each L2 pool's output) to that type: the CPU models of the device paths."""
import math

import torch
import torch.nn.functional as F

import lpips_ref

STAGES = {1: (0, 2), 2: (5, 7), 3: (10, 12, 14), 4: (17, 19, 21), 5: (24, 26, 28)}
WIDTH = {1: 64, 2: 128, 3: 256, 4: 512, 5: 512}
POOLS = {2: 4, 3: 9, 4: 16, 5: 23}            # stage -> the index of its L2pooling
CHANNELS = (3, 64, 128, 256, 512, 512)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
C1 = C2 = 1e-6
KINDS = lpips_ref.KINDS                        # random, noise05, noise002, identical
KINDS_16BIT = ("random", "noise05")            # noise002 scores ~1e-5: the f16 emulation is off by 30-170 % there, no 16-bit case
make_pair = lpips_ref.make_pair


def hann_filter(c: int, dtype=torch.float64) -> torch.Tensor:
    a = torch.tensor([1.0, 2.0, 1.0], dtype=dtype)
    return (torch.outer(a, a) / 16.0).view(1, 1, 3, 3).repeat(c, 1, 1, 1)


def make_weights(seed: int = 4321) -> dict:
    """a full DISTS state dict (fp32, the package's key layout) of seeded random weights: Kaiming-normal convs, 0.05 N biases,
    alpha, beta = |N(0.1, 0.01)| as the package initialises them"""
    g = torch.Generator().manual_seed(seed)
    sd, c_in = {}, 3
    for s, idx in STAGES.items():
        for i in idx:
            sd[f"stage{s}.{i}.weight"] = (torch.randn(WIDTH[s], c_in, 3, 3, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (9 * c_in))).float()
            sd[f"stage{s}.{i}.bias"] = (0.05 * torch.randn(WIDTH[s], generator=g, dtype=torch.float64)).float()
            c_in = WIDTH[s]
    for k in ("alpha", "beta"):
        sd[k] = (0.1 + 0.01 * torch.randn(1, sum(CHANNELS), 1, 1, generator=g, dtype=torch.float64)).abs().float()
    sd["mean"] = torch.tensor(MEAN).view(1, 3, 1, 1)
    sd["std"] = torch.tensor(STD).view(1, 3, 1, 1)
    for s, i in POOLS.items():
        sd[f"stage{s}.{i}.filter"] = hann_filter(WIDTH[s - 1], torch.float32)
    return sd


def split_weights(sd: dict):
    """the same weights as the two published files: (torchvision VGG-16 `features.*` + `classifier.*`, the package's weights.pt)"""
    vgg = {f"features.{k.split('.')[1]}.{k.split('.')[2]}": v for k, v in sd.items() if k.startswith("stage") and not k.endswith("filter")}
    vgg["classifier.0.weight"], vgg["classifier.0.bias"] = torch.zeros(4, 4), torch.zeros(4)
    return vgg, {"alpha": sd["alpha"], "beta": sd["beta"]}


def l2pool(x: torch.Tensor) -> torch.Tensor:
    """NCHW [n, C, h, w] -> [n, C, ceil(h/2), ceil(w/2)] in x's dtype"""
    c = x.shape[1]
    return (F.conv2d(x * x, hann_filter(c, x.dtype), stride=2, padding=1, groups=c) + 1e-12).sqrt()


def five_sums(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """post-ReLU NCHW maps [n, C, h, w] x 2 -> fp64 [n, 5, C]: sum a, sum b, sum a^2, sum b^2, sum a b over the pixels"""
    a, b = a.double(), b.double()
    return torch.stack([a.sum((2, 3)), b.sum((2, 3)), (a * a).sum((2, 3)), (b * b).sum((2, 3)), (a * b).sum((2, 3))], dim=1)


def features(x: torch.Tensor, sd: dict, dtype=torch.float64, emulate=None):
    """[m, 3, h, w] -> the six post-ReLU taps, NCHW; tap 0 is the raw input in fp64"""
    if emulate is not None:
        dtype = torch.float32
    rnd = (lambda t: t.to(emulate).to(dtype)) if emulate is not None else (lambda t: t)
    taps = [x.double()]
    f = rnd((x.to(dtype) - torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1))
    for s, idx in STAGES.items():
        if s > 1:
            f = rnd(l2pool(f))
        for j, i in enumerate(idx):
            f = rnd(F.conv2d(f, rnd(sd[f"stage{s}.{i}.weight"].to(dtype)), sd[f"stage{s}.{i}.bias"].to(dtype), padding=1)).relu()
        taps.append(f)
    return taps


def score(taps_x, taps_y, alpha: torch.Tensor, beta: torch.Tensor, form: str = "package") -> torch.Tensor:
    """the six taps of both inputs -> [n] fp64; the statistics two-pass as the package computes them (mean((f - m)^2), mean(fx fy) - mx my)"""
    alpha, beta = alpha.double().view(-1), beta.double().view(-1)
    wsum = alpha.sum() + beta.sum()
    n = taps_x[0].shape[0]
    total, c0 = torch.zeros(n, dtype=torch.float64), 0
    for fx, fy in zip(taps_x, taps_y):
        fx, fy = fx.double(), fy.double()
        c = fx.shape[1]
        a, b = alpha[c0:c0 + c], beta[c0:c0 + c]
        mx, my = fx.mean((2, 3), keepdim=True), fy.mean((2, 3), keepdim=True)
        vx, vy = ((fx - mx) ** 2).mean((2, 3)), ((fy - my) ** 2).mean((2, 3))
        cov = (fx * fy).mean((2, 3)) - (mx * my).flatten(1)
        mx, my = mx.flatten(1), my.flatten(1)
        if form == "package":
            s1 = (2 * mx * my + C1) / (mx ** 2 + my ** 2 + C1)
            s2 = (2 * cov + C2) / (vx + vy + C2)
            total = total + ((a * s1).sum(1) + (b * s2).sum(1)) / wsum
        else:
            d1 = (mx - my) ** 2 / (mx ** 2 + my ** 2 + C1)
            dc = (fx - mx.view(n, c, 1, 1)) - (fy - my.view(n, c, 1, 1))              # vx + vy - 2 cov = mean(((fx - mx) - (fy - my))^2):
            d2 = (dc ** 2).mean((2, 3)) / (vx + vy + C2)                                # no cancellation, exactly 0 for equal maps
            total = total + ((a * d1).sum(1) + (b * d2).sum(1)) / wsum
        c0 += c
    return 1 - total if form == "package" else total


def dists(x: torch.Tensor, y: torch.Tensor, sd: dict, dtype=torch.float64, emulate=None, form=None) -> torch.Tensor:
    """[n, 3, h, w] x 2 in [0, 1] -> [n] fp64.  fp64 without `form`: the package's `1 - sum` form, the reference.  The emulations
    (dtype=float32 / emulate=...) take the direct form, as the device does."""
    if form is None:
        form = "package" if (dtype == torch.float64 and emulate is None) else "direct"
    n = x.shape[0]
    taps = features(torch.cat([x, y]), sd, dtype, emulate)
    return score([t[:n] for t in taps], [t[n:] for t in taps], sd["alpha"], sd["beta"], form)


# ---- the cases of the whole-metric parity test (tests/test_hip_dists.py) and of the CPU bounds (tests/golden/make_dists_bounds.py) ----
# 5 x 7: maps of 5x7, 3x4, 2x2, 1x1, 1x1 (the last two taps have zero variance); 37 x 45: odd or ragged at every level (19x23, 10x12,
# 5x6, 3x3); 256 x 256: the sampler's resolution
CASES = [(n, h, w) for (h, w) in ((5, 7), (16, 16), (37, 45), (64, 64)) for n in (1, 3)] + [(2, 256, 256)]
WEIGHT_SEED = 4321


def case_seed(n: int, h: int, w: int) -> int:
    return h * 1000 + w + 7 * n


def case_key(kind: str, n: int, h: int, w: int) -> str:
    return f"{kind}/{n}x3x{h}x{w}"
