"""The expectation of the Clean-FID tests: `cleanfid.fid.compute_fid(dir1, dir2)` (mode "clean", Inception-v3; what
src/scripts/compute_fid.py:44-47 calls) restated in fp64 torch / numpy.  A helper module like tests/fid_ref.py: imported by
tests/test_cleanfid_cpu.py, tests/test_hip_cleanfid.py, tests/golden/make_cleanfid_golden.py and tests/golden/make_cleanfid_bounds.py.

The package's arithmetic, from knowledge of the package ("parity unpinned") -- except the resize, which is pinned against
PIL's own output (tests/golden/cleanfid_resize.npz): every channel through `PIL.Image.fromarray(x.astype(float32), mode="F").resize((299, 299),
BICUBIC)` (antialiased, separable, horizontally first, a pass whose size stays is skipped; coefficients and sums in double, rounded to
float32 after each pass), clip to [0, 255], (x - 128) / 128; the FID Inception-v3 (every BasicConv2d: conv(bias=False) -> BatchNorm(eps=1e-3,
eval) -> ReLU) up to the mean over its last 8 x 8 map: 2048 features in fp64.  mu = mean, Sigma = cov (divisor n - 1),
fid = |mu1 - mu2|^2 + tr Sigma1 + tr Sigma2 - 2 tr sqrtm(Sigma1 Sigma2).

No pretrained weights exist offline: `make_weights` draws a seeded set of the right shapes (21.8 M parameters, nothing committed).
`dtype=torch.float32` runs the network in fp32 and everything from the pooled mean on in fp64; `emulate=<16-bit dtype>` also rounds the
folded weights and every stored activation to that type: the CPU models of the device paths."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from fid_ref import (PAIRS, frechet_pkg, frechet_sym, make_images, make_sets, moments, scale, state, state_from_moments)      # noqa: F401  (shared with the feature=64 tests)

D = 2048
EPS = 1e-3
SIZE = 299
MAPS = ("stem", "Mixed_5d", "Mixed_6a", "Mixed_6e", "Mixed_7a", "Mixed_7c")


# ---- the front end ------------------------------------------------------------------------------------------------------------------
def _cubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=None)
def coefficients(n_in: int, n_out: int):
    """[(xmin, normalised double weights)] per output index: PIL's precompute_coeffs for the bicubic filter over the whole axis"""
    scl = float(n_in) / n_out
    fs = max(scl, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    out = []
    for i in range(n_out):
        center = (i + 0.5) * scl
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        k = [_cubic((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        out.append((xmin, k))
    return out


def _pass(x: np.ndarray, n_out: int) -> np.ndarray:
    """resample the LAST axis of the float32 array x: the sum over the taps in double, in tap order, rounded to float32"""
    n_in = x.shape[-1]
    if n_in == n_out:
        return x
    out = np.empty(x.shape[:-1] + (n_out,), dtype=np.float32)
    xd = x.astype(np.float64)
    for i, (xmin, k) in enumerate(coefficients(n_in, n_out)):
        acc = np.zeros(x.shape[:-1], dtype=np.float64)
        for j, kj in enumerate(k):
            acc = acc + xd[..., xmin + j] * kj
        out[..., i] = acc.astype(np.float32)
    return out


def resize_clean(x: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """float32 [..., h, w] -> float32 [..., oh, ow]: PIL's bicubic resize of each plane (before the clip)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x = _pass(x, ow)
    return np.swapaxes(_pass(np.swapaxes(x, -1, -2), oh), -1, -2)


def resize_pil(x: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """the same through PIL itself (CPU only; the goldens and the CPU test)"""
    from PIL import Image
    x = np.ascontiguousarray(x, dtype=np.float32)
    flat = x.reshape(-1, *x.shape[-2:])
    out = np.stack([np.asarray(Image.fromarray(p, mode="F").resize((ow, oh), resample=Image.BICUBIC)) for p in flat])
    return out.reshape(*x.shape[:-2], oh, ow)


def to_255(imgs: torch.Tensor) -> np.ndarray:
    """uint8, or float in [0, 1] (multiplied by 255 in fp32, not quantised) -> float32 numpy in [0, 255]"""
    if imgs.dtype == torch.uint8:
        return imgs.numpy().astype(np.float32)
    return (imgs.to(torch.float32) * torch.tensor(255.0, dtype=torch.float32)).numpy()


def prep(imgs: torch.Tensor, oh: int = SIZE, ow: int = SIZE) -> torch.Tensor:
    """[n, 3, h, w] -> the network's input [n, 3, oh, ow]: (v - 128) / 128 in fp32, as the package computes it on the float32 the resize
    leaves (the subtraction rounds), then exact in fp64"""
    v = np.clip(resize_clean(to_255(imgs), oh, ow), 0, 255)
    return ((torch.from_numpy(v) - 128) / 128).double()


def pattern(n: int, h: int, w: int) -> torch.Tensor:
    """tests/test_hip_fid.py:_pattern: uint8 [n, 3, h, w] whose horizontal and vertical neighbours always differ"""
    i, c, y, x = torch.meshgrid(torch.arange(n), torch.arange(3), torch.arange(h), torch.arange(w), indexing="ij")
    return ((37 * y + 101 * x + 59 * c + 83 * i) % 256).to(torch.uint8).contiguous()


RESIZE_CASES = [(13, 17, 29, 23), (64, 48, 29, 23), (31, 16, 16, 31), (16, 16, 16, 16)]      # h, w, oh, ow


def resize_inputs(h: int, w: int) -> torch.Tensor:
    """uint8 [4, 3, h, w]: two seeded noise images and two of the pattern"""
    g = torch.Generator().manual_seed(1000 * h + w)
    return torch.cat([torch.randint(0, 256, (2, 3, h, w), generator=g, dtype=torch.uint8), pattern(2, h, w)]).contiguous()


# ---- the network --------------------------------------------------------------------------------------------------------------------
def _layers():
    """[(name, c_in, c_out, (kh, kw), stride, (pad_h, pad_w))]: torchvision's Inception3 without AuxLogits and fc, in forward order"""
    out = []
    add = lambda name, c_in, c_out, k=(1, 1), stride=1, pad=(0, 0): out.append((name, c_in, c_out, k, stride, pad))
    add("Conv2d_1a_3x3", 3, 32, (3, 3), 2)
    add("Conv2d_2a_3x3", 32, 32, (3, 3))
    add("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1))
    add("Conv2d_3b_1x1", 64, 80)
    add("Conv2d_4a_3x3", 80, 192, (3, 3))
    for m, c_in, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        add(m + ".branch1x1", c_in, 64)
        add(m + ".branch5x5_1", c_in, 48)
        add(m + ".branch5x5_2", 48, 64, (5, 5), 1, (2, 2))
        add(m + ".branch3x3dbl_1", c_in, 64)
        add(m + ".branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1))
        add(m + ".branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1))
        add(m + ".branch_pool", c_in, pf)
    add("Mixed_6a.branch3x3", 288, 384, (3, 3), 2)
    add("Mixed_6a.branch3x3dbl_1", 288, 64)
    add("Mixed_6a.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1))
    add("Mixed_6a.branch3x3dbl_3", 96, 96, (3, 3), 2)
    for m, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        add(m + ".branch1x1", 768, 192)
        add(m + ".branch7x7_1", 768, c7)
        add(m + ".branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        add(m + ".branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        add(m + ".branch7x7dbl_1", 768, c7)
        add(m + ".branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        add(m + ".branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        add(m + ".branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        add(m + ".branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        add(m + ".branch_pool", 768, 192)
    add("Mixed_7a.branch3x3_1", 768, 192)
    add("Mixed_7a.branch3x3_2", 192, 320, (3, 3), 2)
    add("Mixed_7a.branch7x7x3_1", 768, 192)
    add("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    add("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    add("Mixed_7a.branch7x7x3_4", 192, 192, (3, 3), 2)
    for m, c_in in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        add(m + ".branch1x1", c_in, 320)
        add(m + ".branch3x3_1", c_in, 384)
        add(m + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        add(m + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        add(m + ".branch3x3dbl_1", c_in, 448)
        add(m + ".branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1))
        add(m + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        add(m + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        add(m + ".branch_pool", c_in, 192)
    return out


LAYERS = _layers()
SPEC = {name: (k, stride, pad) for name, _, _, k, stride, pad in LAYERS}
WEIGHT_SEED = 2048


@functools.lru_cache(maxsize=2)
def make_weights(seed: int = WEIGHT_SEED, prefix: str = "") -> dict:
    """torch-fidelity's `pt_inception` state dict (fp32) without fc / AuxLogits, of seeded random values: Kaiming-normal convs, BatchNorm
    gamma in [0.5, 1.5], beta 0.1 N, running_mean 0.1 N, running_var in [0.5, 1.5]"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, c_in, c_out, (kh, kw), _, _ in LAYERS:
        sd[f"{prefix}{name}.conv.weight"] = (torch.randn(c_out, c_in, kh, kw, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (kh * kw * c_in))).float()
        sd[f"{prefix}{name}.bn.weight"] = (0.5 + torch.rand(c_out, generator=g, dtype=torch.float64)).float()
        sd[f"{prefix}{name}.bn.bias"] = (0.1 * torch.randn(c_out, generator=g, dtype=torch.float64)).float()
        sd[f"{prefix}{name}.bn.running_mean"] = (0.1 * torch.randn(c_out, generator=g, dtype=torch.float64)).float()
        sd[f"{prefix}{name}.bn.running_var"] = (0.5 + torch.rand(c_out, generator=g, dtype=torch.float64)).float()
    return sd


def with_other_layers(sd: dict, prefix: str = "") -> dict:
    """the same file as the package ships it: with `num_batches_tracked`, the classifier and the auxiliary head"""
    out = {prefix + k: v for k, v in sd.items()}
    for name, *_ in LAYERS[:3]:
        out[f"{prefix}{name}.bn.num_batches_tracked"] = torch.tensor(7)
    for k in ("AuxLogits.conv0.conv.weight", "AuxLogits.fc.weight", "fc.weight", "fc.bias"):
        out[prefix + k] = torch.zeros(2, 2)
    return out


def fold_bn(sd: dict, name: str):
    """(w', b') in fp64: w' = w gamma / sqrt(var + eps), b' = beta - mean gamma / sqrt(var + eps)"""
    g = sd[f"{name}.bn.weight"].double() / (sd[f"{name}.bn.running_var"].double() + EPS).sqrt()
    return sd[f"{name}.conv.weight"].double() * g.view(-1, 1, 1, 1), sd[f"{name}.bn.bias"].double() - sd[f"{name}.bn.running_mean"].double() * g


def basic_conv(x: torch.Tensor, sd: dict, name: str, dtype=torch.float64, emulate=None) -> torch.Tensor:
    """one BasicConv2d on NCHW.  fp64: BatchNorm applied unfused.  The emulations run the folded convolution with its bias in fp32 and
    round what the device stores (weights, the output)."""
    _, stride, pad = SPEC[name]
    if dtype == torch.float64 and emulate is None:
        f = F.conv2d(x.double(), sd[f"{name}.conv.weight"].double(), None, stride=stride, padding=pad)
        v = lambda k: sd[f"{name}.bn.{k}"].double().view(1, -1, 1, 1)
        return ((f - v("running_mean")) / (v("running_var") + EPS).sqrt() * v("weight") + v("bias")).relu()
    rnd = (lambda t: t.to(emulate).float()) if emulate is not None else (lambda t: t)
    w, b = fold_bn(sd, name)
    return rnd(F.conv2d(x.float(), rnd(w.float()), b.float(), stride=stride, padding=pad)).relu()


def network(x: torch.Tensor, sd: dict, dtype=torch.float64, emulate=None, maps=()):
    """the network's input NCHW [n, 3, 299, 299] -> (the post-ReLU 8 x 8 x 2048 map, {name: post-ReLU map} for the names in `maps`)"""
    exact = dtype == torch.float64 and emulate is None
    rnd = (lambda t: t.to(emulate).float()) if emulate is not None else (lambda t: t)
    cv = lambda name, t: basic_conv(t, sd, name, dtype, emulate)
    avg = lambda t: rnd(F.avg_pool2d(t, 3, 1, 1, count_include_pad=False))
    keep = {}

    def tap(name, t):
        if name in maps:
            keep[name] = t
        return t

    x = x.double() if exact else rnd(x.float())
    x = cv("Conv2d_2b_3x3", cv("Conv2d_2a_3x3", cv("Conv2d_1a_3x3", x)))
    x = F.max_pool2d(x, 3, 2)
    x = cv("Conv2d_4a_3x3", cv("Conv2d_3b_1x1", x))
    x = tap("stem", F.max_pool2d(x, 3, 2))
    for m in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        b1 = cv(m + ".branch1x1", x)
        b5 = cv(m + ".branch5x5_2", cv(m + ".branch5x5_1", x))
        b3 = cv(m + ".branch3x3dbl_3", cv(m + ".branch3x3dbl_2", cv(m + ".branch3x3dbl_1", x)))
        x = tap(m, torch.cat([b1, b5, b3, cv(m + ".branch_pool", avg(x))], 1))
    b3 = cv("Mixed_6a.branch3x3", x)
    bd = cv("Mixed_6a.branch3x3dbl_3", cv("Mixed_6a.branch3x3dbl_2", cv("Mixed_6a.branch3x3dbl_1", x)))
    x = tap("Mixed_6a", torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1))
    for m in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        b1 = cv(m + ".branch1x1", x)
        b7 = cv(m + ".branch7x7_3", cv(m + ".branch7x7_2", cv(m + ".branch7x7_1", x)))
        bd = cv(m + ".branch7x7dbl_1", x)
        for j in (2, 3, 4, 5):
            bd = cv(f"{m}.branch7x7dbl_{j}", bd)
        x = tap(m, torch.cat([b1, b7, bd, cv(m + ".branch_pool", avg(x))], 1))
    b3 = cv("Mixed_7a.branch3x3_2", cv("Mixed_7a.branch3x3_1", x))
    b7 = cv("Mixed_7a.branch7x7x3_1", x)
    for j in (2, 3, 4):
        b7 = cv(f"Mixed_7a.branch7x7x3_{j}", b7)
    x = tap("Mixed_7a", torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1))
    for m in ("Mixed_7b", "Mixed_7c"):
        b1 = cv(m + ".branch1x1", x)
        b3 = cv(m + ".branch3x3_1", x)
        b3 = torch.cat([cv(m + ".branch3x3_2a", b3), cv(m + ".branch3x3_2b", b3)], 1)
        bd = cv(m + ".branch3x3dbl_2", cv(m + ".branch3x3dbl_1", x))
        bd = torch.cat([cv(m + ".branch3x3dbl_3a", bd), cv(m + ".branch3x3dbl_3b", bd)], 1)
        pooled = avg(x) if m == "Mixed_7b" else F.max_pool2d(x, 3, 1, 1)
        x = tap(m, torch.cat([b1, b3, bd, cv(m + ".branch_pool", pooled)], 1))
    return x, keep


def features(imgs: torch.Tensor, sd: dict, dtype=torch.float64, emulate=None, maps=(), chunk: int = 2):
    """uint8 / float [0, 1] images [n, 3, h, w] -> fp64 [n, 2048] (and {name: NCHW map} when `maps` names some)"""
    out, kept = [], {m: [] for m in maps}
    with torch.no_grad():
        for i in range(0, imgs.shape[0], chunk):
            f, keep = network(prep(imgs[i:i + chunk]), sd, dtype, emulate, maps)
            out.append(f.double().mean((2, 3)))
            for k, v in keep.items():
                kept[k].append(v)
    f = torch.cat(out)
    return (f, {k: torch.cat(v) for k, v in kept.items()}) if maps else f


# ---- the cases of the whole-extractor tests -----------------------------------------------------------------------------------------
CASES = [(3, 3, 64, 48), (2, 2, 299, 299)]         # n_real, n_fake, h, w


def case_seed(n_real: int, n_fake: int, h: int, w: int) -> int:
    return h * 1000 + w + 7 * n_real + 13 * n_fake


def case_key(pair: str, n_real: int, n_fake: int, h: int, w: int) -> str:
    return f"{pair}/{n_real}+{n_fake}x3x{h}x{w}"


def case_sets(pair: str, n_real: int, n_fake: int, h: int, w: int):
    """(real, fake) as uint8 [n, 3, h, w]: fid_ref's sets, quantised -- the package's input is bytes"""
    real, fake = make_sets(pair, n_real, n_fake, h, w, seed=case_seed(n_real, n_fake, h, w))
    q = lambda t: (t * 255).round().to(torch.uint8).contiguous()
    return q(real), q(fake)


def map_sample(name: str, shape) -> torch.Tensor:
    """512 seeded flat positions of an NCHW map of `shape`: what tests/golden/cleanfid_features.npz keeps of each map"""
    g = torch.Generator().manual_seed(MAPS.index(name) + 77)
    return torch.randint(0, int(np.prod(shape)), (512,), generator=g)


# ---- the convolutions that run as unfold + 1 x 1 (tests/test_hip_cleanfid.py "unfold + conv") ---------------------------------------
CONV_KERNELS = [((1, 7), (0, 3)), ((7, 1), (3, 0)), ((1, 3), (0, 1)), ((3, 1), (1, 0)), ((5, 5), (2, 2))]
CONV_MAPS = {(1, 7): [(9, 11), (5, 4)], (7, 1): [(9, 11), (5, 4)], (1, 3): [(9, 11)], (3, 1): [(9, 11)], (5, 5): [(9, 11), (3, 3)]}
CONV_N, CONV_CIN, CONV_NOUT = 2, 16, 80


def conv_case(k, hw):
    """(x NCHW fp32 [2, 16, h, w], weight fp32 [80, 16, kh, kw], bias fp32 [80]) of one unit case, seeded"""
    g = torch.Generator().manual_seed(100 * k[0] + 10 * k[1] + hw[0] * 7 + hw[1])
    x = torch.randn(CONV_N, CONV_CIN, *hw, generator=g).relu()
    w = torch.randn(CONV_NOUT, CONV_CIN, *k, generator=g) * math.sqrt(2.0 / (k[0] * k[1] * CONV_CIN))
    return x, w, 0.1 * torch.randn(CONV_NOUT, generator=g)


def conv_want(x, w, b, pad, emulate=None, dtype=torch.float64):
    if dtype == torch.float64 and emulate is None:
        return F.conv2d(x.double(), w.double(), b.double(), padding=pad)
    rnd = (lambda t: t.to(emulate).float()) if emulate is not None else (lambda t: t)
    return rnd(F.conv2d(rnd(x.float()), rnd(w.float()), b.float(), padding=pad)).double()


# ---- the device's solve (csrc/inception.hip): one-sided Jacobi, the same ordering, the same formulas, in numpy fp64 ------------------
SWEEP_CAP = 30


def solve_tol(d: int) -> float:
    return math.sqrt(d) * 2.0 ** -52


def _round_pairs(d: int, r: int):
    k = np.arange(1, d // 2)
    a = np.concatenate([[d - 1], (r + k) % (d - 1)])
    b = np.concatenate([[r], (r - k + (d - 1)) % (d - 1)])
    return np.minimum(a, b), np.maximum(a, b)


def hestenes(a: np.ndarray, vectors: bool):
    """(G by columns as rows, V likewise or None, sweeps, last residual, converged): G = A V with orthogonal columns"""
    d = a.shape[0]
    g = np.array(a, dtype=np.float64).T.copy()          # g[p] = column p
    v = np.eye(d) if vectors else None
    tol, sw, res, done = solve_tol(d), 0, 0.0, False
    floor = tol * tol * float((g * g).sum())            # a pair of columns both at round-off level (|g_p| |g_q| <= tol^2 |A|_F^2) is left alone
    while not done and sw < SWEEP_CAP:
        res = 0.0
        for r in range(d - 1):
            p, q = _round_pairs(d, r)
            x, y = g[p], g[q]
            app, aqq, apq = (x * x).sum(1), (y * y).sum(1), (x * y).sum(1)
            den = np.sqrt(app) * np.sqrt(aqq)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                ratio = np.where(den > floor, np.abs(apq) / den, 0.0)
                res = max(res, float(ratio.max()))
                rot = ratio > tol
                zeta = (aqq - app) / (2.0 * apq)
                t = np.where(zeta >= 0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(zeta * zeta + 1.0))
            t = np.where(rot, t, 0.0)
            h = t * t
            rt = np.sqrt(h + 1.0)
            s, cm1 = ((1.0 / rt) * t)[:, None], (-h / (rt * (1.0 + rt)))[:, None]      # c - 1, and x + ((c - 1) x - s y): no stretch
            g[p], g[q] = x + (cm1 * x - s * y), y + (s * x + cm1 * y)
            if vectors:
                x, y = v[p], v[q]
                v[p], v[q] = x + (cm1 * x - s * y), y + (s * x + cm1 * y)
        sw += 1
        done = res <= tol
    return g, v, sw, res, done


def hestenes_emulation(st1, st2):
    """the device's route in numpy fp64: (fid, info) with info = [sweeps 1, residual 1, sweeps 2, residual 2, capped solves]"""
    (m1, s1), (m2, s2) = moments(st1), moments(st2)
    g, v, sw1, r1, ok1 = hestenes(s1, True)
    lam = (v * g).sum(1)
    sd = np.sqrt(np.maximum(lam, 0))
    t = v @ s2.T                                        # t[j] = Sigma2 v_j
    m = v @ t.T                                         # m[i][j] = v_i . t[j]
    s = sd[:, None] * (0.5 * (m + m.T)) * sd[None, :]
    g2, _, sw2, r2, ok2 = hestenes(s, False)
    c = np.sqrt(np.maximum(np.sqrt((g2 * g2).sum(1)), 0)).sum()
    fid = float(((m1 - m2) ** 2).sum() + (np.trace(s1) + np.trace(s2)) - 2 * c)
    return (fid if ok1 and ok2 else float("nan")), [sw1, r1, sw2, r2, int(not ok1) + int(not ok2)]


def frechet_factored(f1, f2) -> float:
    """The expectation of the whole-extractor tests, from the fp64 FEATURES [n, d] of the two sides: with Sigma_k = A_k^T A_k,
    A_k = (f_k - mu_k) / sqrt(n_k - 1), tr sqrt(Sigma1^1/2 Sigma2 Sigma1^1/2) is the sum of the singular values of the n1 x n2 matrix
    A1 A2^T -- the value of the symmetric form without its round-off.  `frechet_sym` (eigh twice on 2048 x 2048 matrices of rank n - 1)
    is NOT that: the 2040-odd null eigenvalues of Sigma1 come back as +- 1e-12 and add, under the square roots, 1.1e-6 of the scale on
    these very cases (3 + 3 and 2 + 2 images) -- more than the whole f32 bound; the device's solve, measured, sits 1e-9-class from the
    factored value and exactly that 1.1e-6 from `frechet_sym`."""
    f1, f2 = np.asarray(f1, dtype=np.float64), np.asarray(f2, dtype=np.float64)
    m1, m2 = f1.mean(0), f2.mean(0)
    a1, a2 = (f1 - m1) / math.sqrt(len(f1) - 1), (f2 - m2) / math.sqrt(len(f2) - 1)
    c = np.linalg.svd(a1 @ a2.T, compute_uv=False).sum()
    return float(((m1 - m2) ** 2).sum() + (a1 * a1).sum() + (a2 * a2).sum() - 2 * c)


def frechet_sqrtm(st1, st2) -> float:
    """the package's own route: scipy.linalg.sqrtm(Sigma1 Sigma2), the real part of its trace"""
    from scipy import linalg
    (m1, s1), (m2, s2) = moments(st1), moments(st2)
    covmean = linalg.sqrtm(s1.dot(s2))
    if isinstance(covmean, tuple):
        covmean = covmean[0]
    return float(((m1 - m2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2 * np.trace(np.real(covmean)))


# ---- synthetic states for the solve alone -------------------------------------------------------------------------------------------
def random_state(n: int, d: int, seed: int) -> torch.Tensor:
    """the state of n random non-negative feature vectors of width d (rank min(n - 1, d))"""
    f = torch.rand(n, d, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * torch.linspace(0.2, 2.0, d, dtype=torch.float64)
    return state(f)


def synthetic_cases(d: int) -> dict:
    """name -> (class, state 1, state 2, analytic sum sqrt or None) at width d.  `analytic`: Sigma1 = Q diag(a) Q^T, Sigma2 = Q diag(b) Q^T
    commute, so sum sqrt(eig(Sigma1 Sigma2)) = sum sqrt(a_i b_i); `deficient`: n < d samples a side; `identical`: the score is 0."""
    rng = np.random.default_rng(d)
    qm, _ = np.linalg.qr(rng.standard_normal((d, d)))
    a, b = rng.uniform(0.1, 2.0, d), rng.uniform(0.1, 2.0, d)
    mu1, mu2 = rng.uniform(0, 1, d), rng.uniform(0, 1, d)
    out = {"analytic": ("full", state_from_moments(mu1, (qm * a) @ qm.T, 4 * d), state_from_moments(mu2, (qm * b) @ qm.T, 4 * d), float(np.sqrt(a * b).sum())),
           "deficient": ("deficient", random_state(6, d, 11), random_state(6, d, 12), None)}
    if d <= 256:
        out["full"] = ("full", random_state(2 * d, d, 13), random_state(3 * d, d, 14), None)
        out["deficient_vs_full"] = ("deficient", random_state(5, d, 15), random_state(2 * d, d, 16), None)
        out["identical"] = ("identical", random_state(2 * d, d, 17), random_state(2 * d, d, 17), None)
        out["identical_deficient"] = ("identical", random_state(5, d, 18), random_state(5, d, 18), None)
    return out
