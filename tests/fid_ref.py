"""The expectation of the FID tests: torchmetrics' `FrechetInceptionDistance(feature=64, normalize=True)` (what
src/evaluation/metric_computer.py:22,65-68 builds and calls) restated in fp64 torch / numpy.  A helper module like tests/dists_ref.py:
imported by tests/test_fid_cpu.py, tests/test_hip_fid.py and tests/golden/make_fid_bounds.py.

The package's arithmetic, from knowledge of the package ("parity unpinned"): `(imgs * 255).byte()` (an fp32 product,
truncated); torch-fidelity's `interpolate_bilinear_2d_like_tensorflow1x(align_corners=False)` to 299 x 299 (source coordinate
float32(i) * float32(in / out), no half-pixel centres, the x lerp first); (x - 128) / 128; Conv2d_1a_3x3 (3 -> 32, stride 2), Conv2d_2a_3x3
(32 -> 32), Conv2d_2b_3x3 (32 -> 64, padding 1), each conv(bias=False) -> BatchNorm(eps=1e-3, eval) -> ReLU; MaxPool(3, 2); the mean over
the map: 64 features, cast to fp64.  Per side sum f, sum f^T f, n; mu = sum / n, Sigma = (sum f^T f - n mu^T mu) / (n - 1);
fid = |mu1 - mu2|^2 + tr Sigma1 + tr Sigma2 - 2 sum_i Re sqrt(eig_i(Sigma1 Sigma2)).

No pretrained weights exist offline: `make_weights` draws a seeded set of the right shapes.  `dtype=torch.float32` runs the stem in fp32
and everything from the pooled mean on in fp64; `emulate=<16-bit dtype>` also rounds the folded weights and every stored activation (the
stem's input, each conv's output) to that type: the CPU models of the device paths."""
import math

import numpy as np
import torch
import torch.nn.functional as F

D = 64
EPS = 1e-3
LAYERS = (("Conv2d_1a_3x3", 3, 32, 2, 0), ("Conv2d_2a_3x3", 32, 32, 1, 0), ("Conv2d_2b_3x3", 32, 64, 1, 1))   # name, c_in, c_out, stride, pad
SIZE = 299


# ---- the front end ------------------------------------------------------------------------------------------------------------------
def quantise(x: torch.Tensor) -> torch.Tensor:
    """fp32 [0, 1] -> the integer of `(x * 255).byte()` as fp64: the fp32 product, truncated toward zero"""
    return torch.trunc(x.to(torch.float32) * torch.tensor(255.0, dtype=torch.float32)).double()


def taps(n_in: int, n_out: int):
    """(lo, hi, d) of one axis: coordinates in fp32 as the package computes them; lo, hi int64, d fp32"""
    scale = np.float32(n_in) / np.float32(n_out)
    coord = np.arange(n_out, dtype=np.float32) * scale
    assert coord.dtype == np.float32
    lo = np.trunc(coord).astype(np.int64)
    hi = np.minimum(lo + 1, n_in - 1)
    d = coord - lo.astype(np.float32)
    return torch.from_numpy(lo), torch.from_numpy(hi), torch.from_numpy(d.astype(np.float32))


def resize_tf1(x: torch.Tensor, oh: int, ow: int, dtype=torch.float64) -> torch.Tensor:
    """[n, c, h, w] -> [n, c, oh, ow]: the coordinates in fp32, the values in `dtype` (fp64: the reference)"""
    x = x.to(dtype)
    h, w = x.shape[-2:]
    y0, y1, dy = taps(h, oh)
    x0, x1, dx = taps(w, ow)
    dy, dx = dy.to(dtype).view(-1, 1), dx.to(dtype).view(1, -1)
    top, bot = x[..., y0, :], x[..., y1, :]
    v0 = top[..., x0] + (top[..., x1] - top[..., x0]) * dx
    v1 = bot[..., x0] + (bot[..., x1] - bot[..., x0]) * dx
    return v0 + (v1 - v0) * dy


def prep(imgs: torch.Tensor, dtype=torch.float64, oh: int = SIZE, ow: int = SIZE) -> torch.Tensor:
    """fp32 [0, 1] (or uint8) [n, 3, h, w] -> the stem's input [n, 3, oh, ow]"""
    q = imgs.double() if imgs.dtype == torch.uint8 else quantise(imgs)
    return (resize_tf1(q, oh, ow, dtype) - 128) / 128


# ---- the stem -----------------------------------------------------------------------------------------------------------------------
def make_weights(seed: int = 6464, prefix: str = "") -> dict:
    """the stem's part of torch-fidelity's `pt_inception` state dict (fp32) of seeded random values: Kaiming-normal convs, BatchNorm
    gamma in [0.5, 1.5], beta 0.1 N, running_mean 0.1 N, running_var in [0.5, 1.5]; `prefix="inception."`: torchmetrics' layout"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, c_in, c_out, _, _ in LAYERS:
        sd[f"{prefix}{name}.conv.weight"] = (torch.randn(c_out, c_in, 3, 3, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (9 * c_in))).float()
        sd[f"{prefix}{name}.bn.weight"] = (0.5 + torch.rand(c_out, generator=g, dtype=torch.float64)).float()
        sd[f"{prefix}{name}.bn.bias"] = (0.1 * torch.randn(c_out, generator=g, dtype=torch.float64)).float()
        sd[f"{prefix}{name}.bn.running_mean"] = (0.1 * torch.randn(c_out, generator=g, dtype=torch.float64)).float()
        sd[f"{prefix}{name}.bn.running_var"] = (0.5 + torch.rand(c_out, generator=g, dtype=torch.float64)).float()
    return sd


def with_other_layers(sd: dict, prefix: str = "") -> dict:
    """the same file as the package ships it: with `num_batches_tracked` and keys of the layers after the tap"""
    out = dict(sd)
    for name, *_ in LAYERS:
        out[f"{prefix}{name}.bn.num_batches_tracked"] = torch.tensor(7)
    for k in ("Conv2d_3b_1x1.conv.weight", "Conv2d_4a_3x3.bn.running_var", "Mixed_5b.branch1x1.conv.weight", "Mixed_7c.branch_pool.bn.bias",
              "AuxLogits.fc.weight", "fc.weight", "fc.bias"):
        out[prefix + k] = torch.zeros(2, 2)
    return out


def fold_bn(sd: dict, name: str):
    """(w', b') in fp64: w' = w gamma / sqrt(var + eps), b' = beta - mean gamma / sqrt(var + eps)"""
    g = sd[f"{name}.bn.weight"].double() / (sd[f"{name}.bn.running_var"].double() + EPS).sqrt()
    return sd[f"{name}.conv.weight"].double() * g.view(-1, 1, 1, 1), sd[f"{name}.bn.bias"].double() - sd[f"{name}.bn.running_mean"].double() * g


def stem(x: torch.Tensor, sd: dict, dtype=torch.float64, emulate=None) -> torch.Tensor:
    """the stem's input [n, 3, h, w] -> the post-ReLU map of Conv2d_2b_3x3, NCHW.  fp64: BatchNorm applied unfused.  The emulations run
    the folded convolution with its bias, as the device does."""
    if dtype == torch.float64 and emulate is None:
        f = x.double()
        for name, _, _, stride, pad in LAYERS:
            f = F.conv2d(f, sd[f"{name}.conv.weight"].double(), None, stride=stride, padding=pad)
            v = lambda k: sd[f"{name}.bn.{k}"].double().view(1, -1, 1, 1)
            f = ((f - v("running_mean")) / (v("running_var") + EPS).sqrt() * v("weight") + v("bias")).relu()
        return f
    rnd = (lambda t: t.to(emulate).float()) if emulate is not None else (lambda t: t)
    f = rnd(x.float())
    for name, _, _, stride, pad in LAYERS:
        w, b = fold_bn(sd, name)
        f = rnd(F.conv2d(f, rnd(w.float()), b.float(), stride=stride, padding=pad)).relu()
    return f


def maxpool_mean(f: torch.Tensor) -> torch.Tensor:
    """NCHW (ReLU applied here too, so a pre-activation map may be given) -> fp64 [n, C]: MaxPool(3, 2), then the mean over the map"""
    return F.max_pool2d(f.relu(), 3, 2).double().mean((2, 3))


def features(imgs: torch.Tensor, sd: dict, dtype=torch.float64, emulate=None, chunk: int = 4) -> torch.Tensor:
    """fp32 [0, 1] images [n, 3, h, w] -> fp64 [n, 64]"""
    out = []
    for i in range(0, imgs.shape[0], chunk):
        x = prep(imgs[i:i + chunk], torch.float64 if (dtype == torch.float64 and emulate is None) else torch.float32)
        out.append(maxpool_mean(stem(x, sd, dtype, emulate)))
    return torch.cat(out)


# ---- the statistics and the distance ------------------------------------------------------------------------------------------------
def state(f: torch.Tensor) -> torch.Tensor:
    """fp64 [n, D] -> the 1 + D + D D doubles the device keeps: n, sum f, sum f^T f"""
    f = f.double()
    return torch.cat([torch.tensor([float(f.shape[0])], dtype=torch.float64), f.sum(0), (f.t() @ f).reshape(-1)])


def moments(st: torch.Tensor):
    """state -> (mu [D], Sigma [D, D]) as numpy fp64, the package's formula"""
    st = np.asarray(st, dtype=np.float64)
    d = int(round((-1 + math.sqrt(1 + 4 * (len(st) - 1))) / 2))
    n, s, o = st[0], st[1:1 + d], st[1 + d:].reshape(d, d)
    mu = s / n
    return mu, (o - n * np.outer(mu, mu)) / (n - 1)


def scale(st1, st2) -> float:
    """|mu1 - mu2|^2 + tr Sigma1 + tr Sigma2: what an error of the score is measured against (the score itself can be ~ 0)"""
    (m1, s1), (m2, s2) = moments(st1), moments(st2)
    return float(((m1 - m2) ** 2).sum() + np.trace(s1) + np.trace(s2))


def _psd_sqrt(s: np.ndarray) -> np.ndarray:
    lam, v = np.linalg.eigh((s + s.T) / 2)
    return (v * np.sqrt(np.maximum(lam, 0))) @ v.T


def frechet_sym(st1, st2) -> float:
    """the symmetric form the device computes: c = sum sqrt(max(lambda_i(Sigma1^1/2 Sigma2 Sigma1^1/2), 0)), `eigh` twice"""
    (m1, s1), (m2, s2) = moments(st1), moments(st2)
    r = _psd_sqrt(s1)
    m = r @ s2 @ r
    lam = np.linalg.eigvalsh((m + m.T) / 2)
    return float(((m1 - m2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2 * np.sqrt(np.maximum(lam, 0)).sum())


def frechet_pkg(st1, st2) -> float:
    """the package's route: c = sum Re sqrt(eigvals(Sigma1 Sigma2)), complex"""
    (m1, s1), (m2, s2) = moments(st1), moments(st2)
    lam = np.linalg.eigvals(s1 @ s2).astype(np.complex128)
    return float(((m1 - m2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2 * np.sqrt(lam).real.sum())


# the device's solve (csrc/fid.hip): the same constants, the same rotation order, the same operations in fp64
SWEEP_CAP = 30
TOL = 1e-22


def _round_pairs(r: int):
    k = np.arange(1, D // 2)
    a = np.concatenate([[D - 1], (r + k) % (D - 1)])
    b = np.concatenate([[r], (r - k + (D - 1)) % (D - 1)])
    return np.minimum(a, b), np.maximum(a, b)


def jacobi(a: np.ndarray, vectors: bool = False):
    """cyclic Jacobi, round-robin ordering, 32 disjoint rotations a round: (diagonal, V or None, sweeps, off / |A|_F, converged)"""
    a = np.array(a, dtype=np.float64)
    v = np.eye(D) if vectors else None
    off2_of = lambda m: float(((m - np.diag(np.diag(m))) ** 2).sum())
    fro2 = float((a * a).sum())
    off2, thresh, sw = off2_of(a), TOL * TOL * fro2, 0
    while not off2 <= thresh and sw < SWEEP_CAP:
        for r in range(D - 1):
            p, q = _round_pairs(r)
            app, aqq, apq = a[p, p], a[q, q], a[p, q]
            nz = apq != 0
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            t = np.where(nz, t, 0.0)
            c = np.where(nz, 1.0 / np.sqrt(t * t + 1.0), 1.0)
            s = np.where(nz, t * c, 0.0)
            x, y = a[:, p].copy(), a[:, q].copy()
            a[:, p], a[:, q] = c * x - s * y, s * x + c * y
            if vectors:
                x, y = v[:, p].copy(), v[:, q].copy()
                v[:, p], v[:, q] = c * x - s * y, s * x + c * y
            x, y = a[p, :].copy(), a[q, :].copy()
            a[p, :], a[q, :] = c[:, None] * x - s[:, None] * y, s[:, None] * x + c[:, None] * y
            a[p, p], a[q, q] = app - t * apq, aqq + t * apq
            a[p, q] = 0.0
            a[q, p] = 0.0
        sw += 1
        off2 = off2_of(a)
    return np.diag(a).copy(), v, sw, (math.sqrt(off2 / fro2) if fro2 > 0 else 0.0), bool(off2 <= thresh)


def jacobi_emulation(st1, st2):
    """the device's route in numpy fp64: (fid, info) with info = [sweeps 1, off 1, sweeps 2, off 2, solves that hit the cap]"""
    (m1, s1), (m2, s2) = moments(st1), moments(st2)
    d1, v, sw1, off1, ok1 = jacobi(s1, vectors=True)
    sd = np.sqrt(np.maximum(d1, 0))
    m = v.T @ (s2 @ v)
    s = sd[:, None] * (0.5 * (m + m.T)) * sd[None, :]
    lam, _, sw2, off2, ok2 = jacobi(s)
    c = np.sqrt(np.maximum(lam, 0)).sum()
    fid = float(((m1 - m2) ** 2).sum() + (np.trace(s1) + np.trace(s2)) - 2 * c)
    return (fid if ok1 and ok2 else float("nan")), [sw1, off1, sw2, off2, int(not ok1) + int(not ok2)]


def fid(real: torch.Tensor, fake: torch.Tensor, sd: dict, dtype=torch.float64, emulate=None, route=frechet_sym):
    """two image sets -> (score, state of the real set, state of the fake set)"""
    s1, s2 = state(features(real, sd, dtype, emulate)), state(features(fake, sd, dtype, emulate))
    return route(s1, s2), s1, s2


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def make_images(n: int, h: int, w: int, seed: int, kind: str = "mixed") -> torch.Tensor:
    """[n, 3, h, w] fp32 in [0, 1]: image i is smooth (a low-frequency field), noisy (uniform noise) or nearly constant, in turn"""
    g = torch.Generator().manual_seed(seed)
    out = torch.empty(n, 3, h, w)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    for i in range(n):
        k = i % 3 if kind == "mixed" else ("smooth", "noisy", "constant").index(kind)
        if k == 0:
            ph = torch.rand(3, 4, generator=g)
            out[i] = torch.stack([0.5 + 0.25 * torch.sin(6 * (ph[c, 0] * yy + ph[c, 1] * xx) + 6 * ph[c, 2]) + 0.2 * (ph[c, 3] - 0.5) for c in range(3)])
        elif k == 1:
            out[i] = torch.rand(3, h, w, generator=g)
        else:
            out[i] = torch.rand(3, 1, 1, generator=g).expand(3, h, w) * 0.9 + 0.02 * torch.rand(3, h, w, generator=g)
    return out.clamp(0, 1).contiguous()


PAIRS = ("other", "brighter", "noise")


def make_sets(pair: str, n_real: int, n_fake: int, h: int, w: int, seed: int):
    """(real, fake): `other` -- independent sets; `brighter` -- the fake set is another draw, shifted up by 0.1; `noise` -- the first
    min(n) real images with noise of amplitude 0.05 added, then fresh ones"""
    real = make_images(n_real, h, w, seed)
    fake = make_images(n_fake, h, w, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    if pair == "brighter":
        fake = (fake + 0.1).clamp(0, 1)
    elif pair == "noise":
        m = min(n_real, n_fake)
        fake[:m] = (real[:m] + 0.05 * (torch.rand(m, 3, h, w, generator=g) - 0.5)).clamp(0, 1)
    return real, fake.contiguous()


# the cases of the whole-metric parity test (tests/test_hip_fid.py) and of the CPU bounds (tests/golden/make_fid_bounds.py): every one is
# rank-deficient (n - 1 < 64), as the reference's per-scene use is
CASES = [(2, 2, 16, 24), (5, 5, 16, 24), (3, 7, 16, 24), (4, 4, 256, 256)]
WEIGHT_SEED = 6464


def case_seed(n_real: int, n_fake: int, h: int, w: int) -> int:
    return h * 1000 + w + 7 * n_real + 13 * n_fake


def case_key(pair: str, n_real: int, n_fake: int, h: int, w: int) -> str:
    return f"{pair}/{n_real}+{n_fake}x3x{h}x{w}"


# ---- synthetic states for the solve alone (tests/test_hip_fid.py "compute", tests/golden/make_fid_bounds.py) -------------------------
def state_from_moments(mu: np.ndarray, sigma: np.ndarray, n: int = 100) -> torch.Tensor:
    """the state whose `moments` are (mu, sigma) up to round-off"""
    outer = sigma * (n - 1) + n * np.outer(mu, mu)
    return torch.from_numpy(np.concatenate([[float(n)], mu * n, outer.reshape(-1)]))


def random_state(n: int, seed: int, constant_column: bool = False) -> torch.Tensor:
    """the state of n random non-negative feature vectors (rank min(n - 1, 64))"""
    f = torch.rand(n, D, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * torch.linspace(0.2, 2.0, D, dtype=torch.float64)
    if constant_column:
        f[:, 5] = 0.75
    return state(f)


def synthetic_cases() -> dict:
    """name -> (class, state 1, state 2, analytic c or None)"""
    rng = np.random.default_rng(99)
    qm, _ = np.linalg.qr(rng.standard_normal((D, D)))
    a, b = rng.uniform(0.1, 2.0, D), rng.uniform(0.1, 2.0, D)
    mu1, mu2 = rng.uniform(0, 1, D), rng.uniform(0, 1, D)
    wide = np.logspace(-9, 3, D)
    out = {
        "commuting": ("full", state_from_moments(mu1, (qm * a) @ qm.T), state_from_moments(mu2, (qm * b) @ qm.T), float(np.sqrt(a * b).sum())),
        "diagonal": ("full", state_from_moments(mu1, np.diag(a)), state_from_moments(mu2, np.diag(b)), float(np.sqrt(a * b).sum())),
        "decades12": ("full", state_from_moments(mu1, (qm * wide) @ qm.T), state_from_moments(mu2, (qm * wide[::-1]) @ qm.T), None),
        "identical": ("full", random_state(300, 5), random_state(300, 5), None),
        "identical_deficient": ("deficient", random_state(5, 6), random_state(5, 6), None),
        "constant_column": ("deficient", random_state(300, 7, True), random_state(200, 8, True), None),      # a zero row and column: rank 63
        "deficient_vs_full": ("deficient", random_state(5, 9), random_state(300, 10), None),
    }
    for n in (65, 300):
        out[f"full_{n}"] = ("full", random_state(n, 100 + n), random_state(n, 200 + n), None)
    for n in (2, 3, 5, 63):
        out[f"deficient_{n}"] = ("deficient", random_state(n, 300 + n), random_state(n, 400 + n), None)
    return out
