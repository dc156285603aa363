"""Where the worst-element bounds of `close_grad` (test_hip_backward_edges.py) come from: each training kernel's DOCUMENTED arithmetic
evaluated in torch on the CPU -- no kernel runs here -- against the fp64 reference of the tests, over all cases of the kind in
test_hip_backward.py (small-shape tests) and test_hip_backward_edges.py.

    fp32 accumulation        GEMM-like products of the attention backward in K-steps of 16 (the MFMA's K), conv / linear gradients as
                             torch's own fp32 convolution / matmul gradients, column and parameter sums one row after the other
    16-bit rounding          where the kernel rounds: attention P and dS to the activation type before the second products
                             (attention_bwd.hip header); conv data gradients at the upsampled size before the 2x2 sums; every output
                             to its dtype (weight / parameter gradients and column sums are fp32)
    fp32 statistics          the attention log-sum-exp, `out` in the activation type, (mean, rstd) of the norms
    GELU                     the A-S 7.1.26 erf polynomial of common.h (|error| <= 1.5e-7)

`python tests/grad_emulation.py` prints max|emulation - fp64| / rms(fp64) per (kind, dtype) and 3 x that value, the bound.

A further kind, `wgrad_long`, does the same for the split weight gradients of test_hip_wgrad_edges.py, whose sums are up to 4096 pixels long:
products of the dtype-rounded operands, fp32 accumulation over the pixel index in steps of 16, one partial per split of `rows_per_split`
rows (the launch rule restated in that module), partials added in split order in fp32, the accumulate case added onto the previous
gradient.  Its rows give the worst element / RMS and the relative L2 per case family and dtype, over every launch of the family."""
import functools
import math
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import test_hip_backward as B       # noqa: E402
import test_hip_backward_edges as E  # noqa: E402
import test_hip_wgrad_edges as W  # noqa: E402
from test_hip_backward_edges import G, rnd, worst_over_rms  # noqa: E402

DTYPES, IDS = E.DTYPES, E.IDS


def to(t, dtype):
    """rounded once to the dtype"""
    return t.float().to(dtype).float()


def mm(a, b, step=16):
    """a @ b with fp32 accumulation over K in steps of `step`"""
    a, b = a.float(), b.float()
    acc = torch.zeros(*a.shape[:-1], b.shape[-1])
    for k in range(0, a.shape[-1], step):
        acc = acc + a[..., k:k + step] @ b[..., k:k + step, :]
    return acc


def seq_sum(t, dim=0):
    """fp32 sum, one term after the other"""
    return t.float().cumsum(dim).select(dim, -1)


# ------------------------------------------------------------------------------------------------ attention
def emu_attention(c, dtype):
    heads, d = c["heads"], c["d"]
    C_ = heads * d
    scale = torch.tensor(d ** -0.5, dtype=torch.float32)
    c2 = torch.tensor(float(scale) * 1.4426950408889634, dtype=torch.float32)
    out16 = to(c["out"], dtype)
    dq, dk, dv = torch.zeros_like(c["q"]), torch.zeros_like(c["k"]), torch.zeros_like(c["v"])
    q0 = k0 = 0
    for ql, kl in c["segs"]:
        hv = lambda t, r0, n: t[r0:r0 + n].view(n, heads, d).transpose(0, 1).float()      # noqa: E731
        qq, do, oo = hv(c["q"], q0, ql), hv(c["dout"], q0, ql), hv(out16, q0, ql)
        kk, vv = hv(c["k"], k0, kl), hv(c["v"], k0, kl)
        lse = c["lse"][:, q0:q0 + ql].float()
        delta = seq_sum(do * oo, -1)
        p = torch.exp2(mm(qq, kk.transpose(1, 2)) * c2 - lse[..., None])
        ds = p * (mm(do, vv.transpose(1, 2)) - delta[..., None])
        p, ds = to(p, dtype), to(ds, dtype)
        back = lambda t, n: t.transpose(0, 1).reshape(n, C_)      # noqa: E731
        dv[k0:k0 + kl] = back(mm(p.transpose(1, 2), do), kl)
        dk[k0:k0 + kl] = back(mm(ds.transpose(1, 2), qq) * scale, kl)
        dq[q0:q0 + ql] = back(mm(ds, kk) * scale, ql)
        q0, k0 = q0 + ql, k0 + kl
    return to(dq, dtype), to(dk, dtype), to(dv, dtype)


def attention_cases(dtype):
    for d in E.DP_WIDTHS:
        yield E.attn_case(2, d, E.DP_SEGS, dtype)
    for heads, d in E.PROD_WIDTHS:
        yield E.attn_case(heads, d, E.PROD_SEGS, dtype, seed=50)
    yield E.attn_case(2, 64, ((300, 300),), dtype, seed=60, dominate=True)
    for d in (40, 64):
        yield E.attn_case(2, d, E.GUARD_SEGS, dtype, seed=70)
    for _, t, d in E.WIDE:
        if t == dtype:
            yield E.attn_case(2, d, E.WIDE_SEGS, dtype, seed=80)
    for _, heads, d, segs in B.ATTN:
        yield E.attn_case(heads, d, tuple(segs), dtype, seed=26)


def worst_attention(dtype):
    w = 0.0
    for c in attention_cases(dtype):
        for got, ref in zip(emu_attention(c, dtype), (c["gq"], c["gk"], c["gv"])):
            w = max(w, worst_over_rms(got, ref))
    return w


# ------------------------------------------------------------------------------------------------ norms
def silu_grad(g):
    sg = torch.sigmoid(g)
    return sg * (1.0 + g * (1.0 - sg))


def emu_groupnorm(k, dtype, silu, groups=E.GN_GROUPS):
    """-> dx (all channels), dgamma, dbeta"""
    x = (k["a"] if k["b"] is None else torch.cat([k["a"], k["b"]], 1)).float()
    n, c, h, w = x.shape
    xg = x.double().view(n, groups, -1)
    mu = xg.mean(-1).float()
    rs = (xg.var(-1, unbiased=False) + 1e-5).rsqrt().float()
    per_ch = lambda t: t.repeat_interleave(c // groups, 1)[:, :, None, None]      # noqa: E731
    ga, be = k["gamma"].float()[None, :, None, None], k["beta"].float()[None, :, None, None]
    z = (x - per_ch(mu)) * per_ch(rs)
    dg = k["dy"].float()
    if silu:
        dg = dg * silu_grad(z * ga + be)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(n * h * w, c)      # noqa: E731
    dbeta, dgamma = seq_sum(flat(dg)), seq_sum(flat(dg * z))
    inv = 1.0 / (h * w * (c // groups))
    m1 = (dg * ga).view(n, groups, -1).sum(-1) * inv
    m2 = (dg * ga * z).view(n, groups, -1).sum(-1) * inv
    dx = per_ch(rs) * (dg * ga - per_ch(m1) - z * per_ch(m2))
    return to(dx, dtype), dgamma, dbeta


def emu_layernorm(k, dtype):
    x, dy, ga = k["x"].float(), k["dy"].float(), k["gamma"].float()
    c = x.shape[1]
    mean = x.sum(1, keepdim=True) / c
    rstd = (((x - mean) ** 2).sum(1, keepdim=True) / c + 1e-5).rsqrt()
    z = (x - mean) * rstd
    dz = dy * ga
    s1, s2 = dz.sum(1, keepdim=True) / c, (dz * z).sum(1, keepdim=True) / c
    return to(rstd * (dz - s1 - z * s2), dtype), seq_sum(dy * z), seq_sum(dy)


def old_gn_case(dtype, silu, dual):       # test_hip_backward.py::test_groupnorm_backward
    n, c0, c1, h = 3, 64, 32, 12
    a, b = rnd((n, c0, h, h), 17, dtype, 1.5), (rnd((n, c1, h, h), 18, dtype) if dual else None)
    c = c0 + (c1 if dual else 0)
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=G(19)), 0.1 * torch.randn(c, generator=G(20))
    dy = rnd((n, c, h, h), 21, dtype)
    with torch.enable_grad():
        xd, gd, bd = (a if b is None else torch.cat([a, b], 1)).double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
        y = F.group_norm(xd, 32, gd, bd, 1e-5)
        gx, gg, gb = torch.autograd.grad(F.silu(y) if silu else y, (xd, gd, bd), dy.double())
    return dict(a=a, b=b, gamma=gamma, beta=beta, dy=dy), gx, gg, gb


def worst_norms(dtype):
    """-> (dx, parameter sums)"""
    wx = wp = 0.0
    for silu in (False, True):
        for name in E.GN_CASES:
            k = E.gn_case(name, dtype, silu)
            dx, dgam, dbet = emu_groupnorm(k, dtype, silu)
            gx = k["ga"] if k["gb"] is None else torch.cat([k["ga"], k["gb"]], 1)
            c0 = k["ga"].shape[1]
            wx = max(wx, worst_over_rms(dx[:, :c0], k["ga"]), worst_over_rms(dx[:, c0:], k["gb"]) if k["gb"] is not None else 0.0)
            wp = max(wp, worst_over_rms(dgam, k["gg"]), worst_over_rms(dbet, k["gbeta"]))
            assert gx.shape == dx.shape
        for dual in (False, True):
            k, gx, gg, gb = old_gn_case(dtype, silu, dual)
            dx, dgam, dbet = emu_groupnorm(k, dtype, silu)
            wx = max(wx, worst_over_rms(dx[:, :64], gx[:, :64]), worst_over_rms(dx[:, 64:], gx[:, 64:]) if dual else 0.0)
            wp = max(wp, worst_over_rms(dgam, gg), worst_over_rms(dbet, gb))
    for rows, c in [(p.values[0], p.values[1]) for p in E.LN_PARAMS if p.values[2] == dtype] + [(333, 320), (333, 640), (333, 1280)]:
        k = E.ln_case(rows, c, dtype)
        dx, dgam, dbet = emu_layernorm(k, dtype)
        wx = max(wx, worst_over_rms(dx, k["gx"]))
        wp = max(wp, worst_over_rms(dgam, k["gg"]), worst_over_rms(dbet, k["gb"]))
    return wx, wp


def worst_colsum(dtype):
    w = 0.0
    for name, (n_seg, rps, n, per_seg) in E.COLSUM_CASES.items():
        k = E.colsum_case(name, dtype)
        real = k["x"][:, k["col0"]:k["col0"] + n]
        got = seq_sum(real.view(n_seg, rps, n), 1) if per_seg else seq_sum(real)
        w = max(w, worst_over_rms(got, k["ref"]), worst_over_rms(got + 1.5, k["ref"] + 1.5))
    dy = rnd((300, 192), 16, dtype)             # test_linear_gradients_column_slices_and_bias_sums
    w = max(w, worst_over_rms(seq_sum(dy) + 1.0, dy.double().sum(0) + 1.0), worst_over_rms(seq_sum(dy.view(4, 75, 192), 1), dy.double().view(4, 75, 192).sum(1)))
    return w


# ------------------------------------------------------------------------------------------------ conv / linear gradients
def conv_grads(x, w, dy_of, dtype, stride=1, up=False):
    """fp64 and fp32-accumulated (data gradient, weight gradient) of conv2d; `dy_of(shape)` makes the upstream gradient"""
    res = []
    for ft in (torch.float64, torch.float32):
        with torch.enable_grad():
            xd, wd = x.to(ft).requires_grad_(), to(w, dtype).to(ft).requires_grad_()
            xin = F.interpolate(xd, scale_factor=2, mode="nearest").detach().requires_grad_() if up else xd
            y = F.conv2d(xin, wd, None, stride, w.shape[-1] // 2)
            dy = dy_of(tuple(y.shape))
            gx, gw = torch.autograd.grad(y, (xin, wd), dy.to(ft))
        if up:      # the kernel path: gradient at the upsampled size in the activation type, then 2x2 sums
            n, ci, h2, w2 = gx.shape
            if ft == torch.float32:
                gx = to(gx, dtype)
            gx = gx.view(n, ci, h2 // 2, 2, w2 // 2, 2).sum((3, 5))
        res.append((gx if ft == torch.float64 else to(gx, dtype), gw))
    return res


def worst_gemm(dtype):
    """-> (data gradients, weight gradients)"""
    wd = ww = 0.0
    cases = []
    for _, n, ci, co, h, ks, stride, up in B.CONVS:
        cases.append((rnd((n, ci, h, h), 1, dtype), rnd((co, ci, ks, ks), 2, torch.float32, 1 / math.sqrt(ci * ks * ks)), 3, stride, up))
    cases.append((rnd((2, 192, 8, 8), 4, dtype), rnd((64, 192, 3, 3), 6, torch.float32, 1 / math.sqrt(9 * 192)), 7, 1, False))        # skip concat
    cases.append((rnd((2, 11, 8, 8), 8, dtype), rnd((64, 11, 3, 3), 9, torch.float32, 0.1), 10, 1, False))                             # conv_in
    cases.append((rnd((2, 64, 8, 8), 11, dtype), rnd((4, 64, 3, 3), 12, torch.float32, 0.05), 13, 1, False))                           # conv_out
    cases.append((rnd((300, 128, 1, 1), 14, dtype), rnd((192, 128, 1, 1), 15, torch.float32, 1 / math.sqrt(128)), 16, 1, False))       # linear
    for x, w, seed, stride, up in cases:
        (gx, gw), (ex, ew) = conv_grads(x, w, lambda s: rnd(s, seed, dtype), dtype, stride, up)
        wd, ww = max(wd, worst_over_rms(ex, gx)), max(ww, worst_over_rms(ew, gw), worst_over_rms(ew + ew, 2 * gw))
    return wd, ww


# ------------------------------------------------------------------------------------------------ long weight-gradient sums
@functools.lru_cache(maxsize=None)
def im2col(name, dtype):
    """-> (A [M, c * k * k] in PyTorch's (c, ky, kx) column order, dY [M, n_out]) of a case of test_hip_wgrad_edges.py, fp32"""
    k = W.case(name, dtype)
    xin = F.interpolate(k["x"], scale_factor=2, mode="nearest") if k["up"] else k["x"]
    a = F.unfold(xin, k["ks"], padding=k["pad"], stride=k["stride"])              # [n, c * k * k, h_out * w_out]
    return a.permute(0, 2, 1).reshape(-1, a.shape[1]).contiguous(), k["dy"].permute(0, 2, 3, 1).reshape(-1, k["co"]).contiguous()


def emu_wgrad_long(name, dtype, rps, accumulate):
    """one fp32 partial per split of `rps` pixel rows, each accumulated in steps of 16 pixels; partials added in split order"""
    k = W.case(name, dtype)
    a, d = im2col(name, dtype)
    total = None
    for m0 in range(0, a.shape[0], rps):
        part = mm(d[m0:m0 + rps].t(), a[m0:m0 + rps], step=16)
        total = part if total is None else total + part
    total = total.view(k["gw"].shape)
    return k["g0"] + total if accumulate else total


def wgrad_long_table():
    """family -> per dtype (worst element / RMS, relative L2), the maximum over the family's launches"""
    rows = {}
    for dtype in DTYPES:
        for family, name, rps, accumulate in W.emulation_runs(dtype):
            k = W.case(name, dtype)
            ref = k["g0"].double() + k["gw"] if accumulate else k["gw"]
            l2, worst = W.errors(emu_wgrad_long(name, dtype, rps, accumulate), ref)
            cur = rows.setdefault(family, {}).setdefault(dtype, (0.0, 0.0))
            rows[family][dtype] = (max(cur[0], worst), max(cur[1], l2))
    return rows


# ------------------------------------------------------------------------------------------------ elementwise
def erf_as(x):
    """common.h erf_as_f: Abramowitz-Stegun 7.1.26 in fp32"""
    ax = x.abs()
    t = 1.0 / (0.3275911 * ax + 1.0)
    poly = 1.061405429 * t - 1.453152027
    for cf in (1.421413741, -0.284496736, 0.254829592):
        poly = poly * t + cf
    return torch.copysign(1.0 - poly * t * torch.exp(-ax * ax), x)


def gelu_as(x):
    return 0.5 * x * (1.0 + erf_as(x * 0.70710678118654752440))


def gelu_grad_as(x):
    return 0.5 * (1.0 + erf_as(x * 0.70710678118654752440)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)


def worst_eltwise(dtype):
    w = 0.0

    def geglu(rows, D, s0, s1):
        ag, dh = rnd((rows, 2 * D), s0, dtype), rnd((rows, D), s1, dtype)
        with torch.enable_grad():
            agd = ag.double().requires_grad_()
            h = agd[:, :D] * F.gelu(agd[:, D:])
            (gag,) = torch.autograd.grad(h, agd, dh.double())
        a, g = ag[:, :D], ag[:, D:]
        return max(worst_over_rms(to(a * gelu_as(g), dtype), h), worst_over_rms(to(torch.cat([dh * gelu_as(g), dh * a * gelu_grad_as(g)], 1), dtype), gag))
    w = max(w, geglu(77, 8, 93, 94), geglu(9, 5120, 93, 94), geglu(77, 256, 30, 31))
    for act, grad, (rows, d, s0, s1) in ((F.gelu, gelu_grad_as, (77, 1280, 91, 92)), (F.silu, silu_grad, (5, 1280, 32, 33))):
        x, dy = rnd((rows, d), s0, dtype, 2.0), rnd((rows, d), s1, dtype)
        with torch.enable_grad():
            xd = x.double().requires_grad_()
            (gx,) = torch.autograd.grad(act(xd), xd, dy.double())
        w = max(w, worst_over_rms(to(dy * grad(x), dtype), gx))
    for shape, seed in (((2, 6, 10, 8), 95), ((1, 4, 2, 1280), 95), ((2, 8, 8, 32), 34)):
        n, h, wd_, c = shape
        du = rnd(shape, seed, dtype).view(n, h // 2, 2, wd_ // 2, 2, c)
        got = (du[:, :, 0, :, 0] + du[:, :, 0, :, 1]) + (du[:, :, 1, :, 0] + du[:, :, 1, :, 1])
        w = max(w, worst_over_rms(to(got, dtype), du.double().sum((2, 4))))
    if dtype == torch.float32:          # the fp32 MSE gradient: grad_scale * 2 / N formed in fp32, one product
        g = G(96)
        pred, noise = torch.randn(3, 8, 8, 4, generator=g), torch.randn(3, 8, 8, 4, generator=g)
        gs = torch.tensor(2.0 * 0.5 / pred.numel(), dtype=torch.float32)
        w = max(w, worst_over_rms(gs * (pred - noise), (pred.double() - noise.double()) / pred.numel()))
    return w


def table():
    rows = {k: [] for k in ("attn", "norm_dx", "param", "wgrad", "dgrad", "eltwise")}
    for dtype in DTYPES:
        wx, wp = worst_norms(dtype)
        wd, ww = worst_gemm(dtype)
        for k, v in (("attn", worst_attention(dtype)), ("norm_dx", wx), ("param", max(wp, worst_colsum(dtype))), ("wgrad", ww), ("dgrad", wd),
                     ("eltwise", worst_eltwise(dtype))):
            rows[k].append(v)
    return rows


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    print(f"{'kind':10s}" + "".join(f"{i:>11s}" for i in IDS) + "   |" + "".join(f"{'3x ' + i:>11s}" for i in IDS))
    for kind, vals in table().items():
        print(f"{kind:10s}" + "".join(f"{v:11.2e}" for v in vals) + "   |" + "".join(f"{3 * v:11.2e}" for v in vals))
    print()
    print(f"{'wgrad_long':13s}{'longest sum':16s}{'emulated worst element / RMS':34s}{'emulated relative L2':34s}{'bound: worst (3 x)':34s}bound: rel. L2 (3 x)")
    print(f"{'family':13s}{'(pixels)':13s}" + "".join("".join(f"{i:>10s}" for i in IDS) + "    " for _ in range(4)).rstrip())
    long_rows = wgrad_long_table()
    for family in W.EMU:                # (a family that no test runs in a dtype has no value there)
        line = f"{family:13s}{W.EMU[family]['longest']:<13d}"
        for f in (lambda v: v[0], lambda v: v[1], lambda v: 3 * v[0], lambda v: 3 * v[1]):
            line += "".join(f"{f(long_rows[family][t]):10.2e}" if t in long_rows[family] else f"{'-':>10s}" for t in DTYPES) + "    "
        print(line.rstrip())
