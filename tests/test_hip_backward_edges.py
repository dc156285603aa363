"""GPU parity of the TRAINING kernels at their edges: every head width of the attention backward, ragged tiles, second column
sweeps, one-row inputs, capped slab counts -- and a WORST-ELEMENT bound next to the relative L2 of test_hip_backward.py.

One element wrong by k x RMS in a tensor of N elements moves the relative L2 by k / sqrt(N): a bad lane of an epilogue, a wrong
last chunk of a row or a wrong tile corner passes an L2 bound.  `close_grad` therefore also bounds max|got - ref| / rms(ref).

References: torch.autograd on the CPU in fp64 of the same op built from plain torch primitives, from the SAME dtype-rounded inputs.

Where the worst-element bounds come from (never from a kernel): tests/grad_emulation.py evaluates each kernel's DOCUMENTED
arithmetic in torch on the CPU -- fp32 accumulation (GEMM products in K-steps of 16 like the MFMA, column sums one row after the
other), 16-bit rounding where the kernel rounds (attention: P and dS rounded to the activation type before the second products,
attention_bwd.hip header; the saved log-sum-exp and the statistics of the norms in fp32), the A-S 7.1.26 erf of the GELU, the
output rounded to its dtype -- and takes max|emulation - fp64| / rms(fp64) over ALL cases of the kind in this module and in
test_hip_backward.py.  The bound is 3 x the largest value per (kind, dtype): the factor covers a different summation order and
the extreme-value spread of a maximum over <= 1e6 elements.  `python tests/grad_emulation.py` prints the table:

    kind      what                                              emulated worst element / RMS          bound (3 x)
                                                                f32        bf16       f16             f32      bf16     f16
    attn      dq / dk / dv of the attention backward            4.03e-05  1.71e-01  3.34e-02      1.21e-04  5.14e-01  1.00e-01
    norm_dx   dx of GroupNorm(+SiLU) / LayerNorm                1.25e-06  2.34e-02  2.98e-03      3.75e-06  7.02e-02  8.95e-03
    param     dgamma / dbeta / column sums (fp32 outputs)       5.87e-07  7.13e-07  6.34e-07      1.76e-06  2.14e-06  1.90e-06
    wgrad     conv / linear weight gradients (fp32 outputs)     3.09e-06  1.24e-06  2.92e-06      9.26e-06  3.73e-06  8.75e-06
    dgrad     conv / linear data gradients                      2.35e-06  1.42e-02  1.69e-03      7.04e-06  4.27e-02  5.07e-03
    eltwise   GELU / GEGLU / SiLU backward, 2x2 sums            2.22e-06  4.51e-02  5.48e-03      6.67e-06  1.35e-01  1.64e-02

A kernel that exceeds 3 x its emulation is a finding about the kernel, not about the factor.
"""
import functools
import math
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

GRAD_ENABLED = True       # tests/conftest.py::_grad_mode: torch references are differentiated here
pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.float16: 2e-3, torch.bfloat16: 1.2e-2}          # relative L2, as in test_hip_backward.py
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
CSRC = Path(__file__).resolve().parent.parent / "mv_ldm_amd" / "csrc"

# relative-L2 bound per kind: the multiples of TOL that test_hip_backward.py uses for the same kernels
L2 = {"attn": lambda t: 3e-5 if t == torch.float32 else TOL[t] * 3, "norm_dx": lambda t: TOL[t] * 2, "param": lambda t: TOL[t] * 2,
      "wgrad": lambda t: TOL[t], "dgrad": lambda t: TOL[t], "eltwise": lambda t: TOL[t] * 2}
# worst element / RMS per kind: 3 x the emulated value of the table above (tests/grad_emulation.py)
WORST = {
    "attn": {torch.float32: 1.21e-04, torch.bfloat16: 5.14e-01, torch.float16: 1.00e-01},
    "norm_dx": {torch.float32: 3.75e-06, torch.bfloat16: 7.02e-02, torch.float16: 8.95e-03},
    "param": {torch.float32: 1.76e-06, torch.bfloat16: 2.14e-06, torch.float16: 1.90e-06},
    "wgrad": {torch.float32: 9.26e-06, torch.bfloat16: 3.73e-06, torch.float16: 8.75e-06},
    "dgrad": {torch.float32: 7.04e-06, torch.bfloat16: 4.27e-02, torch.float16: 5.07e-03},
    "eltwise": {torch.float32: 6.67e-06, torch.bfloat16: 1.35e-01, torch.float16: 1.64e-02},
}


def worst_over_rms(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.pow(2).mean().sqrt().clamp_min(1e-30))


def close_grad(got, ref, dtype, kind, l2=None, what=""):
    """the relative L2 of test_hip_backward.py (`l2`: the bound of the assertion it joins) AND the worst element over the reference's RMS"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite gradient"
    l2 = L2[kind](dtype) if l2 is None else l2
    e2 = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
    emax = worst_over_rms(got, ref)
    print(f"close_grad {kind} {what}: rel-L2 {e2:.3e} (tol {l2:.1e}), worst/rms {emax:.3e} (tol {WORST[kind][dtype]:.1e})")
    assert e2 < l2 and emax <= WORST[kind][dtype], \
        f"{kind} {what}: rel-L2 {e2:.3e} (tol {l2:.1e}), worst element / rms {emax:.3e} (tol {WORST[kind][dtype]:.1e})"


@pytest.fixture(scope="module")
def ops():
    from mv_ldm_amd import ops as O
    from mv_ldm_amd import _lib as L
    L.load()
    return O


def G(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, dtype, scale=1.0):
    return (torch.randn(shape, generator=G(seed)) * scale).to(dtype).float()


def epc(dtype):
    return 4 if dtype == torch.float32 else 8


def nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ launch rules, restated
# The cases below are chosen to reach named branches of the host-side launch rules.  The rules are restated here and the source is
# required to still hold them, so that a later change of a rule fails a test here instead of silently moving a case off its branch.
def gn_chunks(n_img, hw):
    """norm_bwd.hip gn_chunks -> (row slabs per image, rows per slab)"""
    from mv_ldm_amd import _lib as L
    nchunk = min(L.GN_MAX_CHUNKS, max(1, min(hw // 8, (1024 + n_img - 1) // n_img)))
    rpc = (hw + nchunk - 1) // nchunk
    return (hw + rpc - 1) // rpc, rpc


def column_sweeps(c, dtype):
    """gn_bwd_partial_kernel / gn_bwd_apply_kernel / colsum_partial_kernel: 256 16-byte chunk columns per sweep"""
    return (c // epc(dtype) + 255) // 256


def ln_launch(rows, c, dtype):
    """norm_bwd.hip layernorm_bwd_run -> (workgroups of 4 waves, MAXCH, accepted)"""
    ncc = c // epc(dtype)
    blocks = max(1, min((rows + 3) // 4, 512))
    return blocks, (1 if ncc <= 64 else 2 if ncc <= 128 else 4 if ncc <= 256 else 8), c % epc(dtype) == 0 and ncc <= 64 * 8


def colsum_chunks(n_seg, rows_per_seg):
    """train_misc.hip colsum_run -> (row chunks per segment, rows per chunk)"""
    nchunk = max(1, min(min(rows_per_seg // 8, 512), (1024 + n_seg - 1) // n_seg))
    rpc = (rows_per_seg + nchunk - 1) // nchunk
    return (rows_per_seg + rpc - 1) // rpc, rpc


RULES_IN_SOURCE = [
    ("norm_bwd.hip", "nchunk = std::min(MVLDM_GN_MAX_CHUNKS, std::max(1, std::min(hw / 8, (1024 + n_img - 1) / n_img)));"),
    ("norm_bwd.hip", "rpc = (hw + nchunk - 1) / nchunk; nchunk = (hw + rpc - 1) / rpc;"),
    ("norm_bwd.hip", "for (int cc0 = 0; cc0 < ncc; cc0 += 256) { const int span = min(ncc - cc0, 256); const int RB = max(1, 256 / span);"),
    ("norm_bwd.hip", "const int blocks = std::max(1, std::min((rows + 3) / 4, 512));"),
    ("norm_bwd.hip", "MVLDM_REQUIRE(c % epc == 0 && c / epc <= 64 * 8,"),
    ("norm_bwd.hip", "if (ncc <= 64) MVLDM_LN_BWD(1) else if (ncc <= 128) MVLDM_LN_BWD(2) else if (ncc <= 256) MVLDM_LN_BWD(4) else MVLDM_LN_BWD(8)"),
    ("train_misc.hip", "int nchunk = std::max(1, std::min(std::min(rows_per_seg / 8, 512), (1024 + n_seg - 1) / n_seg));"),
    ("train_misc.hip", "const int rpc = (rows_per_seg + nchunk - 1) / nchunk; nchunk = (rows_per_seg + rpc - 1) / rpc;"),
    ("attention_bwd.hip", "constexpr int BR = 128, BS = 64;"),
    ("attention_bwd.hip", "switch (a.head_dim <= 160 ? dp : 0) {"),
    ("attention_bwd.hip", "if (nch <= 64) return launch_bwd_ref<T, 1>(p, a.n_seg, a.max_q_len, a.max_kv_len, s); if (nch <= 128) return launch_bwd_ref<T, 2>"),
]


def _squeeze(text):
    return re.sub(r"\s+", " ", text)


def attn_dp(d):
    """attention_bwd.hip attention_bwd_run: the DP instantiation of a 16-bit head width"""
    return (d + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ cases
DP_WIDTHS = [8, 24, 32, 56, 72, 96, 104, 112, 128, 136, 144, 152]
DP_SEGS = ((129, 65), (63, 191), (1, 1))      # one row past a resident tile, +-1 around a streamed tile, 1 x 1, q_len != kv_len both ways
PROD_SEGS = ((257, 255), (64, 320), (127, 1))
PROD_WIDTHS = [(8, 40), (5, 64)]              # (heads, d) of the multi-view and the SD attention blocks
GUARD_SEGS = ((65, 129), (129, 65), (1, 1))   # equal totals: q / k / v from one fused projection, gradients into one fused buffer
WIDE = [("f32_d320", torch.float32, 320), ("bf16_d512", torch.bfloat16, 512), ("f32_d64", torch.float32, 64), ("bf16_d64", torch.bfloat16, 64),
        ("f16_d64", torch.float16, 64)]
WIDE_SEGS = ((70, 33),)

GN_CASES = {  # name: n, c0, c1, h, w
    "straddle": (3, 320, 0, 5, 7), "two_sweeps": (2, 1280, 1280, 2, 2), "cap": (2, 64, 0, 17, 17), "concat": (2, 640, 320, 4, 4)}
GN_GROUPS = 32
LN_CASES = [(1, 320), (3, 320), (4099, 320), (2051, 1280), (9, 64), (9, 2560), (9, 2048)]     # rows, c


# c = 2560 (MAXCH = 8) is a 16-bit case: in f32 it has more than 512 chunk columns; c = 2048 is its f32 counterpart
LN_PARAMS = [pytest.param(r, c, t, id=f"{r}x{c}-{i}") for r, c in LN_CASES for t, i in zip(DTYPES, IDS)
             if not (c == 2560 and t == torch.float32) and not (c == 2048 and t != torch.float32)]


COLSUM_CASES = {  # name: n_seg, rows_per_seg, n, per_seg
    "geglu_bias": (1, 40, 10240, False), "conv_out": (1, 128, 4, False), "slice": (1, 100, 64, False), "short_segments": (6, 5, 40, True),
    "many_segments": (1500, 8, 64, False), "many_segments_per_seg": (1500, 8, 64, True)}


def test_cases_reach_the_branches_they_are_named_for():
    """CPU only: the restated launch rules put every case on the branch it is named for, and the source still states those rules"""
    for name, text in RULES_IN_SOURCE:
        assert _squeeze(text) in _squeeze((CSRC / name).read_text()), f"{name} no longer states: {text}"
    # attention: every DP instantiation, and both VALU widths
    assert {attn_dp(d) for d in DP_WIDTHS} | {attn_dp(d) for _, d in PROD_WIDTHS} == set(range(16, 161, 16))
    assert [d for d in DP_WIDTHS + [40] if d < attn_dp(d)] == [8, 24, 56, 72, 104, 136, 152, 40]         # head_dim < DP: guarded fragments
    assert all(d % 8 == 0 for d in DP_WIDTHS)
    assert {(d // epc(t) + 63) // 64 for _, t, d in WIDE} == {1, 2} and 320 // 4 == 80 and 512 > 160
    # GroupNorm
    n, c0, c1, h, w = GN_CASES["straddle"]
    assert gn_chunks(n, h * w) == (4, 9) and h * w - 3 * 9 == 8 and (c0 // GN_GROUPS) % 8 != 0 and (c0 // GN_GROUPS) % 4 != 0
    n, c0, c1, h, w = GN_CASES["two_sweeps"]
    assert gn_chunks(n, h * w) == (1, 4) and column_sweeps(c0 + c1, torch.bfloat16) == 2 and column_sweeps(c0 + c1, torch.float32) == 3
    assert (c0 + c1) // 8 == 320 and (c0 + c1) // 4 == 640
    n, c0, c1, h, w = GN_CASES["cap"]
    assert min(h * w // 8, (1024 + n - 1) // n) == 36 and gn_chunks(n, h * w) == (29, 10) and h * w - 28 * 10 == 9
    n, c0, c1, h, w = GN_CASES["concat"]
    cpg = (c0 + c1) // GN_GROUPS
    assert cpg == 30 and c0 % cpg != 0 and gn_chunks(n, h * w) == (2, 8)
    # LayerNorm
    for t in DTYPES:
        assert ln_launch(1, 320, t)[0] == 1 and ln_launch(3, 320, t)[0] == 1
        blocks = ln_launch(4099, 320, t)[0]
        per_wave = [len(range(wv, 4099, blocks * 4)) for wv in range(blocks * 4)]
        assert blocks == 512 and set(per_wave) == {2, 3}
        assert ln_launch(2051, 1280, t)[0] == 512 and 64 // epc(t) < 64
    assert ln_launch(9, 2560, torch.bfloat16)[1:] == (8, True) and ln_launch(9, 2048, torch.float32)[1:] == (8, True)
    assert [ln_launch(9, c, torch.bfloat16)[1] for c in (64, 320, 1280)] == [1, 1, 4] and [ln_launch(9, c, torch.float32)[1] for c in (64, 320, 1280)] == [1, 2, 8]
    assert not ln_launch(9, 4104, torch.bfloat16)[2] and 4104 % 8 == 0
    # column sums
    assert column_sweeps(10240, torch.bfloat16) == 5 and column_sweeps(10240, torch.float32) == 10
    assert colsum_chunks(1, 40) == (5, 8) and colsum_chunks(6, 5) == (1, 5) and colsum_chunks(1500, 8) == (1, 8) and colsum_chunks(1, 100) == (12, 9)


# ------------------------------------------------------------------------------------------------ attention
@functools.lru_cache(maxsize=None)
def attn_case(heads, d, segs, dtype, seed=40, dominate=False):
    """dtype-rounded inputs, fp64 forward (out, log2-domain log-sum-exp) and fp64 autograd gradients.  Shared: do not write to it."""
    C_ = heads * d
    nq, nk = sum(s[0] for s in segs), sum(s[1] for s in segs)
    q, k, v, dout = rnd((nq, C_), seed, dtype), rnd((nk, C_), seed + 1, dtype), rnd((nk, C_), seed + 2, dtype), rnd((nq, C_), seed + 3, dtype)
    if dominate:        # a key late in the segment that is 6 x a query: the probabilities are recomputed against a large log-sum-exp
        k[nk - 10] = (6.0 * q[17]).to(dtype).float()
    with torch.enable_grad():
        qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
        outs, lses, q0, k0 = [], [], 0, 0
        for ql, kl in segs:
            qq = qd[q0:q0 + ql].view(ql, heads, d).transpose(0, 1)
            kk = kd[k0:k0 + kl].view(kl, heads, d).transpose(0, 1)
            vv = vd[k0:k0 + kl].view(kl, heads, d).transpose(0, 1)
            s = qq @ kk.transpose(1, 2) * d ** -0.5
            outs.append((torch.softmax(s, dim=-1) @ vv).transpose(0, 1).reshape(ql, C_))
            lses.append(torch.logsumexp(s.detach(), -1) / math.log(2))
            q0, k0 = q0 + ql, k0 + kl
        out = torch.cat(outs)
        gq, gk, gv = torch.autograd.grad(out, (qd, kd, vd), dout.double())
    return dict(heads=heads, d=d, segs=segs, q=q, k=k, v=v, dout=dout, out=out.detach(), lse=torch.cat(lses, 1), gq=gq, gk=gk, gv=gv)


def attn_device(c, dtype):
    """q / k / v on the device: column slices of one fused [tokens, 3C] projection when the lengths allow it, else q alone and k / v as
    slices of a fused [kv tokens, 2C] projection"""
    C_ = c["heads"] * c["d"]
    if c["q"].shape[0] == c["k"].shape[0]:
        x = torch.cat([c["q"], c["k"], c["v"]], 1).to(dtype).cuda()
        return x[:, :C_], x[:, C_:2 * C_], x[:, 2 * C_:]
    kv = torch.cat([c["k"], c["v"]], 1).to(dtype).cuda()
    return c["q"].to(dtype).cuda(), kv[:, :C_], kv[:, C_:]


def check_attention(ops, c, dtype, host_forward=False, what=""):
    """backward against fp64 autograd; the saved statistics from the forward kernel, or (host_forward) `out` rounded to the dtype and the
    log-sum-exp from the fp64 forward on the host, so that the backward kernel is judged alone"""
    heads, d, segs = c["heads"], c["d"], c["segs"]
    q_lens, kv_lens = [s[0] for s in segs], [s[1] for s in segs]
    seg = ops.make_segments(q_lens, kv_lens)
    qg, kg, vg = attn_device(c, dtype)
    if host_forward:
        out, lse = c["out"].to(dtype).cuda(), c["lse"].float().cuda()
    else:
        lse = torch.zeros(heads, sum(q_lens), device="cuda")
        out = ops.attention(qg, kg, vg, heads, d, seg, max(q_lens), lse=lse)
        e_out = float((out.double().cpu() - c["out"]).norm() / c["out"].norm())
        e_lse = float((lse.double().cpu() - c["lse"]).abs().max())
        assert e_out < TOL[dtype] * 3 and e_lse < (1e-4 if dtype == torch.float32 else 2e-2), (what, e_out, e_lse)
    dq, dk, dv = ops.attention_bwd(qg, kg, vg, out, c["dout"].to(dtype).cuda(), lse, heads, d, seg, max(q_lens), max(kv_lens))
    for g, r, nm in ((dq, c["gq"], "dq"), (dk, c["gk"], "dk"), (dv, c["gv"], "dv")):
        close_grad(g, r, dtype, "attn", what=f"{what} {nm}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", DP_WIDTHS)
def test_attention_backward_every_head_width(ops, d, dtype):
    """every attention_bwd_kernel<T, DP, MODE> instantiation (with the production widths below: DP = 16 ... 160), half of them with
    head_dim < DP (guarded fragments, zeroed transpose-read columns), over segments around the 128-row and 64-row tile boundaries"""
    check_attention(ops, attn_case(2, d, DP_SEGS, dtype), dtype, what=f"d{d}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("heads,d", PROD_WIDTHS, ids=["d40", "d64"])
def test_attention_backward_ragged_production_widths(ops, heads, d, dtype):
    check_attention(ops, attn_case(heads, d, PROD_SEGS, dtype, seed=50), dtype, what=f"d{d} ragged")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attention_backward_dominating_key(ops, dtype):
    c = attn_case(2, 64, ((300, 300),), dtype, seed=60, dominate=True)
    assert float(c["lse"].max()) > 40          # log2 domain: the recomputed exponent's two terms are both large
    check_attention(ops, c, dtype, what="dominating key")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", [40, 64])
@pytest.mark.parametrize("longer", [False, True], ids=["max_len_exact", "max_len_larger"])
def test_attention_backward_writes_stay_inside_the_segments(ops, d, dtype, longer):
    """dq | dk | dv into a column and row slice of a larger buffer prefilled with 7.0: guard columns beyond 3C (ld_dq > 3C), guard rows
    after the last token and a gap of unowned rows between two segments must still hold 7.0; every in-segment element is written"""
    heads, gap, tail = 2, 3, 5
    C_ = heads * d
    pad = 4 if dtype == torch.float32 else 12           # row strides need 8-byte (MFMA epilogue) / 16-byte (fp32) alignment only
    c = attn_case(heads, d, GUARD_SEGS, dtype, seed=70)
    n = c["q"].shape[0]
    # token rows with a gap after the first segment; rows of the gap and of the tail belong to no segment
    rows, q0, k0 = [], 0, 0
    for i, (ql, kl) in enumerate(GUARD_SEGS):
        rows.append([q0, ql, k0, kl])
        q0, k0 = q0 + ql + (gap if i == 0 else 0), k0 + kl + (gap if i == 0 else 0)
    seg = torch.tensor(rows, dtype=torch.int32, device="cuda")

    def spread(t, lens, fill=0.0):       # [n, cols] -> [n + gap + tail, cols] with the gap rows after the first segment
        o = torch.full((n + gap + tail, t.shape[1]), fill, dtype=t.dtype)
        o[:lens[0]] = t[:lens[0]]
        o[lens[0] + gap:n + gap] = t[lens[0]:]
        return o
    q_lens, kv_lens = [s[0] for s in GUARD_SEGS], [s[1] for s in GUARD_SEGS]
    x = torch.cat([spread(c["q"], q_lens), spread(c["k"], kv_lens), spread(c["v"], kv_lens)], 1).to(dtype).cuda()
    qg, kg, vg = x[:, :C_], x[:, C_:2 * C_], x[:, 2 * C_:]
    lse = spread(c["lse"].t().float(), q_lens).t().contiguous().cuda()
    out = spread(c["out"], q_lens).to(dtype).cuda()
    dout = spread(c["dout"], q_lens).to(dtype).cuda()
    buf = torch.full((n + gap + tail, 3 * C_ + pad), 7.0, dtype=dtype, device="cuda")
    extra = 200 if longer else 0
    ops.attention_bwd(qg, kg, vg, out, dout, lse, heads, d, seg, max(q_lens) + extra, max(kv_lens) + extra, dqkv=buf[:, :3 * C_])
    got = buf.float().cpu()
    assert bool((got[:, 3 * C_:] == 7.0).all()), "guard columns written"
    assert bool((got[n + gap:] == 7.0).all()), "guard rows after the last token written"
    for j, (lens, ref) in enumerate(((q_lens, c["gq"]), (kv_lens, c["gk"]), (kv_lens, c["gv"]))):
        blk = got[:, j * C_:(j + 1) * C_]
        assert bool((blk[lens[0]:lens[0] + gap] == 7.0).all()), ("rows between two segments written", "qkv"[j])
        close_grad(torch.cat([blk[:lens[0]], blk[lens[0] + gap:n + gap]]), ref, dtype, "attn", what=f"d{d} guarded d{'qkv'[j]}")


@pytest.mark.parametrize("case", WIDE, ids=[w[0] for w in WIDE])
def test_attention_backward_from_a_host_forward(ops, case):
    """attention_bwd_ref_kernel<T, 2> (f32, head_dim 320: 80 chunk columns) and <T, 1> behind the 16-bit head_dim > 160 branch (512): the
    forward kernel writes no log-sum-exp there, so `out` and the statistic come from the fp64 forward on the host -- and once at
    head_dim 64 per dtype, where the MFMA / f32 backward is then judged without the forward kernel"""
    _, dtype, d = case
    check_attention(ops, attn_case(2, d, WIDE_SEGS, dtype, seed=80), dtype, host_forward=True, what=case[0])


# ------------------------------------------------------------------------------------------------ GroupNorm
@functools.lru_cache(maxsize=None)
def gn_case(name, dtype, silu):
    n, c0, c1, h, w = GN_CASES[name]
    c = c0 + c1
    a = rnd((n, c0, h, w), 17, dtype, 1.5)
    b = rnd((n, c1, h, w), 18, dtype) if c1 else None
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=G(19)), 0.1 * torch.randn(c, generator=G(20))
    dy = rnd((n, c, h, w), 21, dtype)
    with torch.enable_grad():
        leaves = [t.double().requires_grad_() for t in ((a, b) if c1 else (a,))] + [gamma.double().requires_grad_(), beta.double().requires_grad_()]
        xin = torch.cat(leaves[:2], 1) if c1 else leaves[0]
        y = F.group_norm(xin, GN_GROUPS, leaves[-2], leaves[-1], 1e-5)
        y = F.silu(y) if silu else y
        grads = torch.autograd.grad(y, leaves, dy.double())
    return dict(a=a, b=b, gamma=gamma, beta=beta, dy=dy, ga=grads[0], gb=grads[1] if c1 else None, gg=grads[-2], gbeta=grads[-1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("name", list(GN_CASES))
def test_groupnorm_backward_edges(ops, name, silu, dtype):
    """chunks that straddle groups, second / third column sweeps with one slab, the slab cap with a ragged last slab, a group across the
    concat boundary: dx, dx2, dgamma, dbeta; a second call accumulates to 2 x; MVLDM_NORM_BWD_STORE overwrites a poisoned gradient"""
    from mv_ldm_amd import _lib as L
    k = gn_case(name, dtype, silu)
    c = k["gamma"].numel()
    xa, xb = nhwc(k["a"], dtype), (None if k["b"] is None else nhwc(k["b"], dtype))
    gam, bet, dyd = k["gamma"].cuda(), k["beta"].cuda(), nhwc(k["dy"], dtype)
    stats = torch.zeros(xa.shape[0], GN_GROUPS, 2, device="cuda")
    ops.groupnorm(xa, gam, bet, GN_GROUPS, 1e-5, silu, x2=xb, stats_out=stats)
    dg, db = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    dx, dx2 = ops.groupnorm_bwd(xa, dyd, gam, bet, stats, dg, db, GN_GROUPS, silu, x2=xb)
    close_grad(nchw(dx), k["ga"], dtype, "norm_dx", what=f"{name} dx")
    if xb is not None:
        close_grad(nchw(dx2), k["gb"], dtype, "norm_dx", what=f"{name} dx2")
    close_grad(dg, k["gg"], dtype, "param", what=f"{name} dgamma")
    close_grad(db, k["gbeta"], dtype, "param", what=f"{name} dbeta")
    dg1, db1 = dg.clone(), db.clone()
    ops.groupnorm_bwd(xa, dyd, gam, bet, stats, dg, db, GN_GROUPS, silu, x2=xb)           # accumulates: t + t, exactly
    close_grad(dg, 2 * k["gg"], dtype, "param", what=f"{name} 2 x dgamma")
    close_grad(db, 2 * k["gbeta"], dtype, "param", what=f"{name} 2 x dbeta")
    assert torch.equal(dg, 2 * dg1) and torch.equal(db, 2 * db1)
    pg, pb = torch.full((c,), 7.0, device="cuda"), torch.full((c,), float("nan"), device="cuda")
    ops.groupnorm_bwd(xa, dyd, gam, bet, stats, pg, pb, GN_GROUPS, int(silu) | L.NORM_BWD_STORE, x2=xb)
    assert torch.equal(pg, dg1) and torch.equal(pb, db1)           # written, not added; the same fixed summation order


# ------------------------------------------------------------------------------------------------ LayerNorm
@functools.lru_cache(maxsize=None)
def ln_case(rows, c, dtype):
    x, dy = rnd((rows, c), 22, dtype, 2.0), rnd((rows, c), 25, dtype)
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=G(23)), 0.1 * torch.randn(c, generator=G(24))
    with torch.enable_grad():
        xd, gd, bd = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
        gx, gg, gb = torch.autograd.grad(F.layer_norm(xd, (c,), gd, bd, 1e-5), (xd, gd, bd), dy.double())
    return dict(x=x, dy=dy, gamma=gamma, gx=gx, gg=gg, gb=gb)


def ln_bwd(ops, x, dy, gamma, dg, db, dx, store=False):
    """mvldm_layernorm_bwd through the C ABI: the status is returned, the store flag rides on the dtype tag"""
    from mv_ldm_amd import _lib as L
    c = x.shape[-1]
    ws = ops.workspace(512 * c * 2 * 4, x.device, "lnb")
    return L.load().mvldm_layernorm_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), gamma.data_ptr(), dg.data_ptr(), db.data_ptr(), x.numel() // c, c,
                                        1e-5, ops.dt(x) | (L.NORM_BWD_STORE if store else 0), ws.data_ptr(), ws.numel(), ops.stream())


@pytest.mark.parametrize("rows,c,dtype", LN_PARAMS)
def test_layernorm_backward_edges(ops, rows, c, dtype):
    """idle waves (rows < 4), 2-3 rows accumulated per wave with a ragged last pass (512 workgroups), fewer than 64 chunk columns,
    MAXCH = 8; dx, dgamma, dbeta; accumulate and store"""
    k = ln_case(rows, c, dtype)
    xg, dyd, gam = k["x"].to(dtype).cuda(), k["dy"].to(dtype).cuda(), k["gamma"].cuda()
    dg, db, dx = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda"), torch.full((rows, c), 7.0, dtype=dtype, device="cuda")
    assert ln_bwd(ops, xg, dyd, gam, dg, db, dx) == 0
    close_grad(dx, k["gx"], dtype, "norm_dx", what=f"{rows}x{c} dx")
    close_grad(dg, k["gg"], dtype, "param", what=f"{rows}x{c} dgamma")
    close_grad(db, k["gb"], dtype, "param", what=f"{rows}x{c} dbeta")
    dg1, db1 = dg.clone(), db.clone()
    assert ln_bwd(ops, xg, dyd, gam, dg, db, dx) == 0
    close_grad(dg, 2 * k["gg"], dtype, "param", what=f"{rows}x{c} 2 x dgamma")
    assert torch.equal(dg, 2 * dg1) and torch.equal(db, 2 * db1)
    pg, pb = torch.full((c,), 7.0, device="cuda"), torch.full((c,), float("nan"), device="cuda")
    assert ln_bwd(ops, xg, dyd, gam, pg, pb, dx, store=True) == 0
    assert torch.equal(pg, dg1) and torch.equal(pb, db1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_layernorm_backward_refuses_more_than_512_chunk_columns(ops, dtype):
    """c = 4104 = 513 chunks of 8: a status, and nothing launched -- dx, dgamma, dbeta keep their poison"""
    from mv_ldm_amd import _lib as L
    rows, c = 5, 4104
    xg, dyd = rnd((rows, c), 26, dtype).to(dtype).cuda(), rnd((rows, c), 27, dtype).to(dtype).cuda()
    dg, db, dx = torch.full((c,), 7.0, device="cuda"), torch.full((c,), 7.0, device="cuda"), torch.full((rows, c), 7.0, dtype=dtype, device="cuda")
    rc = ln_bwd(ops, xg, dyd, torch.ones(c, device="cuda"), dg, db, dx)
    assert rc != 0 and b"layernorm_bwd: c=4104" in L.load().mvldm_last_error()
    torch.cuda.synchronize()
    assert bool((dg == 7.0).all()) and bool((db == 7.0).all()) and bool((dx == 7.0).all())
    with pytest.raises(RuntimeError, match="layernorm_bwd: c=4104"):
        ops.layernorm_bwd(xg, dyd, torch.ones(c, device="cuda"), dg, db)


# ------------------------------------------------------------------------------------------------ column sums
@functools.lru_cache(maxsize=None)
def colsum_case(name, dtype):
    n_seg, rps, n, per_seg = COLSUM_CASES[name]
    rows = n_seg * rps
    ld = {"conv_out": epc(dtype), "slice": 192}.get(name, n)            # conv_out: 4 real columns in a 16-byte chunk; slice: columns [64, 128)
    x = rnd((rows, ld), 90, dtype)
    col0 = 64 if name == "slice" else 0
    real = x[:, col0:col0 + n].double()
    return dict(x=x, col0=col0, ref=real.view(n_seg, rps, n).sum(1) if per_seg else real.sum(0))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(COLSUM_CASES))
def test_colsum_edges(ops, name, dtype):
    """5 / 10 column sweeps, a 4-column sum inside a padded chunk, a column slice (ld > n), segments shorter than 8 rows, many one-chunk
    segments: written and accumulated, neighbours of the destination untouched, twice bit-identical (fixed summation order)"""
    n_seg, rps, n, per_seg = COLSUM_CASES[name]
    k = colsum_case(name, dtype)
    xg = k["x"].to(dtype).cuda()[:, k["col0"]:]
    xg = xg[:, :n] if name == "slice" else xg              # conv_out keeps its padded width: n is passed
    results = []
    for accumulate in (False, True):
        for _ in range(2):
            base = 1.5 if accumulate else 7.0              # accumulate: added to; else: poison that must be overwritten
            if per_seg:
                dst = torch.full((n_seg, n + 8), base, device="cuda")       # destination row stride wider than n
                ops.colsum(xg, dst, rows_per_seg=rps, per_seg=True, accumulate=accumulate, n=n)
                got, rest = dst[:, :n], dst[:, n:]
            else:
                dst = torch.full((n + 4,), base, device="cuda")
                ops.colsum(xg, dst[:n], rows_per_seg=rps, accumulate=accumulate, n=n)
                got, rest = dst[:n], dst[n:]
            assert bool((rest == base).all()), "neighbours of the destination written"
            close_grad(got, k["ref"] + (base if accumulate else 0.0), dtype, "param", what=f"{name} accumulate={accumulate}")
            results.append(got.clone())
    assert torch.equal(results[0], results[1]) and torch.equal(results[2], results[3])


# ------------------------------------------------------------------------------------------------ elementwise, loss
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gelu_backward(ops, dtype):
    """MVLDM_TE_GELU_BWD (the ViT feed-forward of the standard path) with the pre-activation in the activation dtype and in fp32"""
    from mv_ldm_amd import _lib as L
    rows, d = 77, 1280
    x, dy = rnd((rows, d), 91, dtype, 2.0), rnd((rows, d), 92, dtype)
    xd = x.double().requires_grad_()
    (gx,) = torch.autograd.grad(F.gelu(xd), xd, dy.double())
    for xin in (x.to(dtype).cuda(), x.cuda()):
        out = torch.full((rows, d), 7.0, dtype=dtype, device="cuda")
        ops.train_eltwise(L.TE_GELU_BWD, xin, dy.to(dtype).cuda(), out, 1, rows * d)
        close_grad(out, gx, dtype, "eltwise", what=f"gelu_bwd x {xin.dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,D", [(77, 8), (9, 5120)], ids=["D8", "D5120"])
def test_geglu_edges(ops, rows, D, dtype):
    """one 16-byte chunk per half (two in f32), and the production width"""
    ag, dh = rnd((rows, 2 * D), 93, dtype), rnd((rows, D), 94, dtype)
    agd = ag.double().requires_grad_()
    h = agd[:, :D] * F.gelu(agd[:, D:])
    (gag,) = torch.autograd.grad(h, agd, dh.double())
    agg = ag.to(dtype).cuda()
    close_grad(ops.geglu_fwd(agg), h, dtype, "eltwise", what="geglu_fwd")
    close_grad(ops.geglu_bwd(agg, dh.to(dtype).cuda()), gag, dtype, "eltwise", what="geglu_bwd")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 6, 10, 8), (1, 4, 2, 1280)], ids=["6x10x8", "4x2x1280"])
def test_resampling_on_non_square_maps(ops, shape, dtype):
    n, h, w, c = shape
    du = rnd(shape, 95, dtype)
    close_grad(ops.pool2x2_sum(du.to(dtype).cuda()), du.double().view(n, h // 2, 2, w // 2, 2, c).sum((2, 4)), dtype, "eltwise", l2=TOL[dtype], what="pool2x2_sum")
    z = ops.zero_insert2x(du.to(dtype).cuda()).float().cpu()
    assert z.shape == (n, 2 * h, 2 * w, c) and torch.equal(z[:, ::2, ::2], du)
    assert float(z[:, 1::2].abs().max()) == 0 and float(z[:, :, 1::2].abs().max()) == 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_add_noise_and_mse_loss_with_a_16_bit_destination(ops, dtype):
    """what the bf16 / f16 trainers pass: the fp32 result rounded ONCE to the destination's type"""
    from mv_ldm_amd import _lib as L
    lib = L.load()
    n, c, h = 6, 4, 8
    g = G(96)
    x0, noise = torch.randn(n, c, h, h, generator=g).cuda(), torch.randn(n, c, h, h, generator=g).cuda()
    coef = torch.rand(n, 2, generator=g).cuda()
    rows = torch.tensor([7, 1, 2, 3, 4, 0], dtype=torch.int32, device="cuda")
    dst = {}
    for t in (torch.float32, dtype):
        dst[t] = torch.full((8, h, h, 16), 7.0, dtype=t, device="cuda")
        L.check(lib.mvldm_add_noise(x0.data_ptr(), noise.data_ptr(), coef.data_ptr(), dst[t].data_ptr(), n, c, h * h, 16, 4, ops.dt(t), rows.data_ptr(), ops.stream()))
    assert torch.equal(dst[dtype], dst[torch.float32].to(dtype))
    assert bool((dst[dtype][..., :4] == 7.0).all()) and bool((dst[dtype][..., 8:] == 7.0).all()) and bool((dst[dtype][[5, 6]] == 7.0).all())
    assert bool((dst[dtype][rows.long()][..., 4:8] != 7.0).any())
    # the loss gradient of the target images, scaled like a half-weighted micro-batch
    n_img, n_tgt = 5, 3
    pred, tgt_noise = torch.randn(n_img, h, h, c, generator=g).cuda(), torch.randn(n_tgt, c, h, h, generator=g).cuda()
    tgt_img = torch.tensor([1, 3, 4], dtype=torch.int32, device="cuda")
    ws = torch.zeros(256, dtype=torch.float64, device="cuda")
    dpred, loss = {}, {}
    for t in (torch.float32, dtype):
        dpred[t], loss[t] = torch.zeros(n_img, h, h, 8, dtype=t, device="cuda"), torch.zeros(1, device="cuda")
        L.check(lib.mvldm_mse_loss(pred.data_ptr(), tgt_noise.data_ptr(), tgt_img.data_ptr(), n_tgt, h * h, c, loss[t].data_ptr(), 0, 0.5,
                                   dpred[t].data_ptr(), 8, ops.dt(t), 0.5, ws.data_ptr(), ops.stream()))
    pd = pred.double().cpu().requires_grad_()
    ref_loss = F.mse_loss(pd[tgt_img.long().cpu()].permute(0, 3, 1, 2), tgt_noise.double().cpu())
    (gp,) = torch.autograd.grad(ref_loss, pd)
    assert torch.equal(loss[dtype], loss[torch.float32]) and abs(float(loss[dtype]) - 0.5 * float(ref_loss)) < 1e-6 * float(ref_loss)
    assert torch.equal(dpred[dtype], dpred[torch.float32].to(dtype))
    assert float(dpred[dtype][..., 4:].float().abs().max()) == 0 and float(dpred[dtype][[0, 2]].float().abs().max()) == 0
    close_grad(dpred[torch.float32][..., :4], 0.5 * gp, torch.float32, "eltwise", l2=1e-6, what="mse gradient")
