"""GPU parity of the GLUE kernels at their edges: what runs between the GEMM / attention / norm kernels in every training step and every
sampler step -- csrc/train_misc.hip (gradient norm, clip coefficient, AdamW, EMA, loss scaler, MSE loss, noise injection, elementwise
backward ops, 2x2 pooling, zero insertion) and csrc/misc.hip (DDIM / DDPM step, step counter, layout conversion, posterior sample,
timestep embedding, eltwise, gather_rows).  The third edge suite, after test_hip_forward_edges.py and test_hip_backward_edges.py: the
unit tests of these kernels stop three to six orders of magnitude below the sizes at which they take their unrolled loop or a second
grid-stride pass; the cases here are the smallest that do.

References: plain torch on the CPU in fp64 from the SAME inputs, or the exact fp32 expression where the kernel claims bit-identity.
Destinations are slices of larger buffers with guard fills (7.0, or -7.0 / 7 for statistics and records) that must be bit-identical
after the launch.  Bounds: exact where the kernel's comment claims it or the arithmetic makes it so; units in the last place of fp32
where derived below; `TOL` of test_hip_ops.py (imported, not restated) for the approximate-math kernels.  Every bounded value goes to
conftest.record_err; tests/golden/measured_errors_glue_edges.json is one MVLDM_TEST_REPORT run on an MI355X.

Only the CPU tests (the helpers' self-test, the launch rules, the sumsq index walk, the planted positions, the loss scaler's stand-in)
are unmarked; every other test carries the gpu mark.

Derived bounds
  * sum of squares: fp32 x fp32 products are exact in fp64; the accumulation error of 8.4 M fp64 terms is below 1e-9 relative, far below
    2^-24 -- norm_out[0] and norm_out[2] within 1 unit in the last place of the fp64 value.  Integer gradients in [-2, 2] whose sum of
    squares stays below 2^24: every product, the fp64 sum and the fp32 norm_out[2] are exact, so norm_out[2] EQUALS the count.
  * AdamW m, v: 2 units in the last place of the fp64 value formed from the fp32 gi = g * gs (the kernel's first operation, restated):
    two rounded products and one rounded sum.  That holds where the two terms do not cancel, so m0 carries the sign of g in these
    inputs (v's terms are never negative), and v0 is either zero or well above (1 - b2) gi^2.  The hyper-parameters are fp32-representable
    numbers, so the kernel, the stand-in and the fp64 reference are handed the same values.
  * AdamW update p_new - p_old: relative L2 against fp64, at most 2 x the same error of the stand-in (tests/torch_optimizer_ops.py) on
    the same inputs.  No bound is chosen in advance: the stand-in's own fp32 rounding sets it, and the margin of 2 covers the different
    operation order, step_size * (m / (sqrt(v) * inv_sqrt_bc2 + eps)) against addcdiv_ with -lr / bc1.
  * EMA: the average and the parameter lie within a factor of two of each other (as a parameter and its running average do), so p - avg
    is exact (Sterbenz) and one rounding is left: 1 unit in the last place against fp64 and against avg.lerp_(p, w).

Where a case could not stay on the branch first planned for it (the CPU test asserts each of these):
  * the vector AdamW kernel at n = 4 x (2 097 152 + 1024) runs 1025 workgroups of 7 to 8 passes each, not more workgroups than the 8192 cap:
    grid_for(n / 4, 2048) reaches the cap only above 16.7 M vectors (1 GB of operands), out of scope here.  The size is kept: it is the
    largest, and the only one with a ragged last pass over more than a thousand workgroups;
  * the MSE shape n_tgt = 3, hw = 61 x 97, c = 4 has 71 004 elements (1.08 passes of the 65 536 threads, the second one ragged), not
    213 012; hw = 183 x 97 has the 213 012 (3.25 passes) and is run as well.

Found by this module: mse_kernel<f16> did not round the fp32 product grad_scale x 2 (pred - noise) / N [x S] to f16, as its contract says
and as the f32 and bf16 instantiations do: the compiler folded multiply and conversion into v_fma_mixlo_f16, which rounds the EXACT product
once -- the neighbouring f16 number in 5 of 71 004 and 15 of 213 012 elements (where the fp32 product lands on an f16 tie; the 768 elements
of the older tests never hit one).  The product is pinned to an fp32 register now.  mvldm_grad_norm cast `g` to 16-byte vectors without
requiring the alignment; it is an MVLDM_ERR_ARG now.  amp_update_kernel and torch._amp_update_scale_ differ for a growth tracker at or above the interval (the kernel
grows at once, torch never again); the kernel's >= stays and the stand-in clamps the tracker (both docstrings say so).
"""
import functools
import math
from collections import Counter
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import record_err
from test_hip_forward_edges import NAME, _squeeze, check_guard, close       # the forward suite's helpers: the same conventions
from test_hip_ops import TOL, G                                             # the project's bounds, imported
from torch_optimizer_ops import TorchOptimizerOps

gpu = pytest.mark.gpu
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
CSRC = Path(__file__).resolve().parent.parent / "mv_ldm_amd" / "csrc"
GUARD = 1024                # elements of fill on either side of a flat destination (a multiple of every 16-byte chunk)
ERR_ARG = -1                # include/mvldm.h MVLDM_ERR_ARG


@pytest.fixture(scope="module")
def ops():
    from mv_ldm_amd import ops as O
    from mv_ldm_amd import _lib as L
    L.load()
    return O


def epc(dtype):
    return 4 if dtype == F32 else 8


def f32r(x):
    """the fp32 number nearest to x, as a Python float: what a `float` parameter of the C ABI receives"""
    return float(torch.tensor(x, dtype=torch.float64).float())


def t32(x):
    return torch.tensor(x, dtype=F32)


def urnd(shape, seed, dtype, lo=-2.0, hi=2.0):
    """uniform fp32 values already representable in `dtype`: bounded, so the worst element over the RMS stays a rounding question"""
    return (torch.rand(shape, generator=G(seed)) * (hi - lo) + lo).to(dtype).float()


# ------------------------------------------------------------------------------------------------ helpers
def flat_guarded(n, dtype, fill=7.0, lead=GUARD, device="cuda"):
    """a flat buffer of `fill` and the n elements of it that the kernel owns, `lead` elements in"""
    buf = torch.full((lead + n + GUARD,), fill, dtype=dtype, device=device)
    return buf, buf[lead:lead + n]


def flat_owned(buf, n, lead=GUARD):
    m = torch.zeros(buf.shape, dtype=torch.bool)
    m[lead:lead + n] = True
    return m


def bit_equal(got, ref, what=""):
    """every element equal (NaN matches NaN); same shape and dtype"""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    same = (got == ref) | ((got != got) & (ref != ref))
    if not bool(same.all()):
        bad = (~same).nonzero()
        at = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {list(at)}: got {got[at].item()!r}, want {ref[at].item()!r}")


def ulp32(x):
    """the spacing of fp32 numbers at float32(x), per element of an fp64 tensor (2^-149 at zero and in the denormal range)"""
    r = x.double().float().double().abs()
    _, e = torch.frexp(r)                                      # r = m 2^e, m in [0.5, 1): the spacing is 2^(e - 24)
    e = torch.where(r == 0, torch.full_like(e, -200), e)
    return torch.ldexp(torch.ones_like(r), (e - 24).clamp_min(-149))


def ordinal32(x):
    """fp32 numbers in their order as integers: neighbours differ by one"""
    i = x.contiguous().view(torch.int32).long()
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def within_ulp(got, ref, k, kind, what=""):
    """fp32 `got` within k units in the last place of `ref`, element by element.  ref in fp64: |got - ref| over the spacing of fp32 at ref;
    ref in fp32: how many representable numbers apart the two are.  The worst element goes to record_err"""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape and got.dtype == F32, (what, got.shape, ref.shape, got.dtype)
    assert bool(torch.isfinite(got).all()), f"{kind} {what}: non-finite output"
    err = (ordinal32(got) - ordinal32(ref)).abs().double() if ref.dtype == F32 else (got.double() - ref.double()).abs() / ulp32(ref.double())
    worst = float(err.max()) if err.numel() else 0.0
    if kind is not None:
        record_err(f"{kind}/ulp", worst)
    print(f"within_ulp {kind} {what}: worst {worst:.3f} units in the last place (bound {k})")
    assert worst <= k, f"{kind} {what}: {worst:.3f} units in the last place at {int(err.argmax())} (bound {k})"


def exact_sum(got, grad, what=""):
    """norm_out[2] of integer gradients EQUALS the count: every product and sum is exact below 2^24"""
    want = int((grad.double() ** 2).sum())
    assert want < 2 ** 24, (what, want)
    assert float(got) == float(want), f"{what}: sum of squares {float(got)!r}, exact count {want} (off by {float(got) - want:+.0f})"


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def test_the_checks_can_fail():
    """CPU: every comparison helper raises on one flipped guard element / one element off by one unit in the last place (one unit beyond
    the bound for the k-unit check) / one element counted twice in the exact sum"""
    for dtype, fill, flip in ((BF16, 7.0, 0.0625), (F32, 7.0, 1e-6), (F32, -7.0, 1e-6), (torch.int32, 7, 1), (torch.int64, -5, 1)):
        buf, view = flat_guarded(40, dtype, fill, device="cpu")
        view.fill_(1)
        own = flat_owned(buf, 40)
        check_guard(buf, own, fill)
        for at in (0, GUARD - 1, GUARD + 40, len(buf) - 1):             # first / last element of the leading and of the trailing guard
            bad = buf.clone()
            bad[at] += flip
            with pytest.raises(AssertionError, match="guard elements written"):
                check_guard(bad, own, fill, "selftest")
    for dtype in DTYPES + [torch.int32]:
        ref = (torch.randn(33, 40, generator=G(1)) * 100).to(dtype)
        bit_equal(ref.clone(), ref, "selftest")
        off = ref.clone()
        off.view(torch.int32 if off.element_size() == 4 else torch.int16)[17, 23] += 1               # the next representable number
        with pytest.raises(AssertionError, match="1 of 1320 elements differ"):
            bit_equal(off, ref, "selftest")
    ref = torch.randn(1000, generator=G(2)).double() * torch.logspace(-45, 30, 1000, dtype=torch.float64)     # denormals to 1e30, exact in fp32
    ref = ref.float().double()
    up = lambda t, k: functools.reduce(lambda a, _: torch.nextafter(a, t32(float("inf"))), range(k), t)
    ref[501], ref[10] = 1.5, 2.0 ** -140                                # a normal and a denormal number
    for k in (1, 2):
        for r in (ref, ref.float()):                                     # against fp64 and against fp32
            within_ulp(ref.float(), r, k, None, "selftest")
            for at in (501, 10):
                edge = ref.float().clone()
                edge[at] = up(edge[at], k)
                within_ulp(edge, r, k, None, "selftest")                 # AT the bound passes
                off = ref.float().clone()
                off[at] = up(off[at], k + 1)
                with pytest.raises(AssertionError, match="units in the last place"):
                    within_ulp(off, r, k, None, "selftest")
    assert float(ulp32(torch.tensor([1.0], dtype=torch.float64))) == 2.0 ** -23 and float(ulp32(torch.tensor([0.0], dtype=torch.float64))) == 2.0 ** -149
    assert float(ulp32(torch.tensor([1.9999], dtype=torch.float64))) == 2.0 ** -23 and float(ulp32(torch.tensor([2.0 ** -130], dtype=torch.float64))) == 2.0 ** -149
    # the exact sum: one element counted twice, one dropped
    g = int_grad(3145729)["g"]
    count = float((g.double() ** 2).sum())
    exact_sum(t32(count), g)
    k = int(g.ne(0).nonzero()[0])
    for wrong in (count + float(g[k]) ** 2, count - float(g[k]) ** 2):
        with pytest.raises(AssertionError, match="exact count"):
            exact_sum(t32(wrong), g, "selftest")
    # the forward suite's close, as used here
    ref = urnd((33, 40), 3, BF16).double()
    close(ref.clone(), ref, BF16, None, "selftest")
    for factor, ok in ((0.5, True), (1.01, False)):                      # one element off by the bound TOL sets for the worst element
        off = ref.clone()
        off[3, 3] += factor * TOL[BF16][1] * ref.pow(2).mean().sqrt()
        if ok:
            close(off, ref, BF16, None, "selftest")
        else:
            with pytest.raises(AssertionError, match="worst element"):
                close(off, ref, BF16, None, "selftest")


# ------------------------------------------------------------------------------------------------ launch rules, restated
# The cases below are named for the loop or the pass they reach.  The host-side rules that decide it are restated here and the source is
# required to still state them (as RULES_IN_SOURCE of test_hip_forward_edges.py): a later change of a rule fails the CPU test instead of
# silently moving a case off its branch.
NORM_BLOCKS, LOSS_BLOCKS, GRID_CAP = 1024, 256, 8192
RULES_IN_SOURCE = [
    ("train_misc.hip", "constexpr int kNormBlocks = 1024;"),
    ("train_misc.hip", "constexpr int kLossBlocks = 256;"),
    ("train_misc.hip", "static inline int grid_for(size_t n, int per = 256) { return (int)std::min<size_t>((n + per - 1) / per, 8192); }"),
    ("misc.hip", "static inline int grid_for(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 8192); }"),
    ("train_misc.hip", "const bool vec = n % 4 == 0 && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;"),
    ("train_misc.hip", "hipLaunchKernelGGL(nt ? adamw_kernel4<true> : adamw_kernel4<false>, dim3(grid_for(n / 4, 2048)), dim3(256)"),
    ("train_misc.hip", "hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(n, 1024)), dim3(256)"),
    ("train_misc.hip", "hipLaunchKernelGGL(ema_kernel, dim3(grid_for(n, 1024)), dim3(256)"),
    ("train_misc.hip", "const size_t n4 = n / 4, step = (size_t)gridDim.x * 256;"),
    ("train_misc.hip", "for (; i + 3 * step < n4; i += 4 * step) {"),
    ("train_misc.hip", "for (; i < n4; i += step) {"),
    ("train_misc.hip", "if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) { const float v = g[n4 * 4 + threadIdx.x]; acc += (double)v * v; }"),
    ("train_misc.hip", "hipLaunchKernelGGL(sumsq_kernel, dim3(kNormBlocks), dim3(256)"),
    ("train_misc.hip", "MVLDM_REQUIRE(n < 4 || ((uintptr_t)g & 15) == 0,"),
    ("train_misc.hip", "hipLaunchKernelGGL(mse_kernel<T>, dim3(kLossBlocks), dim3(256)"),
    ("train_misc.hip", "if (successful >= interval) {"),
    ("train_misc.hip", "(silu_bwd_kernel<TX, T>), dim3(grid_for(n)), dim3(256)"),
    ("train_misc.hip", "(gelu_bwd_kernel<TX, T>), dim3(grid_for(n)), dim3(256)"),
    ("train_misc.hip", "hipLaunchKernelGGL(add_kernel<T>, dim3(grid_for(n / epc)), dim3(256)"),
    ("train_misc.hip", "hipLaunchKernelGGL(geglu_fwd_kernel<T>, dim3(grid_for(n / epc)), dim3(256)"),
    ("train_misc.hip", "hipLaunchKernelGGL(geglu_bwd_kernel<T>, dim3(grid_for(n / epc)), dim3(256)"),
    ("train_misc.hip", "hipLaunchKernelGGL(pool2x2_kernel<T>, dim3(grid_for((size_t)n_img * h * w * (c / epc))), dim3(256)"),
    ("train_misc.hip", "hipLaunchKernelGGL(zero_insert_kernel<T>, dim3(grid_for((size_t)n_img * 4 * h * w * (c / epc))), dim3(256)"),
    ("train_misc.hip", "hipLaunchKernelGGL(add_noise_kernel<T>, dim3(grid_for((size_t)n * c * hw)), dim3(256)"),
    ("misc.hip", "hipLaunchKernelGGL(posterior_sample_kernel, dim3(grid_for(total)), dim3(256)"),
    ("misc.hip", "hipLaunchKernelGGL((eltwise_kernel<TS, TD>), dim3(grid_for(n)), dim3(256)"),
    ("misc.hip", "hipLaunchKernelGGL(ddim_kernel<T>, dim3(grid_for(total)), dim3(256)"),
    ("misc.hip", "hipLaunchKernelGGL(ddpm_kernel, dim3(grid_for(n)), dim3(256)"),
    ("misc.hip", "hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for((size_t)n_rows * cpr)), dim3(256)"),
    ("misc.hip", "hipLaunchKernelGGL(nchw_to_nhwc_kernel<T>, dim3(grid_for(total)), dim3(256)"),
    ("misc.hip", "hipLaunchKernelGGL(nhwc_to_nchw_kernel<T>, dim3(grid_for(total)), dim3(256)"),
    ("misc.hip", "hipLaunchKernelGGL(ddim_advance_kernel, dim3(1), dim3(64)"),
    ("misc.hip", "const int64_t t = t_table[next < n_steps ? next : n_steps - 1];"),
    ("misc.hip", "const int step = min(max(*step_ptr, 0), n_steps - 1);"),
]


def grid_for(items, per=256):
    return min((items + per - 1) // per, GRID_CAP)


def adamw_is_vector(n, offsets):
    """adamw_run's rule, for buffers whose bases are 16-byte aligned and that start `offsets` floats in (p, g, m, v)"""
    return n % 4 == 0 and all(4 * o % 16 == 0 for o in offsets)


def sumsq_walk(n):
    """sumsq_kernel's index walk over the 16-byte vectors of n floats, thread by thread -> how many threads enter the unrolled loop, how
    often, how many remainder passes each takes, how often every vector is read, and which loop reads it (1 unrolled, 2 remainder)"""
    n4, step = n // 4, NORM_BLOCKS * 256
    i = np.arange(step, dtype=np.int64)
    visits, region = np.zeros(n4, dtype=np.int16), np.zeros(n4, dtype=np.int8)
    unrolled, rem = np.zeros(step, dtype=np.int64), np.zeros(step, dtype=np.int64)
    while True:
        live = i + 3 * step < n4
        if not live.any():
            break
        for k in range(4):
            visits[i[live] + k * step] += 1
            region[i[live] + k * step] = 1
        unrolled += live
        i = np.where(live, i + 4 * step, i)                 # a thread that failed the test once never passes it again: i only grows
    while True:
        live = i < n4
        if not live.any():
            break
        visits[i[live]] += 1
        region[i[live]] = 2
        rem += live
        i = np.where(live, i + step, i)
    return dict(entered=int((unrolled > 0).sum()), unrolled=Counter(unrolled.tolist()), rem=Counter(rem.tolist()), visits=visits, region=region,
                tail=n - 4 * n4, last_unrolled=int(np.flatnonzero(region == 1).max()) if (region == 1).any() else None,
                first_rem=int(np.flatnonzero(region == 2).min()) if (region == 2).any() else None)


STEP = NORM_BLOCKS * 256
SUMSQ_CASES = {       # n: threads that enter the unrolled loop, {unrolled passes: threads}, {remainder passes: threads}, scalar tail
    3145729: (0, {0: STEP}, {3: STEP}, 1),                              # one element short of the unrolled loop
    3145734: (1, {1: 1, 0: STEP - 1}, {0: 1, 3: STEP - 1}, 2),          # thread 0 alone enters it
    6295459: (STEP, {1: STEP}, {3: 1000, 2: STEP - 1000}, 3),           # one unrolled pass, then two or three remainder passes
    8388608: (STEP, {2: STEP}, {0: STEP}, 0),                           # two unrolled passes, nothing else
}
INF_N = 6295459       # the size with all three regions: where a non-finite value is planted, as (vector, lane) or the last element
INF_AT = {"unrolled": 2 * STEP + 17, "remainder": 4 * STEP + 33, "nan_unrolled": 3 * STEP + 5}


@functools.lru_cache(maxsize=None)
def walk(n):
    return sumsq_walk(n)


def planted(n):
    """element indices that the exact check must not leave zero: the last vector of the unrolled region, the first of the remainder,
    every tail element"""
    w = walk(n)
    at = []
    for vec in (w["last_unrolled"], w["first_rem"]):
        if vec is not None:
            at += [4 * vec + lane for lane in range(4)]
    return at + list(range(n - w["tail"], n))


INT_SEED = 20250


@functools.lru_cache(maxsize=None)
def int_grad(n):
    """integers in [-2, 2], half of them zeroed (generator seed INT_SEED + n % 1000): the sum of squares is about n, below 2^24 at every
    size here.  The planted positions get +-1 / +-2 in turn."""
    g = G(INT_SEED + n % 1000)
    v = torch.randint(-2, 3, (n,), generator=g).float() * (torch.rand(n, generator=g) < 0.5)
    at = planted(n)
    v[at] = torch.tensor([(2.0, -1.0, 1.0, -2.0)[k % 4] for k in range(len(at))])
    return dict(g=v, planted=at, count=int((v.double() ** 2).sum()))


@functools.lru_cache(maxsize=None)
def real_grad(n):
    g = torch.randn(n, generator=G(3000 + n % 997)) * 1e-2
    return dict(g=g, sumsq=(g.double() ** 2).sum())


# shapes of the "second pass" cases: work items above blocks x 256 threads and no multiple of 256
HW2 = 323 * 325                                 # x 5 images x 4 channels = 2 099 500 work items
N2 = 5 * 4 * HW2
ELT2 = 2 ** 21 + 1                              # the smallest count above 8192 x 256 that is no multiple of 256
GEGLU2 = (699051, 3)                            # rows x chunks per row = 2^21 + 1
POOL2 = (3, 43, 5419, 3)                        # n_img, h, w (of the pooled map), chunks per pixel: 2^21 + 1 output chunks
ZERO2 = (1, 3, 174763, 1)                       # n_img, h, w (of the source), chunks per pixel: 4 x (2^19 + 1) output chunks
GATHER2 = (2049, 1025)                          # rows x 16-byte chunks per row
MSE_SHAPES = {"61x97": (61, 97), "183x97": (183, 97)}
EMA_SIZES = (1000, 1048576 + 7)
ADAMW_BIG = 2097152 * 4 + 1024 * 4
SECOND_PASS = {       # case: (work items, workgroups)
    "mse 61x97": (3 * 61 * 97 * 4, LOSS_BLOCKS), "mse 183x97": (3 * 183 * 97 * 4, LOSS_BLOCKS),
    "ema": (EMA_SIZES[1], grid_for(EMA_SIZES[1], 1024)),
    "add_noise": (N2, grid_for(N2)), "ddim": (N2, grid_for(N2)), "ddpm": (N2, grid_for(N2)), "nchw_to_nhwc": (N2, grid_for(N2)),
    "nhwc_to_nchw": (N2, grid_for(N2)), "posterior": (N2, grid_for(N2)), "eltwise": (N2, grid_for(N2)),
    "gather_rows": (GATHER2[0] * GATHER2[1], grid_for(GATHER2[0] * GATHER2[1])),
    "silu_bwd": (ELT2, grid_for(ELT2)), "gelu_bwd": (ELT2, grid_for(ELT2)), "add": (ELT2, grid_for(ELT2)),
    "geglu_fwd": (GEGLU2[0] * GEGLU2[1], grid_for(GEGLU2[0] * GEGLU2[1])), "geglu_bwd": (GEGLU2[0] * GEGLU2[1], grid_for(GEGLU2[0] * GEGLU2[1])),
    "pool2x2": (POOL2[0] * POOL2[1] * POOL2[2] * POOL2[3], grid_for(POOL2[0] * POOL2[1] * POOL2[2] * POOL2[3])),
    "zero_insert": (ZERO2[0] * 4 * ZERO2[1] * ZERO2[2] * ZERO2[3], grid_for(ZERO2[0] * 4 * ZERO2[1] * ZERO2[2] * ZERO2[3])),
}
ADAMW_SIZES = [      # n, offsets in floats of (p, g, m, v), the kernel the rule picks
    (1000, (0, 0, 0, 0), "vector"), (4099, (0, 0, 0, 0), "scalar"), (4096, (1, 0, 0, 0), "scalar"), (4096, (0, 0, 0, 0), "vector"),
    (ADAMW_BIG, (0, 0, 0, 0), "vector")]


def test_cases_reach_the_branches_they_are_named_for():
    """CPU: the source still states the rules; sumsq_kernel's walk at every size of section A; every second-pass case takes one"""
    for name, text in RULES_IN_SOURCE:
        assert _squeeze(text) in _squeeze((CSRC / name).read_text()), f"{name} no longer states: {text}"
    assert STEP == 262144 and 3 * STEP * 4 + 4 == 3145732               # the unrolled loop needs n / 4 > 3 x 1024 x 256
    for n, (entered, unrolled, rem, tail) in SUMSQ_CASES.items():
        w = walk(n)
        assert w["entered"] == entered and w["tail"] == tail, (n, w["entered"], w["tail"])
        assert {k: v for k, v in w["unrolled"].items() if v} == unrolled and {k: v for k, v in w["rem"].items() if v} == rem, (n, w["unrolled"], w["rem"])
        assert bool((w["visits"] == 1).all()), f"n = {n}: a vector is read {int(w['visits'].min())} or {int(w['visits'].max())} times"
    w = walk(6295459)
    assert w["last_unrolled"] == 4 * STEP - 1 and w["first_rem"] == 4 * STEP            # adjacent: a shifted boundary moves one of them
    assert walk(3145729)["last_unrolled"] is None and walk(8388608)["first_rem"] is None
    assert walk(3145734)["last_unrolled"] == 3 * STEP == 3145734 // 4 - 1 and walk(3145734)["first_rem"] == 1
    w = walk(INF_N)
    assert w["region"][INF_AT["unrolled"]] == 1 and w["region"][INF_AT["nan_unrolled"]] == 1 and w["region"][INF_AT["remainder"]] == 2 and w["tail"] > 0
    for name, (items, blocks) in SECOND_PASS.items():
        assert items > blocks * 256 and items % 256, (name, items, blocks)
    assert SECOND_PASS["mse 61x97"][0] == 71004 and SECOND_PASS["mse 183x97"][0] == 213012      # 1.08 and 3.25 passes of 65 536 threads
    assert all(SECOND_PASS[k][1] == GRID_CAP for k in SECOND_PASS if not k.startswith(("mse", "ema")))
    # the smallest of each form: one chunk / element fewer fits the grid's first pass, or is a multiple of 256 on the way down
    assert ELT2 - 1 == GRID_CAP * 256 and GEGLU2[0] * GEGLU2[1] == ELT2 and POOL2[0] * POOL2[1] * POOL2[2] * POOL2[3] == ELT2
    assert ZERO2[0] * ZERO2[1] * ZERO2[2] * ZERO2[3] == 2 ** 19 + 1                            # zero_insert's count is 4 x this
    # AdamW: which kernel, how many workgroups and passes
    for n, off, kernel in ADAMW_SIZES:
        assert adamw_is_vector(n, off) == (kernel == "vector"), (n, off)
    assert not adamw_is_vector(4096, (1, 0, 0, 0)) and 4096 % 4 == 0                            # through the ALIGNMENT rule, not n % 4
    blocks = grid_for(ADAMW_BIG // 4, 2048)
    assert blocks == 1025 < GRID_CAP and ADAMW_BIG // 4 > blocks * 256 and -(-(ADAMW_BIG // 4) // (blocks * 256)) == 8
    assert grid_for(4099, 1024) == 5 and grid_for(EMA_SIZES[1], 1024) == 1025


def test_the_planted_positions_are_nonzero_and_the_counts_exact():
    """CPU: the integer gradients of the exact check (seed INT_SEED + n % 1000): nonzero at the last vector of the unrolled region, the first
    of the remainder and every tail element; the count stays below 2^24, where fp32 holds every integer"""
    for n in SUMSQ_CASES:
        k = int_grad(n)
        assert len(k["planted"]) == {3145729: 4 + 1, 3145734: 8 + 2, 6295459: 8 + 3, 8388608: 4}[n]
        assert bool((k["g"][k["planted"]] != 0).all()) and 0 < k["count"] < 2 ** 24
        assert float(k["g"].abs().max()) == 2 and bool((k["g"] == k["g"].round()).all())
        assert float(t32(float(k["count"]))) == k["count"]


# ------------------------------------------------------------------------------------------------ A. gradient norm and clip coefficient
def clip_expr(total, max_norm):
    """the fp32 expression min(1, max_norm / (total + 1e-6)); max_norm <= 0: no clipping"""
    if max_norm <= 0:
        return t32(1.0)
    return torch.minimum(t32(1.0), t32(max_norm) / (total.float().cpu() + t32(1e-6)))


def norm_slot(fill=-7.0):
    return flat_guarded(4, F32, fill, lead=8)


def new_record(scale=1.0, tracker=0, adam_step=0, found_inf=0, skipped=0, device="cuda"):
    """an mvldm_amp_state inside a guard of 7s"""
    buf = torch.full((24,), 7, dtype=torch.int32)
    buf[8:16] = 0
    buf[8:9].view(F32).fill_(scale)
    buf[9:13] = torch.tensor([tracker, adam_step, found_inf, skipped], dtype=torch.int32)
    buf = buf.to(device)
    return buf, buf[8:16]


def record_owned():
    m = torch.zeros(24, dtype=torch.bool)
    m[8:16] = True
    return m


def check_norm(norm_buf, norm, sumsq_ref, max_norm, kind, what):
    """guard; norm_out[0] and norm_out[2] within one unit in the last place of the fp64 values; the coefficient bit-equal to the fp32 expression"""
    check_guard(norm_buf, flat_owned(norm_buf, 4, lead=8), -7.0, what)
    assert float(norm[3]) == -7.0, f"{what}: norm_out[3] written"
    within_ulp(norm[0:1], sumsq_ref.sqrt().reshape(1), 1, f"{kind}/norm", what)
    within_ulp(norm[2:3], sumsq_ref.reshape(1), 1, f"{kind}/sumsq", what)
    bit_equal(norm[1].cpu(), clip_expr(norm[0], max_norm), f"{what}: clip coefficient")


@gpu
@pytest.mark.parametrize("n", list(SUMSQ_CASES))
def test_grad_norm_counts_every_element_once(ops, n):
    """integer gradients: norm_out[2] EQUALS the number the CPU counted -- one dropped, duplicated or swapped vector changes it"""
    k = int_grad(n)
    gg = k["g"].cuda()
    assert gg.data_ptr() % 16 == 0
    buf, norm = norm_slot()
    ops.grad_norm(gg, 0.1, norm_out=norm)
    exact_sum(norm[2], k["g"], f"n = {n}")
    check_norm(buf, norm, torch.tensor(float(k["count"]), dtype=torch.float64), 0.1, "grad_norm_int", f"n = {n}")
    assert float(norm[1]) < 1.0


@gpu
@pytest.mark.parametrize("n", list(SUMSQ_CASES))
def test_grad_norm_on_realistic_gradients_and_under_a_loss_scale(ops, n):
    """randn x 1e-2: norm and sum of squares within one unit in the last place of fp64's; handed over as S x g with a record (S = 2^10, 2^-3)
    the three outputs are those of the unscaled run bit for bit, found_inf stays clear and nothing else of the record moves"""
    k = real_grad(n)
    gg = k["g"].cuda()
    buf, norm = norm_slot()
    ops.grad_norm(gg, 0.1, norm_out=norm)
    check_norm(buf, norm, k["sumsq"], 0.1, "grad_norm", f"n = {n}")
    assert 0.0 < float(norm[1]) < 1.0                                   # total above max_norm
    plain = norm.cpu().clone()
    for S in (2.0 ** 10, 2.0 ** -3):
        rbuf, rec = new_record(S, tracker=5, adam_step=11, found_inf=1, skipped=2)
        buf, norm = norm_slot()
        ops.grad_norm((k["g"] * S).cuda(), 0.1, norm_out=norm, amp_state=rec)
        bit_equal(norm.cpu(), plain, f"n = {n}, S = {S}")
        check_guard(buf, flat_owned(buf, 4, lead=8), -7.0, "norm_out")
        check_guard(rbuf, record_owned(), 7, "record")
        assert rec.tolist() == [int(t32(S).view(torch.int32)), 5, 11, 0, 2, 0, 0, 0]            # found_inf cleared by a finite run


@gpu
def test_clip_coefficient_is_the_fp32_expression(ops):
    """total above and below max_norm, an all-zero gradient, max_norm 0 and -1, sumsq_in (the total comes from it, norm_out[2] stays the
    buffer's own), clip_from_sumsq (n = 0)"""
    n = 1000
    k = real_grad(n)
    gg, zero = k["g"].cuda(), torch.zeros(n, device="cuda")
    total = float(k["sumsq"].sqrt())
    for max_norm in (0.5 * total, 2.0 * total, 1e3, 0.0, -1.0):
        buf, norm = norm_slot()
        ops.grad_norm(gg, max_norm, norm_out=norm)
        check_norm(buf, norm, k["sumsq"], max_norm, "clip", f"max_norm {max_norm}")
        assert (float(norm[1]) < 1.0) == (0 < max_norm < total)
    for max_norm in (0.1, 0.0):
        buf, norm = norm_slot()
        ops.grad_norm(zero, max_norm, norm_out=norm)
        assert norm.tolist() == [0.0, 1.0, 0.0, -7.0]
    for sumsq in (123.456, 1e-8, 0.0):
        s_in = t32([sumsq]).cuda()
        buf, norm = norm_slot()
        ops.grad_norm(gg, 0.1, norm_out=norm, sumsq_in=s_in)
        check_guard(buf, flat_owned(buf, 4, lead=8), -7.0, "sumsq_in")
        want_total = t32([sumsq]).double().sqrt().float()                # (float)sqrt((double)sumsq_in[0])
        bit_equal(norm[0:1].cpu(), want_total, f"sumsq_in {sumsq}: total")
        bit_equal(norm[1].cpu(), clip_expr(norm[0], 0.1), f"sumsq_in {sumsq}: coefficient")
        within_ulp(norm[2:3], k["sumsq"].reshape(1), 1, "clip/own_sumsq", f"sumsq_in {sumsq}")
        buf2, norm2 = norm_slot()
        ops.clip_from_sumsq(s_in, 0.1, norm2)
        check_guard(buf2, flat_owned(buf2, 4, lead=8), -7.0, "clip_from_sumsq")
        bit_equal(norm2[0:2].cpu(), norm[0:2].cpu(), f"clip_from_sumsq {sumsq}")
        assert float(norm2[2]) == 0.0 and float(norm2[3]) == -7.0        # an empty buffer's own sum


@gpu
def test_found_inf_from_every_loop_of_the_sum(ops):
    """an inf in the unrolled region, in a remainder pass, in the scalar tail; a NaN; a non-finite sumsq_in over a finite buffer: each sets
    found_inf, and a finite run clears it again"""
    n = INF_N
    gg = (real_grad(n)["g"] * 2.0 ** 10).cuda()
    rbuf, rec = new_record(2.0 ** 10)
    where = {"unrolled": (4 * INF_AT["unrolled"] + 1, float("inf")), "remainder": (4 * INF_AT["remainder"] + 2, float("-inf")),
             "tail": (n - 1, float("inf")), "nan": (4 * INF_AT["nan_unrolled"] + 3, float("nan"))}
    for name, (at, value) in where.items():
        keep = float(gg[at])
        gg[at] = value
        buf, norm = norm_slot()
        ops.grad_norm(gg, 0.1, norm_out=norm, amp_state=rec)
        assert int(rec[3]) == 1 and not math.isfinite(float(norm[0])) and not math.isfinite(float(norm[2])), (name, norm.tolist())
        gg[at] = keep
        ops.grad_norm(gg, 0.1, norm_out=norm, amp_state=rec)
        assert int(rec[3]) == 0 and math.isfinite(float(norm[0])), name
        check_guard(buf, flat_owned(buf, 4, lead=8), -7.0, name)
    finite = norm.cpu().clone()
    for bad in (float("inf"), float("nan")):
        buf, norm = norm_slot()
        ops.grad_norm(gg, 0.1, norm_out=norm, sumsq_in=t32([bad]).cuda(), amp_state=rec)
        assert int(rec[3]) == 1 and not math.isfinite(float(norm[0]))
        bit_equal(norm[2:3].cpu(), finite[2:3], "own sum under a non-finite sumsq_in")
        ops.grad_norm(gg, 0.1, norm_out=norm, amp_state=rec)
        assert int(rec[3]) == 0
    check_guard(rbuf, record_owned(), 7, "record")
    assert rec.tolist()[1:] == [0] * 7


@gpu
def test_grad_norm_refuses_a_misaligned_gradient(ops):
    """sumsq_kernel reads g in 16-byte vectors: a pointer that is not 16-byte aligned is MVLDM_ERR_ARG when n >= 4 and NOTHING is launched
    (norm_out and the record keep their fill).  Only the refusal is tested."""
    from mv_ldm_amd import _lib as L
    lib = L.load()
    base = torch.zeros(64, device="cuda")
    ws = ops.workspace(1024 * 8, base.device, "norm")
    for off in (1, 2, 3):
        g = base[off:off + 8]
        assert g.data_ptr() % 16 == 4 * off
        buf, norm = norm_slot()
        rbuf, rec = new_record(4.0, found_inf=1)
        assert lib.mvldm_grad_norm(g.data_ptr(), 8, None, 0.1, norm.data_ptr(), ws.data_ptr(), ops.stream()) == ERR_ARG
        assert b"16-byte aligned" in lib.mvldm_last_error()
        assert lib.mvldm_grad_norm_amp(g.data_ptr(), 4, None, 0.1, norm.data_ptr(), rec.data_ptr(), ws.data_ptr(), ops.stream()) == ERR_ARG
        torch.cuda.synchronize()
        assert bool((buf == -7.0).all()) and bool((rbuf.cpu() == new_record(4.0, found_inf=1, device="cpu")[0]).all())


# ------------------------------------------------------------------------------------------------ B. AdamW, EMA, loss scaler
ADAMW_DEFAULT = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, wd=1e-2, step=3, grad_scale=1.0, clip=0.37, fresh=False, zeros=False, record=None)
ADAMW_PARAMS = {
    "defaults": {},
    "step1": dict(step=1, fresh=True),
    "step100000": dict(step=100000),                                    # both bias corrections round to 1
    "wd0": dict(wd=0.0),
    "wd0.1": dict(wd=0.1),
    "eps1e-6": dict(eps=1e-6),
    "betas0.8_0.9": dict(betas=(0.8, 0.9)),
    "grad_scale0.25_clipped": dict(grad_scale=0.25, clip=0.61),
    "no_clip": dict(clip=None),
    "zero_gradients": dict(zeros=True),
    "record_step0": dict(record=dict(adam_step=0, found_inf=0), fresh=True),
    "record_step99999": dict(record=dict(adam_step=99999, found_inf=0)),
    "record_found_inf": dict(record=dict(adam_step=7, found_inf=1)),
}
AMP_S = 2.0 ** 10
LEAD = 64                   # floats of guard in front of an optimizer buffer (256 bytes: the slice behind it is 16-byte aligned)


@functools.lru_cache(maxsize=None)
def adamw_inputs(n, fresh, zeros):
    """p0, g, m0, v0: m0 carries the sign of g (no cancellation in b1 m + (1 - b1) g), v0 >= 1e-6 (or both zero: the first step);
    `zeros`: the first 64 gradients are exactly zero with zero moments"""
    g = G(4000 + n % 991)
    p0, gr = torch.randn(n, generator=g) * 0.05, torch.randn(n, generator=g) * 1e-2
    m0 = torch.randn(n, generator=g).abs() * 1e-3 * torch.sign(gr)
    v0 = torch.rand(n, generator=g) * 1e-4 + 1e-6
    if fresh:
        m0, v0 = torch.zeros(n), torch.zeros(n)
    if zeros:
        gr[:64], m0[:64], v0[:64] = 0.0, 0.0, 0.0
    return p0, gr, m0, v0


def run_adamw(ops, n, offsets, name):
    """one AdamW case three ways from the same inputs: the kernel on slices of guarded buffers, TorchOptimizerOps.update, fp64.  m and v within
    2 units in the last place of fp64's; the update's relative L2 error at most twice the stand-in's; under found_inf nothing moves"""
    c = dict(ADAMW_DEFAULT, **ADAMW_PARAMS[name])
    lr, (b1, b2), eps, wd = f32r(c["lr"]), tuple(f32r(b) for b in c["betas"]), f32r(c["eps"]), f32r(c["wd"])
    rec_c = c["record"]
    p0, gr, m0, v0 = adamw_inputs(n, c["fresh"], c["zeros"])
    S = AMP_S if rec_c else 1.0
    handed = gr * S                                                       # exact: S is a power of two
    step = rec_c["adam_step"] + 1 if rec_c else c["step"]
    # ---- the kernel, on slices of guarded buffers
    bufs, views = {}, {}
    for key, src, off in zip("pgmv", (p0, handed, m0, v0), offsets):
        bufs[key] = torch.full((LEAD + 4 + n + GUARD,), 7.0, device="cuda")
        assert bufs[key].data_ptr() % 16 == 0
        views[key] = bufs[key][LEAD + off:LEAD + off + n]
        views[key].copy_(src)
    assert all(views[k].data_ptr() % 16 == 4 * off % 16 for k, off in zip("pgmv", offsets))
    clip = None if c["clip"] is None else t32([9.0, c["clip"], 0.0, 0.0]).cuda()
    rbuf, rec = new_record(S, tracker=4, adam_step=rec_c["adam_step"], found_inf=rec_c["found_inf"], skipped=1) if rec_c else (None, None)
    rec_before = None if rec is None else rec.cpu().clone()
    ops.adamw_step(views["p"], views["g"], views["m"], views["v"], lr, (b1, b2), eps, wd, step=-1 if rec_c else step,
                   grad_scale=c["grad_scale"], clip=clip, amp_state=rec)
    for key, off in zip("pgmv", offsets):
        check_guard(bufs[key], flat_owned(bufs[key], n, lead=LEAD + off), 7.0, f"{name} {key}")
    bit_equal(views["g"].cpu(), handed, "the gradient is read only")
    if rec is not None:
        check_guard(rbuf, record_owned(), 7, "record")
        bit_equal(rec.cpu(), rec_before, "the record is read only")
    got = {k: views[k].cpu() for k in "pmv"}
    # ---- the stand-in, from the same inputs: its norm[1] is the kernel's grad_scale * clip[1], formed in fp32
    gs = t32(c["grad_scale"]) * (t32(1.0) if c["clip"] is None else t32(c["clip"]))
    sp, sm, sv = p0.clone(), m0.clone(), v0.clone()
    TorchOptimizerOps.update(sp, handed.clone(), sm, sv, lr, (b1, b2), eps, wd, step, torch.stack([t32(9.0), gs]), None if rec is None else rec_before.clone())
    if rec_c and rec_c["found_inf"]:
        for k, t0, st in (("p", p0, sp), ("m", m0, sm), ("v", v0, sv)):
            bit_equal(got[k], t0, f"{name}: {k} after a found_inf step")
            bit_equal(st, t0, f"{name}: the stand-in's {k} after a found_inf step")
        return
    # ---- fp64, from the fp32 gi = g * gs that the kernel forms first (gs: x 1/S in fp32 under a record)
    if rec_c:
        gs = gs * (1.0 / t32(S).double()).float()
    gi = (handed * gs).double()
    m_ref = b1 * m0.double() + (1.0 - b1) * gi
    v_ref = b2 * v0.double() + (1.0 - b2) * gi * gi
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    upd_ref = -(lr * wd) * p0.double() - (lr / bc1) * m_ref / (v_ref.sqrt() / math.sqrt(bc2) + eps)
    if step == 100000:
        assert bc1 == 1.0 and bc2 == 1.0
    kind = f"adamw/{'vector' if adamw_is_vector(n, offsets) else 'scalar'}"
    within_ulp(got["m"], m_ref, 2, f"{kind}/m", f"{name} n = {n}")
    within_ulp(got["v"], v_ref, 2, f"{kind}/v", f"{name} n = {n}")
    e_kernel = record_err(f"{kind}/update_rel_l2", rel_l2(got["p"].double() - p0.double(), upd_ref))
    e_standin = record_err(f"{kind}/update_rel_l2_standin", rel_l2(sp.double() - p0.double(), upd_ref))
    record_err(f"{kind}/update_kernel_over_standin", e_kernel / e_standin)
    print(f"adamw {name} n = {n}: update rel-L2 kernel {e_kernel:.3e}, stand-in {e_standin:.3e}")
    assert e_standin > 0 and e_kernel <= 2.0 * e_standin, f"{name} n = {n}: update rel-L2 {e_kernel:.3e}, the stand-in's {e_standin:.3e}"
    if c["zeros"]:       # zero gradient, zero moments: the update is the weight decay alone, p * (1 - lr * wd) with the factor formed in fp32
        bit_equal(got["p"][:64], p0[:64] * (t32(1.0) - t32(lr) * t32(wd)), "zero gradients")
        assert float(got["m"][:64].abs().max()) == 0 and float(got["v"][:64].abs().max()) == 0


@gpu
@pytest.mark.parametrize("n,offsets,kernel", ADAMW_SIZES, ids=[f"{n}{'+1' if o[0] else ''}-{k}" for n, o, k in ADAMW_SIZES])
def test_adamw_sizes_against_fp64_and_the_stand_in(ops, n, offsets, kernel):
    """both kernels (the scalar one through n % 4 and through a parameter pointer one float off the 16-byte grid), one workgroup to 1025 of
    7 to 8 passes; MVLDM_ADAMW_NT at its default"""
    run_adamw(ops, n, offsets, "defaults")
    run_adamw(ops, n, offsets, "record_step0")


@gpu
@pytest.mark.parametrize("n", [4096, 4099], ids=["vector", "scalar"])
@pytest.mark.parametrize("name", [k for k in ADAMW_PARAMS if k != "defaults"])
def test_adamw_parameters_against_fp64_and_the_stand_in(ops, name, n):
    run_adamw(ops, n, (0, 0, 0, 0), name)


@functools.lru_cache(maxsize=None)
def ema_inputs(n):
    g = G(5000 + n % 983)
    p = torch.randn(n, generator=g)
    avg = p * (1.0 + (0.1 * torch.randn(n, generator=g)).clamp(-0.4, 0.4))          # within a factor of two: p - avg is exact
    assert bool(((p - avg).double() == p.double() - avg.double()).all())
    return avg, p


@gpu
@pytest.mark.parametrize("w", [0.005, 0.499, 0.5, 0.75, 0.0, 1.0])
@pytest.mark.parametrize("n", EMA_SIZES)
def test_ema_both_branches_against_lerp_and_fp64(ops, n, w):
    """w < 0.5 and w >= 0.5 (torch's two forms), one workgroup and 1025 of four passes; w = 0 leaves avg, w = 1 gives p, bit for bit"""
    avg0, p = ema_inputs(n)
    w32 = f32r(w)
    buf, avg = flat_guarded(n, F32)
    avg.copy_(avg0)
    pg = p.cuda()
    ops.ema_update(avg, pg, w32)
    check_guard(buf, flat_owned(buf, n), 7.0, f"ema n = {n}")
    bit_equal(pg.cpu(), p, "p is read only")
    got = avg.cpu()
    if w in (0.0, 1.0):
        bit_equal(got, avg0 if w == 0.0 else p, f"w = {w}")
        return
    within_ulp(got, avg0.clone().lerp_(p, w32), 1, f"ema/lerp/{'lo' if w < 0.5 else 'hi'}", f"n = {n} w = {w}")
    within_ulp(got, avg0.double() + w32 * (p.double() - avg0.double()), 1, f"ema/fp64/{'lo' if w < 0.5 else 'hi'}", f"n = {n} w = {w}")


SCALER_SEQUENCES = {      # name: (S, tracker, growth, backoff, interval, [found_inf of each call])
    "interval3_grows": (2.0 ** 10, 0, 2.0, 0.5, 3, [0, 0, 0, 0]),
    "skip_in_the_middle": (2.0 ** 10, 0, 2.0, 0.5, 3, [0, 1, 0, 0, 0, 1, 1]),
    "growth_refused_at_3e38": (3e38, 2, 2.0, 0.5, 3, [0, 0]),
    "denormal_backoff": (2.0 ** -126, 1, 2.0, 0.5, 3, [1, 1, 0]),
    "interval1": (2.0 ** 4, 0, 2.0, 0.5, 1, [0, 0, 1, 0]),
    "tracker_above_interval": (2.0 ** 10, 5, 2.0, 0.5, 3, [0, 0, 0, 0]),
}
SCALER_EXPECT = {         # the record after the LAST call: S, tracker, adam_step, found_inf, skipped
    "interval3_grows": (2.0 ** 11, 1, 4, 0, 0),
    "skip_in_the_middle": (2.0 ** 8, 0, 4, 0, 3),
    "growth_refused_at_3e38": (f32r(3e38), 1, 2, 0, 0),
    "denormal_backoff": (2.0 ** -128, 1, 1, 0, 2),
    "interval1": (2.0 ** 6, 0, 3, 0, 1),
    "tracker_above_interval": (2.0 ** 12, 0, 4, 0, 0),
}


def stand_in_sequence(name):
    """the record after every call of the sequence, by TorchOptimizerOps.update_scale"""
    S, tracker, growth, backoff, interval, founds = SCALER_SEQUENCES[name]
    _, rec = new_record(S, tracker=tracker, device="cpu")
    out = []
    for found in founds:
        rec[3] = found
        TorchOptimizerOps.update_scale(rec, growth, backoff, interval)
        out.append(rec.clone())
    return out


@pytest.mark.parametrize("name", list(SCALER_SEQUENCES))
def test_loss_scaler_stand_in_sequences(name):
    """CPU: what the stand-in makes of each sequence -- growth at the interval, a skip that resets the tracker and does not advance AdamW,
    a growth that would not be finite refused, a denormal S kept, and a tracker ABOVE the interval (a record resumed under a shorter
    one) growing at once, which is the kernel's >= and not torch's == (the stand-in clamps the tracker first)"""
    last = stand_in_sequence(name)[-1]
    assert (float(last[0:1].view(F32)), *last[1:5].tolist()) == SCALER_EXPECT[name] and last[5:].tolist() == [0, 0, 0]
    if name == "tracker_above_interval":
        first = stand_in_sequence(name)[0]
        assert (float(first[0:1].view(F32)), int(first[1])) == (2.0 ** 11, 0)
        s, t = t32([2.0 ** 10]), torch.tensor([5], dtype=torch.int32)
        torch._amp_update_scale_(s, t, t32([0.0]), 2.0, 0.5, 3)
        assert (float(s), int(t)) == (2.0 ** 10, 6)                     # torch alone: never grows again


@gpu
@pytest.mark.parametrize("name", list(SCALER_SEQUENCES))
def test_loss_scaler_kernel_and_stand_in_step_together(ops, name):
    """amp_update_kernel and TorchOptimizerOps.update_scale from the same record: the whole record equal after every call"""
    S, tracker, growth, backoff, interval, founds = SCALER_SEQUENCES[name]
    rbuf, rec = new_record(S, tracker=tracker)
    for call, (found, want) in enumerate(zip(founds, stand_in_sequence(name))):
        rec[3] = found
        ops.amp_update(rec, growth, backoff, interval)
        assert rec.tolist() == want.tolist(), (name, call, rec.tolist(), want.tolist(), float(rec[0:1].view(F32)), float(want[0:1].view(F32)))
        check_guard(rbuf, record_owned(), 7, f"{name} call {call}")


# ------------------------------------------------------------------------------------------------ C. loss and noise
MSE_IMG, MSE_TGT, MSE_C, MSE_DC = 5, [4, 0, 2], 4, 8


@functools.lru_cache(maxsize=None)
def mse_inputs(shape, outliers):
    h, w = MSE_SHAPES[shape]
    hw, g = h * w, G(6000 + h)
    pred, noise = torch.randn(MSE_IMG, hw, MSE_C, generator=g), torch.randn(len(MSE_TGT), MSE_C, hw, generator=g)
    if outliers:          # differences of 3e5 to 2e6: 2^16 x the f16 gradient of these overflows
        at = torch.randint(0, hw, (12,), generator=g)
        for k, pix in enumerate(at.tolist()):
            pred[MSE_TGT[k % 3], pix, k % MSE_C] = (-1) ** k * 3e5 * (1 + k % 7)
    d = pred[MSE_TGT] - noise.permute(0, 2, 1)                            # the fp32 difference, [t][pix][ch]
    pd = pred.double().requires_grad_()
    with torch.enable_grad():
        loss = F.mse_loss(pd[MSE_TGT].permute(0, 2, 1), noise.double())
        (gp,) = torch.autograd.grad(loss, pd)
    return dict(pred=pred, noise=noise, d=d, sum64=(d.double() ** 2).sum(), N=float(len(MSE_TGT) * hw * MSE_C), loss64=loss.detach(), grad64=gp, hw=hw)


def run_mse(ops, shape, dtype, amp_scale=None, outliers=False):
    """accumulate 0 then 1, loss_scale 1/3, grad_scale 1/6; dpred [5][hw][8] between two guard images, the whole buffer prefilled with 7.0:
    the kernel writes the 4 channels of the 3 target images and NOTHING else -- that the non-target images and the padding channels of
    dpred are zero in the product is the caller's contract (it zero-fills them), not the kernel's"""
    from mv_ldm_amd import _lib as L
    lib, k = L.load(), mse_inputs(shape, outliers)
    hw, N = k["hw"], k["N"]
    loss_scale, grad_scale = f32r(1 / 3), f32r(1 / 6)
    pred, noise, tgt = k["pred"].cuda(), k["noise"].cuda(), torch.tensor(MSE_TGT, dtype=torch.int32, device="cuda")
    dbuf = torch.full((1 + MSE_IMG + 1, hw, MSE_DC), 7.0, dtype=dtype, device="cuda")
    dpred = dbuf[1:1 + MSE_IMG]
    lbuf, loss = flat_guarded(1, F32, -7.0, lead=8)
    wbuf, ws = flat_guarded(LOSS_BLOCKS, torch.float64, -7.0, lead=8)
    s_dev = None if amp_scale is None else t32([amp_scale]).cuda()
    for acc in (0, 1):
        args = (pred.data_ptr(), noise.data_ptr(), tgt.data_ptr(), len(MSE_TGT), hw, MSE_C, loss.data_ptr(), acc, loss_scale, dpred.data_ptr(), MSE_DC,
                ops.dt(dtype), grad_scale)
        if amp_scale is None:
            L.check(lib.mvldm_mse_loss(*args, ws.data_ptr(), ops.stream()))
        else:
            L.check(lib.mvldm_mse_loss_amp(*args, s_dev.data_ptr(), ws.data_ptr(), ops.stream()))
        if acc == 0:
            first = loss.cpu().clone()
    kind, what = f"mse/{NAME[dtype]}", f"{shape} {NAME[dtype]} S = {amp_scale}"
    check_guard(lbuf, flat_owned(lbuf, 1, lead=8), -7.0, what + " loss")
    check_guard(wbuf, flat_owned(wbuf, LOSS_BLOCKS, lead=8), -7.0, what + " workspace")
    own = torch.zeros(dbuf.shape, dtype=torch.bool)
    own[[1 + t for t in MSE_TGT], :, :MSE_C] = True
    check_guard(dbuf, own, 7.0, what + " dpred")
    # reference 1, the restatement: fp32 difference, fp64 sum, (float)(loss_scale / N * sum); dpred = float(2 grad_scale / N) [* S] * d, rounded once
    within_ulp(first, (loss_scale / N * k["sum64"]).reshape(1), 1, f"{kind}/loss", what)
    bit_equal(loss.cpu(), first + first, what + ": the accumulated loss")
    gscale = t32(f32r(2.0 * grad_scale / N))
    if amp_scale is not None:
        gscale = gscale * t32(amp_scale)
    want = (gscale * k["d"]).to(dtype)
    bit_equal(dpred[MSE_TGT][..., :MSE_C].cpu(), want, what + ": dpred")
    if dtype == F16 and amp_scale == 2.0 ** 16:
        assert outliers and 0 < int(torch.isinf(want).sum()) <= 12, int(torch.isinf(want).sum())
    # reference 2: F.mse_loss in fp64 and its autograd gradient, the bounds of test_add_noise_and_mse_loss
    if dtype == F32 and not outliers:
        e_loss = record_err(f"{kind}/loss_rel", abs(float(first) - loss_scale * float(k["loss64"])) / float(k["loss64"]))
        e_grad = record_err(f"{kind}/grad_rel_l2", rel_l2(dpred[..., :MSE_C].cpu()[MSE_TGT] / (amp_scale or 1.0), grad_scale * k["grad64"][MSE_TGT]))
        assert e_loss < 1e-6 and e_grad < 1e-6, (what, e_loss, e_grad)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", list(MSE_SHAPES))
def test_mse_loss_second_pass_and_what_it_writes(ops, shape, dtype):
    run_mse(ops, shape, dtype)
    run_mse(ops, shape, dtype, amp_scale=2.0 ** 12)


@gpu
def test_mse_loss_f16_gradient_overflows_where_the_restatement_does(ops):
    """S = 2^16 and differences of 3e5 and more: the f16 dpred is inf exactly where float16(float32 product) is"""
    run_mse(ops, "61x97", F16, amp_scale=2.0 ** 16, outliers=True)
    run_mse(ops, "61x97", F32, amp_scale=2.0 ** 16, outliers=True)


@gpu
def test_mse_loss_refusals_write_nothing(ops):
    """dpred narrower than the loss's channels, no target image, a null workspace: MVLDM_ERR_ARG, loss and dpred keep their fill"""
    from mv_ldm_amd import _lib as L
    lib, k = L.load(), mse_inputs("61x97", False)
    pred, noise, tgt = k["pred"].cuda(), k["noise"].cuda(), torch.tensor(MSE_TGT, dtype=torch.int32, device="cuda")
    dpred, loss, ws = torch.full((MSE_IMG, k["hw"], MSE_DC), 7.0, device="cuda"), torch.full((1,), -7.0, device="cuda"), torch.full((256,), -7.0, dtype=torch.float64, device="cuda")
    head = (pred.data_ptr(), noise.data_ptr(), tgt.data_ptr())
    assert lib.mvldm_mse_loss(*head, 3, k["hw"], MSE_C, loss.data_ptr(), 0, 1.0, dpred.data_ptr(), 3, L.F32, 1.0, ws.data_ptr(), ops.stream()) == ERR_ARG
    assert lib.mvldm_mse_loss(*head, 0, k["hw"], MSE_C, loss.data_ptr(), 0, 1.0, dpred.data_ptr(), MSE_DC, L.F32, 1.0, ws.data_ptr(), ops.stream()) == ERR_ARG
    assert lib.mvldm_mse_loss(*head, 3, k["hw"], MSE_C, loss.data_ptr(), 0, 1.0, dpred.data_ptr(), MSE_DC, L.F32, 1.0, None, ops.stream()) == ERR_ARG
    assert lib.mvldm_mse_loss_amp(*head, 3, k["hw"], MSE_C, loss.data_ptr(), 0, 1.0, dpred.data_ptr(), 3, L.F16, 1.0, loss.data_ptr(), ws.data_ptr(), ops.stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((dpred == 7.0).all()) and float(loss) == -7.0 and bool((ws == -7.0).all())


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_add_noise_second_pass(ops, dtype):
    """2 099 500 elements into channels [3, 7) of 16, five sources permuted into seven destination images: the torch fp32 expression
    sqrt(a) x0 + sqrt(1 - a) noise (separately rounded), rounded once to the destination's type; everything else keeps the fill"""
    from mv_ldm_amd import _lib as L
    n, c, h, w = 5, 4, 323, 325
    g = G(6100)
    x0, noise, coef = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g), torch.rand(n, 2, generator=g)
    img_map = [6, 2, 0, 5, 3]
    want = (coef[:, 0].view(n, 1, 1, 1) * x0 + coef[:, 1].view(n, 1, 1, 1) * noise).permute(0, 2, 3, 1).to(dtype)
    buf, flat = flat_guarded(7 * HW2 * 16, dtype)
    dst = flat.view(7, h, w, 16)
    x0g, noiseg, coefg, mapg = x0.cuda(), noise.cuda(), coef.cuda(), torch.tensor(img_map, dtype=torch.int32, device="cuda")
    L.check(L.load().mvldm_add_noise(x0g.data_ptr(), noiseg.data_ptr(), coefg.data_ptr(), dst.data_ptr(), n, c, HW2, 16, 3, ops.dt(dtype),
                                     mapg.data_ptr(), ops.stream()))
    own = torch.zeros(7, h, w, 16, dtype=torch.bool)
    own[img_map, :, :, 3:7] = True
    check_guard(buf, torch.cat([torch.zeros(GUARD, dtype=torch.bool), own.flatten(), torch.zeros(GUARD, dtype=torch.bool)]), 7.0, "add_noise")
    bit_equal(dst[img_map][..., 3:7].cpu(), want, "add_noise")


# ------------------------------------------------------------------------------------------------ D. sampler-step kernels
def ddim_coef(s):
    """the coefficient table of a set-up oracle DDIMScheduler, as test_ddim_cfg_step_bit_exact forms it"""
    ac, ratio, rows = s.alphas_cumprod, s.config.num_train_timesteps // s.num_inference_steps, []
    for t in s.timesteps.tolist():
        a_t, a_p = ac[t], ac[t - ratio] if t - ratio >= 0 else s.final_alpha_cumprod
        rows.append(torch.stack([(1 - a_t) ** 0.5, a_t ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5]))
    return torch.stack(rows).float().contiguous()


@gpu
def test_ddim_step_second_pass_with_guidance_clipping_and_a_16_bit_input_row(ops):
    """2 099 500 elements, uncond_img, clip_range 1, unet_in bf16 with 16 channels inside a guard: x_next bit-equal to the oracle scheduler's
    fp32 expression; the cond AND uncond images of unet_in hold its bf16 rounding in channels [0, 4), everything else keeps the fill"""
    from oracle.scheduler import DDIMScheduler
    s = DDIMScheduler(clip_sample=True)
    s.set_timesteps(50)
    coef = ddim_coef(s).cuda()
    n_tgt, n_img, h, w, c = 5, 12, 323, 325, 4
    g = G(7000)
    eps, x = torch.randn(n_img, h, w, c, generator=g), torch.randn(n_tgt, h, w, c, generator=g) * 1.5
    cond, unc = [1, 3, 5, 7, 10], [0, 2, 4, 6, 8]
    step = 31
    pred = eps[unc] + 3.0 * (eps[cond] - eps[unc])
    out = s.step(pred, s.timesteps[step], x)
    assert 0.01 < float((out.pred_original_sample.abs() == 1.0).float().mean()) < 0.99             # the clamp is at work, not everywhere
    buf, flat = flat_guarded(n_img * h * w * 16, BF16)
    unet_in = flat.view(n_img, h, w, 16)
    got = ops.ddim_cfg_step(eps.cuda(), x.cuda(), torch.tensor(cond, dtype=torch.int32).cuda(), torch.tensor(unc, dtype=torch.int32).cuda(), 3.0, coef,
                            torch.tensor([step], dtype=torch.int32).cuda(), unet_in, clip_range=1.0)
    bit_equal(got.cpu(), out.prev_sample, "x_next")
    own = torch.zeros(n_img, h, w, 16, dtype=torch.bool)
    own[cond + unc, :, :, :c] = True
    check_guard(buf, torch.cat([torch.zeros(GUARD, dtype=torch.bool), own.flatten(), torch.zeros(GUARD, dtype=torch.bool)]), 7.0, "unet_in")
    bit_equal(unet_in[cond][..., :c].cpu(), out.prev_sample.to(BF16), "unet_in, cond images")
    bit_equal(unet_in[unc][..., :c].cpu(), out.prev_sample.to(BF16), "unet_in, uncond images")


@gpu
def test_ddim_step_counter_below_zero_and_a_one_step_table(ops):
    """*step_ptr = -3 acts as step 0; n_steps = 1: every counter value is that one row"""
    from oracle.scheduler import DDIMScheduler
    s = DDIMScheduler(clip_sample=False)
    s.set_timesteps(5)
    coef = ddim_coef(s)
    g = G(7001)
    eps, x = torch.randn(3, 5, 7, 4, generator=g), torch.randn(2, 5, 7, 4, generator=g)
    cond = torch.tensor([2, 0], dtype=torch.int32).cuda()
    run = lambda table, ptr: ops.ddim_cfg_step(eps.cuda(), x.cuda(), cond, None, 0.0, table.cuda(), torch.tensor([ptr], dtype=torch.int32).cuda(), None).cpu()
    want = s.step(eps[[2, 0]], s.timesteps[0], x).prev_sample
    bit_equal(run(coef, 0), want, "step 0")
    bit_equal(run(coef, -3), want, "step -3")
    one = coef[3:4].contiguous()
    want = s.step(eps[[2, 0]], s.timesteps[3], x).prev_sample
    for ptr in (0, -1, 1, 7):
        bit_equal(run(one, ptr), want, f"n_steps = 1, counter {ptr}")


def ddpm_expr(ec, eu, x, z, cfg, coef, clip):
    """DDPMScheduler.step behind the CFG compose in the order of its fp32 operations (csrc/misc.hip ddpm_kernel's comment)"""
    sb, sa, c0, c1, sigma = coef
    e = ec if eu is None else eu + cfg * (ec - eu)
    x0 = (x - sb * e) / sa
    if clip > 0:
        x0 = x0.clamp(-clip, clip)
    prev = c0 * x0 + c1 * x
    return prev + (sigma * z if z is not None else 0.0)


@gpu
def test_ddpm_step_second_pass(ops):
    """2 099 500 elements with and without eps_u, clipped and not; noise = None at sigma = 0; bit-equal to the fp32 expression"""
    g = G(7100)
    ec, eu, x, z = (torch.randn(N2, generator=g) for _ in range(4))
    x = x * 1.7
    coef = t32([0.6, 0.8, 0.3, 0.69, 0.05])
    coef0 = t32([0.1, 0.995, 0.99, 0.01, 0.0])
    dev = {k: v.cuda() for k, v in dict(ec=ec, eu=eu, x=x, z=z).items()}
    for use_u, clip in ((True, 1.0), (False, 0.0)):
        got = ops.ddpm_cfg_step(dev["ec"], dev["eu"] if use_u else None, dev["x"], dev["z"], 3.0, coef.cuda(), clip)
        bit_equal(got.cpu(), ddpm_expr(ec, eu if use_u else None, x, z, t32(3.0), coef, clip), f"ddpm eps_u {use_u}")
    got = ops.ddpm_cfg_step(dev["ec"], dev["eu"], dev["x"], None, 3.0, coef0.cuda(), 1.0)
    bit_equal(got.cpu(), ddpm_expr(ec, eu, x, None, t32(3.0), coef0, 1.0), "ddpm sigma 0 without noise")


@gpu
@pytest.mark.parametrize("n_rows", [0, 1, 200])
def test_ddim_advance_rows_and_the_end_of_the_table(ops, n_rows):
    """no rows (null row pointers: the counter still advances), one row, more rows than the 64 threads; a counter at n_steps - 2, n_steps - 1
    and n_steps + 5: past the end the timestep is the table's LAST entry.  The table ends where its allocation's trailing guard begins, and
    that guard holds a sentinel timestep: a read past the end would show as a wrong value"""
    from mv_ldm_amd import _lib as L
    lib, n_steps, total_rows = L.load(), 50, 300
    table = torch.arange(980, -1, -20, dtype=torch.int64)
    assert len(table) == n_steps
    rows = torch.randperm(total_rows, generator=G(7200))[:n_rows].to(torch.int32)
    rows_dev = rows.cuda() if n_rows else None
    for counter in (0, 17, n_steps - 2, n_steps - 1, n_steps + 5):
        tbuf, tab = flat_guarded(n_steps, torch.int64, 123456789, lead=8)
        tab.copy_(table)
        tsbuf, ts = flat_guarded(total_rows, torch.int64, -5, lead=8)
        cbuf, cnt = flat_guarded(1, torch.int32, 7, lead=8)
        cnt.fill_(counter)
        L.check(lib.mvldm_ddim_advance(cnt.data_ptr(), tab.data_ptr(), n_steps, ts.data_ptr() if n_rows else None, ops.ptr(rows_dev), n_rows, ops.stream()))
        want = torch.full((total_rows,), -5, dtype=torch.int64)
        want[rows.long()] = table[min(counter + 1, n_steps - 1)]
        assert int(cnt) == counter + 1
        bit_equal(ts.cpu(), want, f"counter {counter}, {n_rows} rows")
        for b, nn, fill in ((tbuf, n_steps, 123456789), (tsbuf, total_rows, -5), (cbuf, 1, 7)):
            check_guard(b, flat_owned(b, nn, lead=8), fill, f"counter {counter}")
        bit_equal(tab.cpu(), table, "the table is read only")


@functools.lru_cache(maxsize=None)
def layout_src():
    return torch.randn(5, 4, 323, 325, generator=G(7300)) * 0.18


LAYOUT_SCALE, LAYOUT_SHIFT = f32r(1 / 0.18215), f32r(0.1)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_nchw_to_nhwc_second_pass(ops, dtype):
    """x * (1 / 0.18215) + 0.1 as torch rounds it -- the product, then the sum: the library is built with -ffp-contract=off, and an FMA
    here would differ in the last place of thousands of the 2 099 500 elements -- rounded once to the destination's type, into channels
    [2, 6) of 8 of permuted destination images inside a guard"""
    src = layout_src()
    n, c, h, w = src.shape
    img_map = [3, 0, 6, 1, 4]
    buf, flat = flat_guarded(7 * HW2 * 8, dtype)
    dst = flat.view(7, h, w, 8)
    ops.nchw_to_nhwc(src.cuda(), dtype, dst=dst, c_off=2, scale=LAYOUT_SCALE, shift=LAYOUT_SHIFT, img_map=torch.tensor(img_map, dtype=torch.int32).cuda())
    own = torch.zeros(7, h, w, 8, dtype=torch.bool)
    own[img_map, :, :, 2:6] = True
    check_guard(buf, torch.cat([torch.zeros(GUARD, dtype=torch.bool), own.flatten(), torch.zeros(GUARD, dtype=torch.bool)]), 7.0, "nchw_to_nhwc")
    prod = src * t32(LAYOUT_SCALE)
    want = prod + t32(LAYOUT_SHIFT)
    fused = (src.double() * LAYOUT_SCALE + LAYOUT_SHIFT).float()                                # what one rounding (an FMA) would give
    assert int((fused != want).sum()) > 1000                                                    # so this case tells the two apart
    bit_equal(dst[img_map][..., 2:6].cpu(), want.permute(0, 2, 3, 1).to(dtype), "nchw_to_nhwc")


@gpu
@pytest.mark.parametrize("clamp01", [False, True], ids=["plain", "clamp01"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_nhwc_to_nchw_second_pass(ops, dtype, clamp01):
    """channels [3, 7) of 8 of a typed NHWC source -> fp32 NCHW, * scale + shift separately rounded, clamped to [0, 1] or not"""
    from mv_ldm_amd import _lib as L
    x = layout_src().to(dtype)                                                                  # [5, 4, 323, 325], representable in dtype
    n, c, h, w = x.shape
    src = torch.full((n, h, w, 8), 3.0, dtype=dtype)
    src[..., 3:7] = x.permute(0, 2, 3, 1)
    buf, flat = flat_guarded(N2, F32)
    srcg = src.cuda()
    L.check(L.load().mvldm_nhwc_to_nchw(srcg.data_ptr(), flat.data_ptr(), n, c, HW2, 8, 3, ops.dt(dtype), LAYOUT_SCALE, LAYOUT_SHIFT, int(clamp01),
                                        ops.stream()))
    check_guard(buf, flat_owned(buf, N2), 7.0, "nhwc_to_nchw")
    want = x.float() * t32(LAYOUT_SCALE) + t32(LAYOUT_SHIFT)
    if clamp01:
        assert 0.05 < float((want < 0).float().mean()) and 0.05 < float((want > 1).float().mean())
        want = want.clamp(0, 1)
    bit_equal(flat.view(n, c, h, w).cpu(), want, f"nhwc_to_nchw clamp01 {clamp01}")


@gpu
def test_posterior_sample_second_pass(ops):
    """2 099 500 elements, both clamps of logvar in the same run; the bound of test_posterior_sample_and_mapped_layout, 2e-6 of the torch fp32
    expression element by element.  The device's expf and torch's exp may differ in the last place, and a RELATIVE bound on mean + std x noise
    carries that over only where the two terms do not cancel (with random signs some of the 2 M elements end up 1.8e-3 apart, from an
    std one unit in the last place apart): the noise takes the sign of the mean here, so the bound is a statement about expf"""
    from mv_ldm_amd import _lib as L
    g = G(7400)
    mom = torch.randn(5, 8, 323, 325, generator=g) * 3
    mom[0, 4:], mom[1, 4:] = 40.0, -50.0
    noise = torch.randn(5, 4, 323, 325, generator=g).abs() * torch.sign(mom[:, :4])
    ref = (mom[:, :4] + torch.exp(0.5 * mom[:, 4:].clamp(-30.0, 20.0)) * noise) * 0.18215
    buf, flat = flat_guarded(N2, F32)
    momg, noiseg = mom.cuda(), noise.cuda()
    L.check(L.load().mvldm_posterior_sample(momg.data_ptr(), noiseg.data_ptr(), flat.data_ptr(), 5, 4, HW2, 0.18215, ops.stream()))
    check_guard(buf, flat_owned(buf, N2), 7.0, "posterior_sample")
    got = flat.view(5, 4, 323, 325).cpu()
    record_err("posterior/rel", float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max()))
    assert bool(((got - ref).abs() <= 2e-6 * ref.abs() + 1e-30).all())
    assert float(got[0].abs().max()) > 1e3                                                   # exp(0.5 x 20) was at work


@gpu
@pytest.mark.parametrize("n,dim", [(7, 6), (6, 320)])
def test_timestep_embedding_sin_first(ops, n, dim):
    """flip_sin_to_cos = 0: [sin | cos], against the oracle Timesteps; far below one workgroup and the production width"""
    from oracle.blocks import Timesteps
    t = torch.tensor([0, 1, 20, 333, 980, 999, 500][:n], dtype=torch.int64)
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)
    ref = Timesteps(dim, flip_sin_to_cos=False)(t)
    assert torch.equal(ref[:, :half], torch.sin(t[:, None].float() * freqs[None, :]))               # the explicit sin | cos order
    for dtype, bound in ((F32, 2e-6), (BF16, 4e-3)):
        y = ops.timestep_embed(t.cuda(), freqs.cuda(), dim, False, dtype=dtype)
        e = record_err(f"temb_sin_first/{NAME[dtype]}", float((y.float().cpu() - ref).abs().max()))
        assert e < bound, (n, dim, dtype, e)
    if dim > 6:
        assert not torch.allclose(ref, Timesteps(dim, flip_sin_to_cos=True)(t))


def run_eltwise(ops, x, op, dst_dtype):
    from mv_ldm_amd import _lib as L
    buf, y = flat_guarded(x.numel(), dst_dtype)
    L.check(L.load().mvldm_eltwise_fwd(x.data_ptr(), y.data_ptr(), x.numel(), op, ops.dt(x), ops.dt(dst_dtype), ops.stream()))
    check_guard(buf, flat_owned(buf, x.numel()), 7.0, f"eltwise op {op} {x.dtype} -> {dst_dtype}")
    return y


@gpu
@pytest.mark.parametrize("dst", DTYPES, ids=["to_f32", "to_bf16", "to_f16"])
@pytest.mark.parametrize("src", DTYPES, ids=["f32", "bf16", "f16"])
def test_eltwise_copy_converts_like_torch(ops, src, dst):
    """all nine source x destination pairs: equal to torch's conversion (f16 overflow to inf included); one element, 1077, and f32 -> 16-bit
    above the second pass"""
    sizes = [1, 1077] + ([N2] if src == F32 and dst != F32 else [])
    for n in sizes:
        x = (torch.randn(n, generator=G(7500 + n % 97)) * torch.logspace(-6, 6, n)).to(src)
        bit_equal(run_eltwise(ops, x.cuda(), 0, dst).cpu(), x.to(dst), f"copy {NAME[src]} -> {NAME[dst]} n = {n}")


@gpu
@pytest.mark.parametrize("dst", DTYPES, ids=["to_f32", "to_bf16", "to_f16"])
@pytest.mark.parametrize("op,fn", [(1, F.silu), (2, F.gelu)], ids=["silu", "gelu"])
def test_eltwise_silu_and_gelu(ops, op, fn, dst):
    """MVLDM_ELT_SILU and MVLDM_ELT_GELU from fp32 into each destination type, above the second pass and for one element"""
    from mv_ldm_amd import _lib as L
    assert (L.ELT_SILU, L.ELT_GELU) == (1, 2)
    x = urnd((N2,), 7600 + op, F32, -4.0, 4.0)
    close(run_eltwise(ops, x.cuda(), op, dst), fn(x.double()), dst, f"glue_eltwise/{'silu' if op == 1 else 'gelu'}", f"n = {N2}")
    one = t32([0.7])
    close(run_eltwise(ops, one.cuda(), op, dst), fn(one.double()), dst, None, "n = 1")


@gpu
def test_gather_rows_second_pass(ops):
    """2049 rows of 1025 chunks with both index vectors (test_gather_rows_is_exact has the small cases): exact, untouched rows keep the fill"""
    n_rows, cpr = GATHER2
    g, w = G(7700), cpr * 4
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_rows + 7, w), generator=g, dtype=torch.int32)
    si = torch.randint(0, n_rows + 7, (n_rows,), generator=g, dtype=torch.int32)
    di = torch.randperm(n_rows + 13, generator=g)[:n_rows].to(torch.int32)
    buf, flat = flat_guarded((n_rows + 13) * w, torch.int32, 7)
    dst = flat.view(n_rows + 13, w)
    ops.gather_rows(src.cuda(), dst, si.cuda(), di.cuda(), n_rows=n_rows)
    check_guard(buf, flat_owned(buf, (n_rows + 13) * w), 7, "gather_rows")
    want = torch.full((n_rows + 13, w), 7, dtype=torch.int32)
    want[di.long()] = src[si.long()]
    bit_equal(dst.cpu(), want, "gather_rows")


# ------------------------------------------------------------------------------------------------ E. elementwise training kernels
E_DTYPES, E_IDS = [F32, BF16], ["f32", "bf16"]


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def silu_grad64(x):
    s = torch.sigmoid(x)
    return s * (1.0 + x * (1.0 - s))


@gpu
@pytest.mark.parametrize("a_dtype,dtype", [(F32, F32), (BF16, BF16), (F32, BF16)], ids=["f32", "bf16", "f32_x_bf16_dy"])
@pytest.mark.parametrize("op,grad", [(0, silu_grad64), (4, gelu_grad64)], ids=["silu_bwd", "gelu_bwd"])
def test_activation_backward_second_pass(ops, op, grad, a_dtype, dtype):
    """2^21 + 1 elements: one thread takes a second pass; the pre-activation in the gradient's type and in fp32 under bf16 gradients"""
    from mv_ldm_amd import _lib as L
    assert (L.TE_SILU_BWD, L.TE_GELU_BWD) == (0, 4)
    x, dy = urnd((ELT2,), 8000 + op, a_dtype, -4.0, 4.0), urnd((ELT2,), 8001 + op, dtype)
    buf, out = flat_guarded(ELT2, dtype)
    ops.train_eltwise(op, x.to(a_dtype).cuda(), dy.to(dtype).cuda(), out, 1, ELT2)
    check_guard(buf, flat_owned(buf, ELT2), 7.0, "activation backward")
    close(out, dy.double() * grad(x.double()), dtype, f"glue_train/{'silu_bwd' if op == 0 else 'gelu_bwd'}{'_f32x' if a_dtype != dtype else ''}", f"n = {ELT2}")


@gpu
@pytest.mark.parametrize("dtype", E_DTYPES, ids=E_IDS)
def test_add_second_pass_and_ragged_refusal(ops, dtype):
    """a += b over 2^21 + 1 chunks: the fp32 sum rounded once, exactly; an element count that is no whole number of chunks is refused and
    nothing is written"""
    from mv_ldm_amd import _lib as L
    n = ELT2 * epc(dtype)
    a0, b = urnd((n,), 8100, dtype), urnd((n,), 8101, dtype)
    buf, a = flat_guarded(n, dtype)
    a.copy_(a0.to(dtype))
    ops.train_eltwise(L.TE_ADD, b.to(dtype).cuda(), None, a, 1, n)
    check_guard(buf, flat_owned(buf, n), 7.0, "add")
    bit_equal(a.cpu(), (a0 + b).to(dtype), "add")
    small = torch.full((64,), 7.0, dtype=dtype, device="cuda")
    rc = L.load().mvldm_train_eltwise(L.TE_ADD, small.data_ptr(), None, small.data_ptr(), 1, epc(dtype) * 3 + 1, ops.dt(dtype), ops.dt(dtype), ops.stream())
    torch.cuda.synchronize()
    assert rc == ERR_ARG and bool((small == 7.0).all())


def geglu_case(dtype):
    rows, dc = GEGLU2
    D = dc * epc(dtype)
    ag, dh = urnd((rows, 2 * D), 8200, dtype), urnd((rows, D), 8201, dtype)
    a, gate, d = ag[:, :D].double(), ag[:, D:].double(), dh.double()
    gelu = F.gelu(gate)
    return dict(ag=ag, dh=dh, D=D, h=a * gelu, dag=torch.cat([d * gelu, d * a * gelu_grad64(gate)], dim=1))


@gpu
@pytest.mark.parametrize("dtype", E_DTYPES, ids=E_IDS)
def test_geglu_forward_and_backward_second_pass(ops, dtype):
    """699 051 rows of 3 chunks = 2^21 + 1 work items (the row / column split of the index is at work in every pass)"""
    from mv_ldm_amd import _lib as L
    k = geglu_case(dtype)
    rows, D = GEGLU2[0], k["D"]
    agg = k["ag"].to(dtype).cuda()
    buf, flat = flat_guarded(rows * D, dtype)
    ops.train_eltwise(L.TE_GEGLU_FWD, agg, None, flat, rows, D)
    check_guard(buf, flat_owned(buf, rows * D), 7.0, "geglu_fwd")
    close(flat.view(rows, D), k["h"], dtype, "glue_train/geglu_fwd", f"{rows} x {D}")
    buf, flat = flat_guarded(rows * 2 * D, dtype)
    ops.train_eltwise(L.TE_GEGLU_BWD, agg, k["dh"].to(dtype).cuda(), flat, rows, D)
    check_guard(buf, flat_owned(buf, rows * 2 * D), 7.0, "geglu_bwd")
    close(flat.view(rows, 2 * D), k["dag"], dtype, "glue_train/geglu_bwd", f"{rows} x {D}")


@gpu
@pytest.mark.parametrize("dtype", E_DTYPES, ids=E_IDS)
def test_pool2x2_second_pass(ops, dtype):
    """2^21 + 1 output chunks: (a + b) + (d + e) in fp32, in the kernel's order, rounded once -- exactly"""
    from mv_ldm_amd import _lib as L
    n, h, w, cc = POOL2
    c = cc * epc(dtype)
    du = urnd((n, 2 * h, 2 * w, c), 8300, dtype)
    v = du.view(n, h, 2, w, 2, c)
    want = ((v[:, :, 0, :, 0] + v[:, :, 0, :, 1]) + (v[:, :, 1, :, 0] + v[:, :, 1, :, 1])).to(dtype)
    buf, flat = flat_guarded(n * h * w * c, dtype)
    dug = du.to(dtype).cuda()
    L.check(L.load().mvldm_pool2x2_sum(dug.data_ptr(), flat.data_ptr(), n, h, w, c, ops.dt(dtype), ops.stream()))
    check_guard(buf, flat_owned(buf, n * h * w * c), 7.0, "pool2x2")
    bit_equal(flat.view(n, h, w, c).cpu(), want, "pool2x2")


@gpu
@pytest.mark.parametrize("dtype", E_DTYPES, ids=E_IDS)
def test_zero_insert_second_pass(ops, dtype):
    """4 x (2^19 + 1) output chunks: the source at the even positions, zero elsewhere, exactly"""
    from mv_ldm_amd import _lib as L
    n, h, w, cc = ZERO2
    c = cc * epc(dtype)
    x = urnd((n, h, w, c), 8400, dtype).to(dtype)
    want = torch.zeros(n, 2 * h, 2 * w, c, dtype=dtype)
    want[:, ::2, ::2] = x
    buf, flat = flat_guarded(want.numel(), dtype)
    xg = x.cuda()
    L.check(L.load().mvldm_zero_insert2x(xg.data_ptr(), flat.data_ptr(), n, h, w, c, ops.dt(dtype), ops.stream()))
    check_guard(buf, flat_owned(buf, want.numel()), 7.0, "zero_insert")
    bit_equal(flat.view(want.shape).cpu(), want, "zero_insert")
