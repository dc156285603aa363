"""GPU parity of the WEIGHT-GRADIENT kernels (csrc/wgrad.hip) at their edges: both forms (register-staged `wgrad_kernel`, wide LDS-DMA
`wgrad_dma_kernel`) at every split target the plan-time tuner may freeze (plan._WGRAD_TARGETS, bits 10-12 of `accumulate`), the
workspace cap, non-square and odd maps, a skip concat whose channel tile straddles the two sources, Linears as column slices of a wider
`dy` -- with the gradient and the slab workspace SLICES OF LARGER POISONED BUFFERS.  The sibling of test_hip_backward_edges.py (bounds)
and test_hip_forward_edges.py (guards).

References: torch.autograd on the CPU in fp64, from the SAME dtype-rounded inputs, built once per case (functools.lru_cache; shared, never
written to).

Guards: the gradient is rows [row0, row0 + n_out) of an fp32 buffer with GUARD_ROWS = 320 further rows (the tallest tile), prefilled with
-7.0 -- with accumulate = 0 the interior too, so that every element must be written.  The slab workspace is the leading bytes of a uint8
buffer prefilled with 0xA5 that is one slab longer than what the library is told; everything past `splits * slab` bytes (`splits` from the
restated rule; nothing at all on the direct single-split path) must still hold the fill.  `dy` and `x` are followed by 640 rows / as many images
of 3.0, so that a read past the split's range changes a value instead of finding allocator zeros.  Guards are compared bit for bit after each
launch, before any value (`check_guard` of test_hip_forward_edges.py).

Bounds (never from a kernel): tests/grad_emulation.py, kind `wgrad_long`, evaluates the kernels' documented arithmetic in torch on the CPU
-- products of the dtype-rounded operands, fp32 accumulation over the pixel index in steps of 16, one partial per split of `rows_per_split`
rows (the restated rule), partials added in split order in fp32, the accumulate case added onto the previous gradient -- against the fp64
reference, over every (case, form, target, workspace) of a family below.  A bound is 3 x the family's emulated value (the project's factor:
a different summation order, the extreme-value spread), for the relative L2 AND the worst element over the reference's RMS; the relative L2
is never looser than TOL[dtype] of test_hip_backward.py, and where no sum of a family is longer than the 300 pixels WORST["wgrad"] of
test_hip_backward_edges.py was emulated on, the worst element is never looser than that either.  `python tests/grad_emulation.py` prints:

    wgrad_long   longest sum     emulated worst element / RMS      emulated relative L2              bound: worst (3 x)                bound: rel. L2 (3 x)
    family       (pixels)            f32      bf16       f16           f32      bf16       f16           f32      bf16       f16           f32      bf16       f16
    sweep        2048           9.45e-07  1.86e-06  2.03e-06      1.33e-07  2.05e-07  2.14e-07      2.83e-06  5.57e-06  6.10e-06      4.00e-07  6.16e-07  6.42e-07
    cap          4096                  -  3.10e-06  3.73e-06             -  2.87e-07  2.91e-07             -  9.29e-06  1.12e-05             -  8.62e-07  8.72e-07
    maps         320                   -  1.01e-06  1.05e-06             -  8.40e-08  1.08e-07             -  3.04e-06  3.15e-06             -  2.52e-07  3.23e-07
    gather       120            5.77e-07  4.74e-07  5.34e-07      8.88e-08  4.93e-08  8.23e-08      1.73e-06  1.42e-06  1.60e-06      2.66e-07  1.48e-07  2.47e-07
    concat       300            7.78e-07  9.38e-07  6.45e-07      1.11e-07  8.20e-08  1.05e-07      2.33e-06  2.81e-06  1.94e-06      3.32e-07  2.46e-07  3.16e-07
    linear       320            6.59e-07  6.85e-07  7.10e-07      1.24e-07  9.88e-08  1.19e-07      1.98e-06  2.05e-06  2.13e-06      3.73e-07  2.97e-07  3.58e-07

Every bounded value goes to conftest.record_err; tests/golden/measured_errors_wgrad_edges.json is one MVLDM_TEST_REPORT run on an MI355X.
A kernel that exceeds 3 x its emulation is a finding about the kernel, not about the factor.

Only the three CPU tests (launch rules, workgroup map, the checks' self-test) are unmarked; every other test carries the gpu mark.

Found by this module: wgrad_kernel<float> chained its v_mfma_f32_32x32x2_f32 over the whole split, two pixels per fp32 addition -- 8 x as
many dependent additions as the 16-pixel steps of the 16-bit MFMAs and of the emulation.  On an MI355X the 3x3 straddling concat in f32
had a worst element of 3.43e-06 x RMS against its bound of 2.33e-06, and the f32 sweep sat at 2.76e-06 / 2.83e-06 (relative L2 3.95e-07 /
3.99e-07).  The kernel now sums 16 pixels into a fresh partial and adds that once; the same cases measure 7.78e-07 and 9.45e-07 (relative
L2 1.33e-07), the emulated values.  The two claims of wgrad.hip's comments held as written: the two forms are bit-identical over the same
split ranges, and accumulate = 1 is g0 + the same reduced sum.

The one-split-per-XCD map exists in experiment builds only (the product library reads no environment variable), so its device test
compiles wgrad.hip alone with -DMVLDM_EXPERIMENTS (4 s) next to the product library instead of setting the knob against the product.
"""
import functools
import hashlib
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import record_err
from test_hip_backward import TOL, G, rnd
from test_hip_backward_edges import WORST, worst_over_rms
from test_hip_forward_edges import check_guard

GRAD_ENABLED = True       # tests/conftest.py::_grad_mode: torch references are differentiated here
gpu = pytest.mark.gpu
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES, HALF = [F32, BF16, F16], [BF16, F16]
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "mv_ldm_amd" / "csrc"
GUARD_ROWS = 320          # the tallest tile: WD_BN of the wide form
GRAD_FILL, WS_FILL, JUNK = -7.0, 0xA5, 3.0
JUNK_ROWS = 640           # rows of JUNK behind dy and x: the longest split here that ends past M (7 x 640 rows over M = 4096)
SWEEP_SLABS = 32.0        # the sweep's caller-owned workspace, in slabs


@pytest.fixture(scope="module")
def ops():
    from mv_ldm_amd import ops as O
    from mv_ldm_amd import _lib as L
    L.load()
    return O


def epc(dtype):
    return 4 if dtype == F32 else 8


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ cases
def _c(n, h, w, c0, co, ks=3, stride=1, pad=None, up=False, c1=0):
    return dict(n=n, h=h, w=w, c0=c0, c1=c1, co=co, ks=ks, stride=stride, pad=ks // 2 if pad is None else pad, up=up)


CASES = {
    "sweep": _c(8, 16, 32, 192, 320), "sweep4": _c(4, 16, 32, 192, 320),                               # M = 4096 / 2048 (f32)
    "map8x32": _c(3, 8, 32, 64, 160), "map32x4": _c(5, 32, 4, 72, 200), "map4x8": _c(3, 4, 8, 128, 320),
    "map1x64": _c(2, 1, 64, 64, 160), "map64x1": _c(2, 64, 1, 64, 160),
    "g5x7": _c(3, 5, 7, 24, 40), "g7x5s2": _c(2, 7, 5, 24, 40, stride=2), "g3x5up": _c(2, 3, 5, 24, 40, up=True),
    "g6x9p0": _c(2, 6, 9, 24, 40, pad=0), "g5x7big": _c(3, 5, 7, 72, 136),
    "cat3x3": _c(3, 6, 10, 72, 136, c1=40), "cat1x1": _c(300, 1, 1, 72, 136, ks=1, c1=40),
    "lin2051": _c(2051, 1, 1, 136, 328, ks=1), "lin777": _c(777, 1, 1, 1032, 168, ks=1),
}
MAPS = ["map8x32", "map32x4", "map4x8", "map1x64", "map64x1"]
GATHER = ["g5x7", "g7x5s2", "g3x5up", "g6x9p0", "g5x7big"]
CONCAT = ["cat3x3", "cat1x1"]
LINEARS = ["lin2051", "lin777"]
DY_SIDE = 8               # a Linear's dy is columns [8, 8 + n_out) of a [rows, n_out + 24] tensor
GRAD_ROW0 = 8             # ... and its gradient rows [8, 8 + n_out) of the guarded buffer


def geom(c):
    """-> (h_out, w_out, M, taps, ctot)"""
    hs, ws = (2 * c["h"], 2 * c["w"]) if c["up"] else (c["h"], c["w"])
    ho, wo = (hs + 2 * c["pad"] - c["ks"]) // c["stride"] + 1, (ws + 2 * c["pad"] - c["ks"]) // c["stride"] + 1
    return ho, wo, c["n"] * ho * wo, c["ks"] ** 2, c["c0"] + c["c1"]


def slab_bytes(c):
    _, _, _, taps, ctot = geom(c)
    return c["co"] * taps * ctot * 4


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """dtype-rounded inputs (NCHW, both sources of a concat in one tensor), the upstream gradient and the fp64 autograd weight gradient
    ([co, c, k, k]; [co, c] for a Linear).  Shared: do not write to it."""
    c = CASES[name]
    seed = 400 + 10 * list(CASES).index(name)
    ho, wo, M, taps, ctot = geom(c)
    x = rnd((c["n"], ctot, c["h"], c["w"]), seed, dtype)
    w = rnd((c["co"], ctot, c["ks"], c["ks"]), seed + 1, dtype, 1 / math.sqrt(ctot * taps))
    dy = rnd((c["n"], c["co"], ho, wo), seed + 2, dtype)
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    with torch.enable_grad():
        wd = w.double().requires_grad_()
        xin = F.interpolate(x.double(), scale_factor=2, mode="nearest") if c["up"] else x.double()
        y = F.conv2d(xin, wd, None, c["stride"], c["pad"])
        assert tuple(y.shape) == tuple(dy.shape)
        gw, = torch.autograd.grad(y, (wd,), dy.double())
    gw = gw.reshape(c["co"], ctot) if c["ks"] == 1 else gw
    g0 = rnd(tuple(gw.shape), seed + 3, F32, float(gw.pow(2).mean().sqrt()) / 8)      # the previous gradient of the accumulate case
    return dict(c, name=name, x=x, dy=dy, gw=gw.detach(), g0=g0)


# ------------------------------------------------------------------------------------------------ launch rules, restated
# The host rules that decide the form, the split count and the rows of a split are restated here, and the source is required to still state
# them: a later change of a rule fails the CPU test instead of silently moving a case off the branch it is named for.
RULES_IN_SOURCE = [
    ("csrc/wgrad.hip", "constexpr int WG_BN = 128, WG_BC = 64, WG_BP = 64;"),
    ("csrc/wgrad.hip", "constexpr int WD_BN = 320, WD_BC = 128;"),
    ("csrc/wgrad.hip", "p.tiles_n = cdiv_(d.n_out, WG_BN); p.tiles_c = cdiv_(p.ctot, WG_BC);"),
    ("csrc/wgrad.hip", "const int tiles = p.tiles_n * p.taps * p.tiles_c; const int blocks = cdiv_(p.M, WG_BP);"),
    ("csrc/wgrad.hip", 'static const int kTarget = knob_int("MVLDM_WGRAD_TARGET", 512);'),
    ("csrc/wgrad.hip", "const int target = tcode ? (64 << tcode) : kTarget;"),
    ("csrc/wgrad.hip", "splits = std::max(1, std::min(cdiv_(target, tiles), std::max(1, blocks / 4)));"),
    ("csrc/wgrad.hip", "const size_t slab = (size_t)d.n_out * p.kdim * sizeof(float); while (splits > 1 && (size_t)splits * slab > d.workspace_bytes) --splits;"),
    ("csrc/wgrad.hip", "MVLDM_REQUIRE(d.workspace && (size_t)splits * slab <= d.workspace_bytes,"),
    ("csrc/wgrad.hip", "p.rows_per_split = cdiv_(blocks, splits) * WG_BP; splits = cdiv_(p.M, p.rows_per_split);"),
    ("csrc/wgrad.hip", "p.tiles_n = cdiv_(d.n_out, WD_BN); p.tiles_c = cdiv_(p.ctot, WD_BC);"),
    ("csrc/wgrad.hip", "const int tiles = p.tiles_n * p.taps * p.tiles_c, blocks = cdiv_(p.M, 64);"),
    ("csrc/wgrad.hip", 'static const int kTarget = knob_int("MVLDM_WGRAD_WIDE_TARGET", 256);'),
    ("csrc/wgrad.hip", "splits = std::max(1, std::min(target / std::max(tiles, 1), std::max(1, blocks / 4)));"),
    ("csrc/wgrad.hip", "MVLDM_REQUIRE((size_t)splits * slab <= d.workspace_bytes,"),
    ("csrc/wgrad.hip", "p.rows_per_split = cdiv_(blocks, splits) * 64; splits = cdiv_(p.M, p.rows_per_split);"),
    ("csrc/wgrad.hip", "const int m_begin = split * p.rows_per_split, m_end = min(p.M, m_begin + p.rows_per_split);"),
    ("csrc/wgrad.hip", "return on && splits == 1 && p.taps == 1 && d.c_in == p.ctot && (d.accumulate & 1) == 0;"),
    ("csrc/wgrad.hip", "if (d.act_dtype == MVLDM_F32 || d.src1 || d.c1 || d.stride != 1 || d.upsample) return false;"),
    ("csrc/wgrad.hip", "if (d.n_out < 160 || d.c0 < 64 || d.c0 % 8 || d.dy_ld % 8) return false;"),
    ("csrc/wgrad.hip", "if (d.ksize == 3 && (d.pad != 1 || d.h_in != d.h_out || d.w_in != d.w_out || ilog2_exact(d.w_out) < 0 || ilog2_exact(d.h_out) < 0)) return false;"),
    ("csrc/wgrad.hip", "if (d.ksize == 1 && (d.pad != 0 || d.h_in != d.h_out || d.w_in != d.w_out)) return false;"),
    ("csrc/wgrad.hip", "const int form = (d0.accumulate >> 8) & 3; MVLDM_REQUIRE(form != 2 || wgrad_wide_ok(d0), \"wgrad: the wide form does not take this problem\");"),
    ("csrc/wgrad.hip", "const int tcode = (d0.accumulate >> 10) & 7;"),
    ("csrc/wgrad.hip", "const int ox = m & wmask, oy = (m >> q.lw) & hmask;"),
    ("csrc/wgrad.hip", "const bool from0 = ch < p.c0;"),
    # the workgroup map
    ("csrc/wgrad.hip", "const int b = blockIdx.x, xcd = b & 7, i = b >> 3; if (!p.xcd_map) { tile = b % p.n_tiles; split = b / p.n_tiles; return split < p.n_splits; }"),
    ("csrc/wgrad.hip", "if (p.n_splits >= 8) { tile = i % p.n_tiles; split = (i / p.n_tiles) * 8 + xcd; return split < p.n_splits; }"),
    ("csrc/wgrad.hip", "split = xcd % p.n_splits; const int rank = xcd / p.n_splits, cnt = (8 - split + p.n_splits - 1) / p.n_splits;"),
    ("csrc/wgrad.hip", "tile = i * cnt + rank; return tile < p.n_tiles;"),
    ("csrc/wgrad.hip", "if (!kWgXcd) return tiles * splits; return splits >= 8 ? 8 * ((splits + 7) / 8) * tiles : 8 * ((tiles + (8 / splits) - 1) / (8 / splits));"),
    # the host side
    ("ops.py", 'scratch = workspace(min(max(need * 8, 1 << 20), max(need, 512 << 20)), x.device, "wgrad")'),
    ("ops.py", "int(accumulate) | (int(form) << 8) | (int(target) << 10)"),
    ("plan.py", "v = form + 4 * tcode trial.u.wgrad.accumulate = (d.accumulate & 1) | (v << 8)"),
]


def _squeeze(text):
    return re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", text))


def cap_splits(splits, slab, ws_bytes):
    """the workspace cap of both forms -> the capped split count, None when not even one slab fits (the launch is refused)"""
    while splits > 1 and splits * slab > ws_bytes:
        splits -= 1
    return splits if splits * slab <= ws_bytes else None


def wgrad_plan(M, n_out, ctot, taps, code=0, ws_bytes=1 << 40):
    """wgrad.hip wgrad_plan, the register-staged form -> (planned splits, rows per split, splits that run) or None (refused)"""
    tiles, blocks = cdiv(n_out, 128) * taps * cdiv(ctot, 64), cdiv(M, 64)
    target = (64 << code) if code else 512
    planned = max(1, min(cdiv(target, tiles), max(1, blocks // 4)))
    splits = cap_splits(planned, n_out * taps * ctot * 4, ws_bytes)
    if splits is None:
        return None
    rps = cdiv(blocks, splits) * 64
    return planned, rps, cdiv(M, rps)


def wgrad_plan_wide(M, n_out, ctot, taps, code=0, ws_bytes=1 << 40):
    """wgrad.hip wgrad_run_wide (after wgrad_plan's argument and workspace checks)"""
    if wgrad_plan(M, n_out, ctot, taps, 0, ws_bytes) is None:
        return None
    tiles, blocks = cdiv(n_out, 320) * taps * cdiv(ctot, 128), cdiv(M, 64)
    target = (64 << code) if code else 256
    planned = max(1, min(target // max(tiles, 1), max(1, blocks // 4)))
    splits = cap_splits(planned, n_out * taps * ctot * 4, ws_bytes)
    if splits is None:
        return None
    rps = cdiv(blocks, splits) * 64
    return planned, rps, cdiv(M, rps)


def pow2(v):
    return v > 0 and v & (v - 1) == 0


def wide_ok(c, dtype, dy_ld=None):
    """wgrad.hip wgrad_wide_ok"""
    ho, wo, M, taps, ctot = geom(c)
    dy_ld = c["co"] if dy_ld is None else dy_ld
    if dtype == F32 or c["c1"] or c["stride"] != 1 or c["up"]:
        return False
    if c["co"] < 160 or c["c0"] < 64 or c["c0"] % 8 or dy_ld % 8:
        return False
    if c["ks"] == 3 and (c["pad"] != 1 or (c["h"], c["w"]) != (ho, wo) or not pow2(wo) or not pow2(ho)):
        return False
    if c["ks"] == 1 and (c["pad"] != 0 or (c["h"], c["w"]) != (ho, wo)):
        return False
    return c["n"] * c["h"] * c["w"] * c["c0"] * 2 < 0xFFFFFFF0


def launch_plan(name, dtype, form, code=0, ws_slabs=SWEEP_SLABS, accumulate=False):
    """an explicitly requested form -> dict(planned, rps, splits, direct) or None when the library refuses the launch"""
    c = CASES[name]
    _, _, M, taps, ctot = geom(c)
    if form == 2 and not wide_ok(c, dtype, c["co"] + 3 * DY_SIDE if name in LINEARS else None):
        return None
    r = (wgrad_plan_wide if form == 2 else wgrad_plan)(M, c["co"], ctot, taps, code, int(ws_slabs * slab_bytes(c)))
    if r is None:
        return None
    planned, rps, splits = r
    return dict(planned=planned, rps=rps, splits=splits, direct=splits == 1 and taps == 1 and not accumulate)      # (c_in == ctot in every case here)


def forms_of(name, dtype):
    return [f for f in (1, 2) if launch_plan(name, dtype, f) is not None]


# (form, code) -> (rows per split, splits that run) of the sweep case; codes 0 and 2 of form 2 PLAN 14 splits
SWEEP_TABLE = {(1, 0): (640, 7), (1, 1): (2048, 2), (1, 2): (1024, 4), (1, 3): (640, 7), (1, 4): (320, 13), (1, 5): (256, 16),
               (2, 0): (320, 13), (2, 1): (640, 7), (2, 2): (320, 13), (2, 3): (256, 16), (2, 4): (256, 16), (2, 5): (256, 16)}
SWEEP_F32 = {(1, 0): (320, 7), (1, 2): (512, 4), (1, 5): (256, 8)}            # 4 images, M = 2048
CAP_SLABS = {1.5: (4096, 1), 2.5: (2048, 2), 5.5: (832, 5)}                    # workspace in slabs -> (rows per split, splits), both forms


def wg_grid(tiles, splits, xcd):
    return tiles * splits if not xcd else 8 * cdiv(splits, 8) * tiles if splits >= 8 else 8 * cdiv(tiles, 8 // splits)


def wg_map(b, tiles, splits, xcd):
    """wgrad.hip wg_map over an array of workgroup ids -> (tile, split, valid)"""
    x, i = b & 7, b >> 3
    if not xcd:
        return b % tiles, b // tiles, b // tiles < splits
    if splits >= 8:
        s = (i // tiles) * 8 + x
        return i % tiles, s, s < splits
    s = x % splits
    rank, cnt = x // splits, (8 - s + splits - 1) // splits
    t = i * cnt + rank
    return t, s, t < tiles


# ------------------------------------------------------------------------------------------------ bounds
# (emulated worst element / RMS, emulated relative L2) per family and dtype: the table of the module docstring (tests/grad_emulation.py);
# `longest`: the longest fp32 sum of the family in pixels
EMU = {
    "sweep": {"longest": 2048, F32: (9.45e-07, 1.33e-07), BF16: (1.86e-06, 2.05e-07), F16: (2.03e-06, 2.14e-07)},
    "cap": {"longest": 4096, BF16: (3.10e-06, 2.87e-07), F16: (3.73e-06, 2.91e-07)},
    "maps": {"longest": 320, BF16: (1.01e-06, 8.40e-08), F16: (1.05e-06, 1.08e-07)},
    "gather": {"longest": 120, F32: (5.77e-07, 8.88e-08), BF16: (4.74e-07, 4.93e-08), F16: (5.34e-07, 8.23e-08)},
    "concat": {"longest": 300, F32: (7.78e-07, 1.11e-07), BF16: (9.38e-07, 8.20e-08), F16: (6.45e-07, 1.05e-07)},
    "linear": {"longest": 320, F32: (6.59e-07, 1.24e-07), BF16: (6.85e-07, 9.88e-08), F16: (7.10e-07, 1.19e-07)},
}


def bound(family, dtype):
    """-> (relative L2, worst element / RMS): 3 x the emulation, never looser than the bounds the older tests hold the same kernels to"""
    worst, l2 = EMU[family][dtype]
    return min(3 * l2, TOL[dtype]), (min(3 * worst, WORST["wgrad"][dtype]) if EMU[family]["longest"] <= 300 else 3 * worst)


def errors(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30)), worst_over_rms(got, ref)


def close(got, ref, dtype, family, what=""):
    assert torch.isfinite(got).all(), f"{what}: non-finite gradient"
    e2, emax = errors(got, ref)
    if family != "selftest":
        record_err(f"{family}/rel_l2/{NAME[dtype]}", e2)
        record_err(f"{family}/worst_over_rms/{NAME[dtype]}", emax)
    l2b, wb = bound("sweep" if family == "selftest" else family, dtype)
    print(f"close {family} {what}: rel-L2 {e2:.3e} (tol {l2b:.2e}), worst/rms {emax:.3e} (tol {wb:.2e})")
    assert e2 <= l2b and emax <= wb, f"{family} {what}: rel-L2 {e2:.3e} (tol {l2b:.2e}), worst element / rms {emax:.3e} (tol {wb:.2e})"


def emulation_runs(dtype):
    """every (family, case, rows per split, accumulate) the GPU tests below launch in `dtype`: what tests/grad_emulation.py evaluates"""
    runs = set()
    if dtype == F32:
        runs |= {("sweep", "sweep4", rps, False) for rps, _ in SWEEP_F32.values()} | {("sweep", "sweep4", SWEEP_F32[(1, 0)][0], True)}
    else:
        runs |= {("sweep", "sweep", rps, False) for rps, _ in SWEEP_TABLE.values()}
        runs |= {("sweep", "sweep", SWEEP_TABLE[k][0], True) for k in ((1, 0), (2, 0))}
        runs |= {("cap", "sweep", rps, False) for rps, _ in CAP_SLABS.values()}
    for family, names in (("maps", MAPS), ("gather", GATHER), ("concat", CONCAT), ("linear", LINEARS)):
        for name in names if family != "maps" or dtype != F32 else []:
            for form in forms_of(name, dtype):
                runs.add((family, name, launch_plan(name, dtype, form)["rps"], False))
    return sorted(runs)


# ------------------------------------------------------------------------------------------------ CPU tests
def test_cases_reach_the_branches_they_are_named_for():
    """CPU only: the restated launch rules put every case where the tables above say, and the source still states those rules"""
    from mv_ldm_amd import plan
    for name, text in RULES_IN_SOURCE:
        assert _squeeze(text) in _squeeze((ROOT / "mv_ldm_amd" / name).read_text()), f"{name} no longer states: {text}"
    assert plan._WGRAD_TARGETS == (0, 1, 2, 3, 4, 5), "a new tuner candidate: sweep it in SWEEP_TABLE"
    assert sorted(SWEEP_TABLE) == [(f, t) for f in (1, 2) for t in plan._WGRAD_TARGETS]
    # the sweep: 12 candidates, 5 distinct (rows per split, splits); two of form 2 run fewer splits than they plan
    c = CASES["sweep"]
    assert geom(c) == (16, 32, 4096, 9, 192) and slab_bytes(c) == 2211840
    for dtype in HALF:
        for (form, code), want in SWEEP_TABLE.items():
            p = launch_plan("sweep", dtype, form, code)
            assert (p["rps"], p["splits"]) == want and not p["direct"], (form, code, p)
            assert p["planned"] == (14 if (form, code) in ((2, 0), (2, 2)) else p["splits"])
            assert p["splits"] * slab_bytes(c) <= SWEEP_SLABS * slab_bytes(c) - slab_bytes(c)
    assert len(set(SWEEP_TABLE.values())) == 5 and max(s for _, s in SWEEP_TABLE.values()) == 16 > 8
    assert SWEEP_TABLE[(1, 0)] == SWEEP_TABLE[(2, 1)] and SWEEP_TABLE[(1, 4)] == SWEEP_TABLE[(2, 0)] and SWEEP_TABLE[(1, 5)] == SWEEP_TABLE[(2, 3)]
    for (form, code), want in SWEEP_F32.items():
        p = launch_plan("sweep4", F32, form, code)
        assert (p["rps"], p["splits"]) == want and launch_plan("sweep4", F32, 2) is None
    # the eager default workspace would have capped the sweep at 8 splits
    need = slab_bytes(c)
    eager = min(max(need * 8, 1 << 20), max(need, 512 << 20))
    assert eager == 8 * need and wgrad_plan(4096, 320, 192, 9, 5, eager)[2] == 8 and wgrad_plan_wide(4096, 320, 192, 9, 0, eager)[2] == 8
    # the workspace cap, and the refusal below one slab
    for slabs, want in CAP_SLABS.items():
        for form in (1, 2):
            p = launch_plan("sweep", BF16, form, 0, slabs)
            assert (p["rps"], p["splits"]) == want and p["planned"] in (7, 14), (slabs, form, p)
    assert launch_plan("sweep", BF16, 1, 0, 0.5) is None and launch_plan("sweep", BF16, 2, 0, 0.5) is None
    # non-square power-of-two maps: both forms, the split counts of the issue's table
    want = {"map8x32": (256, 3), "map32x4": (320, 2), "map4x8": (128, 1), "map1x64": (128, 1), "map64x1": (128, 1)}
    for name in MAPS:
        c = CASES[name]
        assert c["h"] != c["w"] and pow2(c["h"]) and pow2(c["w"])
        for dtype in HALF:
            assert forms_of(name, dtype) == [1, 2]
            for form in (1, 2):
                p = launch_plan(name, dtype, form)
                assert (p["rps"], p["splits"]) == want[name] and not p["direct"], (name, form, p)
        assert forms_of(name, F32) == [1]
    assert geom(CASES["map4x8"])[2] == 96 and 96 % 64 == 32                                   # one ragged 64-pixel step
    assert CASES["map32x4"]["c0"] % 64 and CASES["map32x4"]["co"] % 128 and CASES["map32x4"]["co"] % 320      # ragged c and n tiles
    # the general gather: register-staged form only; odd maps, stride 2, upsampling, pad 0
    assert [geom(CASES[n])[:2] for n in GATHER] == [(5, 7), (4, 3), (6, 10), (4, 7), (5, 7)]
    for name in GATHER + CONCAT:
        for dtype in DTYPES:
            assert forms_of(name, dtype) == [1], (name, dtype)
            assert CASES[name]["c0"] % epc(dtype) == 0 and CASES[name]["c1"] % epc(dtype) == 0 and CASES[name]["co"] % epc(dtype) == 0
    big = CASES["g5x7big"]
    assert big["c0"] > 64 and big["c0"] % 64 and big["co"] > 128 and big["co"] % 128              # two ragged tiles in n and in c
    # the straddling concat: the second 64-channel tile takes channels 64..71 from source 0 and 72..111 from source 1
    for name in CONCAT:
        c = CASES[name]
        assert (c["c0"], c["c1"], c["co"]) == (72, 40, 136) and 64 < c["c0"] < 128 and c["c0"] % 64
    assert geom(CASES["cat1x1"])[2] == 300 and geom(CASES["cat3x3"])[2] == 180
    # Linears: 7 and 3 splits with ragged last splits, both forms; one split and a written gradient would take the direct path
    for name, splits, last in (("lin2051", 7, 131), ("lin777", 3, 137)):
        M = CASES[name]["n"]
        for dtype in DTYPES:
            assert forms_of(name, dtype) == ([1] if dtype == F32 else [1, 2])
            for form in forms_of(name, dtype):
                p = launch_plan(name, dtype, form)
                assert (p["rps"], p["splits"]) == (320, splits) and M - (splits - 1) * 320 == last and not p["direct"]
    assert launch_plan("lin777", BF16, 1, 0, 1.5)["direct"] and not launch_plan("lin777", BF16, 1, 0, 1.5, accumulate=True)["direct"]
    # the bounds: never looser than what the older tests hold the same kernels to
    for family, row in EMU.items():
        for dtype in [t for t in DTYPES if t in row]:
            l2b, wb = bound(family, dtype)
            assert l2b <= TOL[dtype] and l2b <= 3 * row[dtype][1] and wb <= 3 * row[dtype][0]
            assert wb <= WORST["wgrad"][dtype] or row["longest"] > 300
    longest = {f: 0 for f in EMU}
    for dtype in DTYPES:
        for family, name, rps, _ in emulation_runs(dtype):
            longest[family] = max(longest[family], min(rps, geom(CASES[name])[2]))
    assert longest == {f: EMU[f]["longest"] for f in EMU}


def test_xcd_map_deals_every_tile_and_split_once():
    """CPU only: wg_map over a grid of wg_grid workgroups yields every (tile, split) exactly once and nothing else -- the default map and
    the one-split-per-XCD map (MVLDM_WGRAD_XCD=1 of experiment builds), splits 1..39 x tiles 1..99"""
    for xcd in (0, 1):
        for splits in range(1, 40):
            for tiles in range(1, 100):
                b = np.arange(wg_grid(tiles, splits, xcd))
                t, s, ok = wg_map(b, tiles, splits, xcd)
                t, s = np.broadcast_to(t, b.shape)[ok], np.broadcast_to(s, b.shape)[ok]
                assert t.size == tiles * splits and t.min() >= 0 and t.max() < tiles and s.min() >= 0 and s.max() < splits, (xcd, splits, tiles)
                assert np.unique(s * tiles + t).size == tiles * splits, (xcd, splits, tiles)
                if xcd and splits < 8:          # a split stays on the XCDs {x : x mod splits == split}
                    assert np.array_equal((b[ok] & 7) % splits, s)
                elif xcd:
                    assert np.array_equal(b[ok] & 7, s & 7)


def pixel_term(k, img, oy, ox):
    """the term of output pixel (img, oy, ox) in the fp64 gradient of a 3x3 / stride 1 / pad 1 case"""
    xp = F.pad(k["x"][img].double(), (1, 1, 1, 1))
    return torch.einsum("o,ckl->ockl", k["dy"][img, :, oy, ox].double(), xp[:, oy:oy + 3, ox:ox + 3])


def test_the_checks_can_fail():
    """CPU only: the sweep case's fp64 gradient with ONE pixel row of dy dropped breaks the worst-element bound by a wide margin (in every
    dtype's bound), and check_guard fires on one flipped element of a gradient guard row and of the workspace tail"""
    for dtype in HALF:
        k = case("sweep", dtype)
        close(k["gw"].clone(), k["gw"], dtype, "selftest")
        dropped = k["gw"] - pixel_term(k, 5, 9, 17)
        e2, emax = errors(dropped, k["gw"])
        l2b, wb = bound("sweep", dtype)
        assert emax > 100 * wb, (emax, wb)
        assert abs(e2 - 1 / 64) < 4e-3            # one of 4096 pixels: at the edge of TOL[bf16] = 1.2e-2, the relative L2 alone would not do
        with pytest.raises(AssertionError, match="worst element"):
            close(dropped, k["gw"], dtype, "selftest")
    buf = torch.full((40 + GUARD_ROWS, 27), GRAD_FILL)
    own = torch.zeros(buf.shape[0], 1, dtype=torch.bool)
    own[8:40] = True
    buf[8:40] = 1.0
    check_guard(buf, own, GRAD_FILL)
    for r, col in ((7, 26), (40, 0), (40 + GUARD_ROWS - 1, 26)):
        bad = buf.clone()
        bad[r, col] = GRAD_FILL + 1e-6
        with pytest.raises(AssertionError, match="guard elements written"):
            check_guard(bad, own, GRAD_FILL)
    ws = torch.full((4096,), WS_FILL, dtype=torch.uint8)
    check_guard(ws[1024:], torch.zeros(1, dtype=torch.bool), WS_FILL)
    ws[4095] = WS_FILL ^ 1
    with pytest.raises(AssertionError, match="guard elements written"):
        check_guard(ws[1024:], torch.zeros(1, dtype=torch.bool), WS_FILL)


# ------------------------------------------------------------------------------------------------ device launch
def device_inputs(k, dtype, dy_side=0):
    """x (x2) NHWC with further images of JUNK behind it, dy as [M, n_out] columns of a [M + JUNK_ROWS, ld] tensor whose further rows
    hold JUNK and whose further columns (dy_side on the left, 2 x dy_side on the right) other data"""
    n, c0, co = k["n"], k["c0"], k["co"]
    M = geom(k)[2]

    extra = cdiv(JUNK_ROWS, geom(k)[0] * geom(k)[1])         # images of JUNK: as many pixel rows as behind dy

    def source(t):
        buf = torch.full((n + extra, k["h"], k["w"], t.shape[1]), JUNK, dtype=dtype, device="cuda")
        buf[:n] = t.permute(0, 2, 3, 1).to(dtype)
        return buf[:n]
    xa = source(k["x"][:, :c0])
    xb = source(k["x"][:, c0:]) if k["c1"] else None
    dyb = torch.full((M + JUNK_ROWS, co + 3 * dy_side), JUNK, dtype=dtype, device="cuda")
    if dy_side:
        dyb[:M] = rnd((M, co + 3 * dy_side), 399, dtype).to(dtype)
    dyb[:M, dy_side:dy_side + co] = k["dy"].permute(0, 2, 3, 1).reshape(M, co).to(dtype)
    return xa, xb, dyb[:M, dy_side:dy_side + co]


_WS_BUFS = {}


def run(ops, name, dtype, form, code=0, ws_slabs=SWEEP_SLABS, g0=None, dy_side=0, row0=0, inputs=None):
    """one launch into poisoned buffers; guards checked bit for bit -> the gradient (device, a copy)"""
    k = case(name, dtype)
    plan = launch_plan(name, dtype, form, code, ws_slabs, accumulate=g0 is not None)
    assert plan is not None, "the restated rules refuse this launch"
    xa, xb, dy = device_inputs(k, dtype, dy_side) if inputs is None else inputs
    co, slab = k["co"], slab_bytes(k)
    gbuf = torch.full((row0 + co + GUARD_ROWS, k["gw"][0].numel()), GRAD_FILL, device="cuda")
    own = torch.zeros(gbuf.shape[0], 1, dtype=torch.bool)
    own[row0:row0 + co] = True
    grad = gbuf[row0:row0 + co].view(k["gw"].shape)
    if g0 is not None:
        grad.copy_(g0)
    ws_bytes = int(ws_slabs * slab)
    wbuf = _WS_BUFS.get(ws_bytes + slab)
    if wbuf is None:
        _WS_BUFS.clear()
        wbuf = _WS_BUFS.setdefault(ws_bytes + slab, torch.empty(ws_bytes + slab, dtype=torch.uint8, device="cuda"))
    wbuf.fill_(WS_FILL)
    ops.conv_wgrad(xa, dy, grad, ksize=k["ks"], stride=k["stride"], pad=k["pad"], upsample=k["up"], x2=xb, accumulate=g0 is not None,
                   form=form, target=code, ws=wbuf[:ws_bytes])
    torch.cuda.synchronize()
    what = f"{name} {NAME[dtype]} form {form} code {code} ws {ws_slabs}"
    check_guard(gbuf, own, GRAD_FILL, f"{what}: gradient")
    used = 0 if plan["direct"] else plan["splits"] * slab
    assert ws_bytes + slab - used >= slab
    check_guard(wbuf[used:], torch.zeros(1, dtype=torch.bool), WS_FILL, f"{what}: workspace past {plan['splits']} slabs")
    return grad.clone()


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ the sweep
@gpu
@pytest.mark.parametrize("dtype", HALF, ids=["bf16", "f16"])
def test_every_form_and_split_target_the_tuner_may_freeze(ops, dtype):
    """all 12 (form, target) candidates of plan.autotune_wgrad on 8 images of 16 x 32, 192 -> 320 channels (M = 4096, up to 16 splits in a
    caller-owned workspace of 32 slabs) against fp64; candidates that share (rows per split, splits) are bit-identical -- across the two
    forms too, the claim of the wide form's header; a second launch gives the same bits; accumulate = 1 onto g0 is g0 + first exactly"""
    k = case("sweep", dtype)
    inputs = device_inputs(k, dtype)
    got = {}
    for key in SWEEP_TABLE:
        got[key] = run(ops, "sweep", dtype, *key, inputs=inputs)
        close(got[key], k["gw"], dtype, "sweep", f"form {key[0]} code {key[1]}")
    for a in SWEEP_TABLE:
        for b in SWEEP_TABLE:
            if a < b and SWEEP_TABLE[a] == SWEEP_TABLE[b]:
                assert torch.equal(got[a], got[b]), f"(form, code) {a} and {b}: same split ranges {SWEEP_TABLE[a]}, different bits"
    g0 = k["g0"].cuda()
    for key in ((1, 0), (2, 0)):
        assert torch.equal(run(ops, "sweep", dtype, *key, inputs=inputs), got[key]), f"{key}: a second launch differs"
        acc = run(ops, "sweep", dtype, *key, g0=g0, inputs=inputs)
        close(acc, k["g0"].double() + k["gw"], dtype, "sweep", f"form {key[0]} accumulate")
        assert torch.equal(acc, g0 + got[key]), f"{key}: accumulate is not g0 + the same reduced sum"


@gpu
def test_split_targets_in_f32(ops):
    """the register-staged form in f32 (v_mfma_f32_32x32x2_f32) at targets 0, 2 and 5 on 4 of the images: 7, 4 and 8 splits"""
    k = case("sweep4", F32)
    inputs = device_inputs(k, F32)
    got = {}
    for key in SWEEP_F32:
        got[key] = run(ops, "sweep4", F32, *key, inputs=inputs)
        close(got[key], k["gw"], F32, "sweep", f"form {key[0]} code {key[1]}")
    assert torch.equal(run(ops, "sweep4", F32, 1, 0, inputs=inputs), got[(1, 0)])
    g0 = k["g0"].cuda()
    acc = run(ops, "sweep4", F32, 1, 0, g0=g0, inputs=inputs)
    close(acc, k["g0"].double() + k["gw"], F32, "sweep", "accumulate")
    assert torch.equal(acc, g0 + got[(1, 0)])
    with pytest.raises(RuntimeError, match="wide form"):
        ops.conv_wgrad(inputs[0], inputs[2], torch.zeros(k["gw"].shape, device="cuda"), ksize=3, form=2)


@gpu
@pytest.mark.parametrize("dtype", HALF, ids=["bf16", "f16"])
@pytest.mark.parametrize("form", [1, 2], ids=["small", "wide"])
def test_workspace_cap(ops, form, dtype):
    """workspaces of 1.5, 2.5 and 5.5 slabs run 1, 2 and 5 splits (7 / 13 wanted): correct, and nothing past the last slab written; half a
    slab is refused and the poisoned gradient stays as it was"""
    k = case("sweep", dtype)
    inputs = device_inputs(k, dtype)
    for slabs in CAP_SLABS:
        close(run(ops, "sweep", dtype, form, 0, slabs, inputs=inputs), k["gw"], dtype, "cap", f"form {form} ws {slabs} slabs")
    gbuf = torch.full((320 + GUARD_ROWS, 9 * 192), GRAD_FILL, device="cuda")
    wbuf = torch.full((slab_bytes(k) // 2 + slab_bytes(k),), WS_FILL, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="workspace of .* bytes too small"):
        ops.conv_wgrad(inputs[0], inputs[2], gbuf[:320].view(320, 192, 3, 3), ksize=3, form=form, ws=wbuf[:slab_bytes(k) // 2])
    torch.cuda.synchronize()
    none = torch.zeros(1, dtype=torch.bool)
    check_guard(gbuf, none, GRAD_FILL, "refused launch: gradient")
    check_guard(wbuf, none, WS_FILL, "refused launch: workspace")


# ------------------------------------------------------------------------------------------------ maps
@gpu
@pytest.mark.parametrize("dtype", HALF, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", MAPS)
def test_non_square_power_of_two_maps(ops, name, dtype):
    """h_out != w_out in both forms: the wide form's shift-and-mask pixel split (lw / lh, wmask / hmask) and the register-staged form's
    divisions; the two forms plan the same split ranges here and must agree bit for bit; a map of one row (column) leaves the taps of the
    missing rows (columns) wholly outside the image: exactly 0.0"""
    k = case(name, dtype)
    inputs = device_inputs(k, dtype)
    g1, g2 = (run(ops, name, dtype, form, ws_slabs=4.0, inputs=inputs) for form in (1, 2))
    close(g1, k["gw"], dtype, "maps", f"{name} form 1")
    close(g2, k["gw"], dtype, "maps", f"{name} form 2")
    assert torch.equal(g1, g2), f"{name}: the two forms differ over the same split ranges"
    for g in (g1, g2):
        if k["h"] == 1:
            assert bool((g[:, :, 0] == 0.0).all()) and bool((g[:, :, 2] == 0.0).all())
        if k["w"] == 1:
            assert bool((g[:, :, :, 0] == 0.0).all()) and bool((g[:, :, :, 2] == 0.0).all())


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", GATHER)
def test_general_gather_on_odd_maps(ops, name, dtype):
    """the register-staged form's `/ w_out`, `* stride`, `>>= 1` gather on odd non-square maps: stride 1, stride 2, upsampled, pad = 0;
    the wide form refuses each of them"""
    k = case(name, dtype)
    inputs = device_inputs(k, dtype)
    got = run(ops, name, dtype, 1, ws_slabs=4.0, inputs=inputs)
    close(got, k["gw"], dtype, "gather", name)
    with pytest.raises(RuntimeError, match="wide form"):
        ops.conv_wgrad(inputs[0], inputs[2], torch.zeros(k["gw"].shape, device="cuda"), ksize=3, stride=k["stride"], pad=k["pad"],
                       upsample=k["up"], form=2)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", CONCAT)
def test_skip_concat_whose_channel_tile_straddles_the_sources(ops, name, dtype):
    """c0 = 72: the second 64-channel tile reads channels 64..71 from source 0 and 72..111 from source 1 (`from0 = ch < p.c0` inside a tile)"""
    k = case(name, dtype)
    close(run(ops, name, dtype, 1, ws_slabs=4.0), k["gw"], dtype, "concat", name)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", LINEARS)
def test_linears_as_slices_with_ragged_last_splits(ops, name, dtype):
    """7 (3) splits whose last has 131 (137) rows; dy is a column slice of a wider tensor with other data beside it (dy_ld > n_out), the
    gradient a row slice of a larger one; the two forms plan the same split ranges: same bits"""
    k = case(name, dtype)
    inputs = device_inputs(k, dtype, DY_SIDE)
    assert inputs[2].stride(0) == k["co"] + 3 * DY_SIDE and inputs[2].storage_offset() == DY_SIDE
    got = [run(ops, name, dtype, form, ws_slabs=8.0, row0=GRAD_ROW0, inputs=inputs) for form in forms_of(name, dtype)]
    for g in got:
        close(g, k["gw"], dtype, "linear", name)
    assert len(got) == (1 if dtype == F32 else 2) and all(torch.equal(got[0], g) for g in got)


# ------------------------------------------------------------------------------------------------ the one-split-per-XCD map on the device
XCD_RUNS = [("map8x32", 1), ("map8x32", 2), ("lin777", 1), ("lin777", 2)]


def xcd_digests(ops, dtype):
    """`ops`: anything with ops.conv_wgrad's signature"""
    return [digest(run(ops, name, dtype, form, ws_slabs=8.0, dy_side=DY_SIDE if name in LINEARS else 0)) for name, form in XCD_RUNS]


EXP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-result", "-DMVLDM_EXPERIMENTS"]


@gpu
def test_xcd_workgroup_map_changes_no_sum(ops, tmp_path):
    """MVLDM_WGRAD_XCD=1 changes which workgroup computes a (tile, split), never a sum.  The product library compiles no environment knob
    in (csrc/common.h knob_int, tests/test_abi.py), so wgrad.hip alone is compiled here with -DMVLDM_EXPERIMENTS into a library that
    resolves the rest from the product library (-Bsymbolic: its own wgrad_run, not the product's); one fresh child process -- the knob is read when that library loads -- runs the 8 x 32 map
    and the 777-row Linear through it in both forms and prints their SHA-256 digests, which must equal the parent's"""
    from mv_ldm_amd import _build, _lib as L
    exp = tmp_path / "libwgrad_exp.so"
    subprocess.run([_build._hipcc(), *EXP_FLAGS, "-shared", "-x", "hip", str(CSRC / "wgrad.hip"), "-x", "none", str(L.LIB_PATH),
                    "-Wl,-Bsymbolic", "-o", str(exp)], check=True, capture_output=True, text=True)
    env = dict(os.environ, MVLDM_WGRAD_XCD="1")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [str(Path(__file__).resolve()), "--xcd-child", str(exp)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("digest ")]
    assert [ln[1] for ln in lines] == [NAME[t] for t in HALF for _ in XCD_RUNS] and "xcd_map 1" in r.stdout
    want = [d for t in HALF for d in xcd_digests(ops, t)]
    assert [ln[2] for ln in lines] == want


def _xcd_child(exp_path):
    """the child of test_xcd_workgroup_map_changes_no_sum: the same launches through the experiment build of wgrad.hip"""
    import ctypes as C
    from mv_ldm_amd import _lib as L
    from mv_ldm_amd import ops as O
    assert os.environ.get("MVLDM_WGRAD_XCD") == "1"
    torch.zeros(1, device="cuda")
    exp = C.CDLL(str(exp_path))
    exp.mvldm_igemm_wgrad.restype, exp.mvldm_igemm_wgrad.argtypes = C.c_int, [C.POINTER(L.WgradDesc), C.c_void_p]

    class Through:          # ops.conv_wgrad's descriptor, run by the experiment library
        @staticmethod
        def conv_wgrad(x, dy, grad, *, ksize, stride, pad, upsample, x2, accumulate, form, target, ws):
            ho, wo = geom(dict(h=x.shape[1], w=x.shape[2], up=upsample, pad=pad, ks=ksize, stride=stride, n=x.shape[0], c0=0, c1=0))[:2]
            d = O.wgrad_desc(x, x2, dy, grad, ws, h_out=ho, w_out=wo, ksize=ksize, stride=stride, pad=pad, upsample=upsample, n_out=grad.shape[0],
                             accumulate=accumulate, form=form, target=target)
            rc = exp.mvldm_igemm_wgrad(C.byref(d), O.stream())
            assert rc == 0, rc
            return grad
    print(f"xcd_map {int(os.environ['MVLDM_WGRAD_XCD'])}")
    for dtype in HALF:
        for d in xcd_digests(Through, dtype):
            print(f"digest {NAME[dtype]} {d}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--xcd-child":
        torch.set_grad_enabled(False)
        _xcd_child(sys.argv[2])
