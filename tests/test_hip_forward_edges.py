"""GPU parity of the FORWARD kernels at their edges -- ragged tiles, every tile id a shape can keep, every head width of the attention
forward, the plan-only kernels (attention_merge, gather_rows), the norm instantiations -- with every destination a SLICE OF A LARGER
BUFFER, so that a store past the last row, past n_out into the n_pad padding or into column head_dim of the last head fails an assertion
instead of landing in allocator slack.  The forward counterpart of test_hip_backward_edges.py.

References: the same operation in plain torch on the CPU in fp64, from the SAME dtype-rounded inputs (`rnd` of test_hip_ops.py).
Bounds: `TOL` of test_hip_ops.py (relative L2, worst element over the reference's RMS), imported, not restated.  Every bounded value is
also handed to conftest.record_err; tests/golden/measured_errors_forward_edges.json is one MVLDM_TEST_REPORT run on an MI355X.

Guards: a destination of `rows x cols` lives in a buffer of `rows + GUARD_ROWS` rows of `cols + 16` (or 8) columns prefilled with 7.0
(-7.0 for fp32 / fp64 statistics).  GUARD_ROWS = 256 is the tallest tile of any kernel here, so an overrun of up to one tile stays
inside the allocation.  After the launch the guards must be bit-identical to the fill, then the interior is compared.

Only the two CPU tests (the launch rules, the helpers' self-test) are unmarked; every other test carries the gpu mark (a module-wide
pytestmark would skip those two on a machine without a GPU).

Where a case could not stay on the kernel first planned for it (the CPU test asserts each of these):
  * tile 15 computes whole images in groups of 48 / 64 / 192 rows: it refuses the 7 x 11 images of the base shape and any two-source 3x3,
    so its conv and phase cases use 5 images of 3 x 4 pixels (stride 2: 7 x 5 and the VAE's 8 x 6);
  * tiles 11 and 17 take 3x3 / stride-1 convs only, tile 17 one source only: a Linear that asks for them runs tile 7, so none does;
  * tile 10 (odd TN) and tile 18 have no GEGLU epilogue;
  * splitk = 3 at 128 channels is 2 splits on the lean 16-bit loop (splits own whole 64-channel blocks), 3 in f32.

Found by this module: attn_merge_kernel<float> missed the elementwise bound eps |ref| + eps 1e-3 (eps = 2^-22) by up to 78 x where the two
sides cancel (fp32 weights carry 2^-24 of each TERM); its weights and sum are fp64 now and the worst element is 0.25 x the bound.
"""
import functools
import math
import re
from collections import Counter
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from conftest import record_err
from test_hip_ops import TOL, G, rnd        # the project's bounds: (relative L2, worst element / RMS) per dtype

gpu = pytest.mark.gpu
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
HALF = [BF16, F16]
CSRC = Path(__file__).resolve().parent.parent / "mv_ldm_amd" / "csrc"
GUARD_ROWS = 256            # the tallest tile (BM of the 8-wave igemm tiles, 2 x BQ of the attention)
EPI_NONE, EPI_GEGLU = 0, 2


@pytest.fixture(scope="module")
def ops():
    from mv_ldm_amd import ops as O
    from mv_ldm_amd import _lib as L
    L.load()
    return O


def epc(dtype):
    return 4 if dtype == F32 else 8


# ------------------------------------------------------------------------------------------------ helpers
def close(got, ref, dtype, kind, what="", worst_factor=1.0):
    """test_hip_ops.close with the measured values recorded under `kind` (None: not recorded): relative L2 and worst element over the
    reference's RMS against TOL"""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    rl2, rmax = TOL[dtype]
    rms = ref.pow(2).mean().sqrt().clamp_min(1e-30)
    e2, emax = float((got - ref).norm() / ref.norm().clamp_min(1e-30)), float((got - ref).abs().max() / rms)
    if kind is not None:
        record_err(f"{kind}/rel_l2/{NAME[dtype]}", e2)
        record_err(f"{kind}/worst_over_rms/{NAME[dtype]}", emax)
    print(f"close {kind} {what}: rel-L2 {e2:.3e} (tol {rl2:.1e}), worst/rms {emax:.3e} (tol {rmax * worst_factor:.1e})")
    assert e2 <= rl2 and emax <= rmax * worst_factor, \
        f"{kind} {what}: rel-L2 {e2:.3e} (tol {rl2}), worst element / rms {emax:.3e} (tol {rmax * worst_factor})"


def check_guard(buf, owned, fill, what=""):
    """every element of `buf` outside the boolean mask `owned` (broadcastable to buf's shape) is bit-identical to `fill`"""
    g = buf[~owned.to(buf.device).expand(buf.shape)]
    if not torch.equal(g, torch.full_like(g, fill)):
        bad = (buf != fill) & ~owned.to(buf.device).expand(buf.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} guard elements written, first at {bad.nonzero()[0].tolist()} of {tuple(buf.shape)}")


def block(shape, rows, cols):
    """mask of the leading rows x cols block of a 2-D buffer"""
    m = torch.zeros(shape, dtype=torch.bool)
    m[:rows, :cols] = True
    return m


def guarded(rows, cols, dtype, fill=7.0, extra_cols=16):
    """a device buffer [rows + GUARD_ROWS, cols + extra_cols] of `fill`; the destination is its leading rows"""
    return torch.full((rows + GUARD_ROWS, cols + extra_cols), fill, dtype=dtype, device="cuda")


def test_the_checks_can_fail():
    """CPU: check_guard raises on one flipped guard element (a guard row, a guard column), close on one interior element off by 1 x RMS"""
    for dtype, fill in ((BF16, 7.0), (F32, -7.0)):
        buf = torch.full((5 + GUARD_ROWS, 24), fill, dtype=dtype)
        own = block(buf.shape, 5, 8)
        buf[:5, :8] = 1.0
        check_guard(buf, own, fill)
        for r, c in ((5, 0), (5 + GUARD_ROWS - 1, 23), (4, 8), (0, 23)):       # first / last guard row, first / last guard column
            bad = buf.clone()
            bad[r, c] = fill + (0.0625 if dtype == BF16 else 1e-6)              # one ulp-sized flip
            with pytest.raises(AssertionError, match="guard elements written"):
                check_guard(bad, own, fill)
        neg = buf.clone()
        neg[5, 3] = -fill
        with pytest.raises(AssertionError):
            check_guard(neg, own, fill)
    for dtype in DTYPES:
        ref = rnd((33, 40), 1, dtype).double()
        close(ref.clone(), ref, dtype, None, "selftest")
        off = ref.clone()
        off[17, 23] += ref.pow(2).mean().sqrt()
        with pytest.raises(AssertionError, match="worst element"):
            close(off, ref, dtype, None, "selftest")


# ------------------------------------------------------------------------------------------------ launch rules, restated
# The cases below are named for the kernel, tile or instantiation they run.  The host-side rules that decide it are restated here, and the
# source is required to still state them: a later change of a rule fails the CPU test instead of silently moving a case off its kernel.
RULES_IN_SOURCE = [
    ("igemm.hip", "if (tile >= 6 && !p.use_bl) tile = 2;"),
    ("igemm.hip", "if (deep_tile(tile) && d.upsample) tile = 2;"),
    ("igemm.hip", "const int cbs = p.k_tiles / p.taps; const int per = cdiv(cbs, std::min(splitk, cbs)); p.k_tiles_per_split = per * p.taps; p.splitk = cdiv(cbs, per);"),
    ("igemm.hip", "p.k_tiles_per_split = cdiv(p.k_tiles, splitk); p.splitk = cdiv(p.k_tiles, p.k_tiles_per_split);"),
    ("igemm.hip", "p.use_bl = d.act_dtype != MVLDM_F32 && d.k_order == 1 && !t_force_sync && !kEnvSync &&"),
    ("igemm.hip", "p.stage_epi = d.act_dtype != MVLDM_F32 && !kEnvNoStage && (p.splitk > 1 || (!p.dst_f32 && p.n_dst % 8 == 0 && p.dst_ld % 8 == 0));"),
    ("igemm.hip", "if (tile >= 9 && tile <= 10 && (!p.stage_epi || (tile == 10 && d.epilogue == MVLDM_EPI_GEGLU))) tile = 7;"),
    ("igemm.hip", "if (tile == 11 && !(p.use_bl && p.stage_epi && p.splitk == 1 && d.ksize == 3 && d.stride == 1 && d.pad == 1 && !d.upsample && "
                  "d.h_out == d.h_in && d.w_out == d.w_in && halo_rows_for(d.w_in) <= 384 && halo_smem(d.w_in) <= 160 * 1024)) tile = 7;"),
    ("igemm.hip", "if (tile == 17 && !(p.use_bl && p.stage_epi && p.splitk == 1 && d.ksize == 3 && d.stride == 1 && d.pad == 1 && !d.upsample && d.c1 == 0 && "
                  "d.h_out == d.h_in && d.w_out == d.w_in && d.epilogue != MVLDM_EPI_GEGLU && halow_smem(d.w_in) <= 160 * 1024)) tile = 7;"),
    ("igemm.hip", "if (tile != 7 && tile != 10) tile = 2;"),
    ("igemm.hip", "if (p.use_bl && d.upsample == 1 && tile != 7) tile = 2;"),
    ("igemm.hip", "if (!p.dst_f32 && p.n_dst % 8 == 0 && p.dst_ld % 8 == 0 && ((uintptr_t)p.ws % 16) == 0 &&"),
    ("igemm.hip", "if (req == 15) return skinny_run(d, s);"),
    ("igemm.hip", "return req == 12 ? linear_pp_run(d, s) : req == 13 ? linear_pw_run(d, s) : req == 14 ? linear_ws_run(d, s) : linear_rs_run(d, s);"),
    ("igemm_common.h", "inline bool deep_tile(int tile) { return tile == 18; }"),
    ("igemm_common.h", "inline int halo_rows_for(int w_in) { return (256 + 2 * (w_in + 1) + 7) / 8 * 8; }"),
    ("igemm_common.h", "inline int halo_smem(int w_in) { return 2 * halo_rows_for(w_in) * 128 + 3 * 128 * 128 + 128 + 1024; }"),
    ("igemm_common.h", "inline int halow_smem(int w_in) { return 2 * halo_rows_for(w_in) * 128 + 2 * 320 * 128 + 128 + 1024; }"),
    ("igemm_common.h", "constexpr TileCfg kTiles[] = {{0, 0, 0}, {128, 128, 256}, {128, 64, 256}, {64, 128, 256}, {64, 64, 128}, {32, 64, 64},"),
    ("linear_pp.hip", "d.c0 + d.c1 < 320 || d.k_pad != d.c0 + d.c1 || d.n_out % 8 || n_dst % 8 || dst_ld % 8 || dst_ld < n_dst) return false;"),
    ("linear_pw.hip", "d.c0 + d.c1 < 320 || d.k_pad != d.c0 + d.c1 || d.n_out % 8 || n_dst % 8 || dst_ld % 8 || dst_ld < n_dst) return false;"),
    ("linear_ws.hip", "if (d.src1 || d.c1 || d.c0 != WS_K || d.k_pad != WS_K || d.n_pad % WS_BN || d.n_out != d.n_pad) return false;"),
    ("linear_ws.hip", "if (n_dst % 8 || dst_ld % 8 || dst_ld < n_dst) return false;"),
    ("linear_ws.hip", "constexpr int WS_K = 320, WS_KS = WS_K / 16, WS_NW = 10, WS_BN = 320, WS_ROWS = 64;"),
    ("linear_rs.hip", "k < 256 || k % 128 || d.k_pad != k || d.n_out % 8 || n_dst % 8 || dst_ld % 8 || dst_ld < n_dst) return false;"),
    ("skinny.hip", "if (dst_ld % 4 || dst_ld < n_dst) return false;"),
    ("skinny.hip", "if (d.epilogue == MVLDM_EPI_GEGLU && (d.n_out % 64 || d.row_bias || d.n_out != d.n_pad)) return false;"),
    ("skinny.hip", "if (d.residual && d.upsample >= 2) return false;"),
    ("skinny.hip", "const int rows = c.mt * 16; if (hw_out > rows || rows % hw_out) return false; const int G = rows / hw_out; "
                   "if (G * hw_in > rows * c.sm) return false;"),
    ("skinny.hip", "if (d.c1 > 0) { const bool sk2 = c.sc > 0 && c.taps == 1 &&"),
    ("skinny.hip", "{9, 9, 1, 3, 1, 10, 1, 0}, {9, 9, 1, 4, 1, 10, 1, 0},"),
    ("skinny.hip", "{9, 9, 1, 3, 1, 5, 4, 0}, {4, 8, 2, 3, 1, 5, 1, 0}, {4, 8, 2, 4, 1, 5, 1, 0},"),
    ("skinny.hip", "{9, 9, 1, 12, 1, 3, 1, 0}, {4, 8, 2, 12, 1, 3, 1, 0},"),
    ("attention.hip", "constexpr int BQ = 128, BKV = 64;"),
    ("attention.hip", "const int dp = (head_dim + 15) / 16 * 16;"),
    ("attention.hip", "if (p.d % 8 == 0 && p.d < DP) return launch_attn_q<T, DP, true>(p, n_seg, max_q_len, s);"),
    ("attention.hip", "if (nch <= 64) hipLaunchKernelGGL((attention_wide_kernel<T, 1>), grid, dim3(256), 0, s, p); "
                      "else if (nch <= 128) hipLaunchKernelGGL((attention_wide_kernel<T, 2>), grid, dim3(256), 0, s, p); "
                      "else if (nch <= 256) hipLaunchKernelGGL((attention_wide_kernel<T, 4>), grid, dim3(256), 0, s, p);"),
    ("attention.hip", "if (head_dim == 512 && !valu && !p.lse) return launch_attn_dsplit<T, 128>(p, n_seg, max_q_len, s);"),
    ("attention.hip", "if (head_dim > 160) {"),
    ("attention.hip", "p.remap = max_q_len <= 2048;"),
    ("attention.hip", "MVLDM_REQUIRE(!lse || head_dim <= 160,"),
    ("norm.hip", "if (!((cpg >= epc && true) || (epc % cpg == 0 && epc / cpg == 2))) return 0;"),
    ("norm.hip", "const int base = cpg / gcd(cpg, epc) * epc;"),
    ("norm.hip", "if (c % span || span / cpg > 64) continue;"),
    ("norm.hip", "const int l = cps / gcd(cps, 64) * 64; if (l > 1024) continue;"),
    ("norm.hip", "int n = std::max(l, std::min(1024, x_nthr) / l * l);"),
    ("norm.hip", "while (n > l && (long long)(n - l) >= chunks) n -= l; const int k = (int)((chunks + n - 1) / n); if (k > 16) continue;"),
    ("norm.hip", "const bool enough = (long long)n_img * (c / span) >= 512;"),
    ("norm.hip", "if (!force_wide && !enough) break;"),
    ("norm.hip", "if (f_kt <= 2) MVLDM_GN_FUSED(2); else if (f_kt <= 4) MVLDM_GN_FUSED(4); else if (f_kt <= 8) MVLDM_GN_FUSED(8); "
                 "else if (f_kt <= 12) MVLDM_GN_FUSED(12); else MVLDM_GN_FUSED(16);"),
    ("norm.hip", "int nchunk = std::min(MVLDM_GN_MAX_CHUNKS, std::max(1, std::min(hw / 8, (1024 + n_img - 1) / n_img)));"),
    ("norm.hip", "if (rows >= 1024) { for (int cpl = 5; cpl >= 3; --cpl) { if (ncc % cpl) continue; const int lpr = ncc / cpl; "
                 "if (lpr != 8 && lpr != 16 && lpr != 32) continue;"),
    ("norm.hip", "else if (ncc <= 512) hipLaunchKernelGGL((layernorm_kernel<T, 8>)"),
    ("norm.hip", "else hipLaunchKernelGGL((layernorm_kernel<T, 16>)"),
    ("norm.hip", "MVLDM_REQUIRE(ncc <= 64 * 16,"),
]


def _squeeze(text):
    return re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", text))


def cdiv(a, b):
    return (a + b - 1) // b


def halo_rows_for(w_in):
    return (256 + 2 * (w_in + 1) + 7) // 8 * 8


def out_hw(c):
    """ops.conv_out_hw for a case"""
    h, w, ks, st, up = c["h"], c["w"], c["ksize"], c.get("stride", 1), c.get("upsample", 0)
    pad = c.get("pad", ks // 2)
    if up >= 2:
        return h, w
    if ks == 3 and st == 2 and pad == 0:
        return (h + 1 - 3) // 2 + 1, (w + 1 - 3) // 2 + 1
    return ((2 if up else 1) * h + 2 * pad - ks) // st + 1, ((2 if up else 1) * w + 2 * pad - ks) // st + 1


SK_ROWS = {9: ((48, 1), (64, 1), (48, 4), (192, 1)), 4: ((48, 1), (64, 1), (192, 1))}       # skinny.hip kSkCfgs: (16 x mt rows, source-row multiple sm)


def skinny_fits(c):
    """skinny.hip sk_cfg_fits over the table: does ANY configuration compute the case (whole images per workgroup)?"""
    taps = c["ksize"] ** 2
    if taps == 1:
        return True                      # Linear geometry: every row is an image of one pixel
    if c["c1"]:
        return False                     # two sources: the 1x1 / Linear configurations only
    ho, wo = out_hw(c)
    return any(ho * wo <= rows and rows % (ho * wo) == 0 and rows // (ho * wo) * c["h"] * c["w"] <= rows * sm for rows, sm in SK_ROWS[taps])


def igemm_resolve(c):
    """igemm.hip igemm_run / fill_params (+ the *_applicable rules of the Linear tiles and tile 15) for an explicitly requested tile ->
    (the tile that runs or None when the launch is refused, effective split-K, stage_epi, reduce kernel: None / 'vec' / 'scalar')"""
    dtype, req, k, taps = c["dtype"], c["tile"], c["c0"] + c["c1"], c["ksize"] ** 2
    half = dtype != F32
    bk = 64 if half else 32
    k_pad = cdiv(taps * k, bk) * bk
    k_order = int(k % bk == 0 and (c["c1"] == 0 or c["c0"] % bk == 0))
    n_out, n_pad = c["n_out"], cdiv(c["n_out"], 64) * 64
    geglu = c["epi"] == EPI_GEGLU
    n_dst = n_out // 2 if geglu else n_out
    dst_ld, dst_f32, up, splitk = c["dst_ld"], c.get("dst_f32", False) or not half, c.get("upsample", 0), c.get("splitk", 1)
    res = c.get("residual", False)
    if req in (12, 13, 14, 19, 15):
        lin = c["ksize"] == 1 and c.get("stride", 1) == 1 and up == 0 and splitk <= 1 and not (geglu and res)
        common = half and not dst_f32 and k_order == 1 and c["c0"] % 64 == 0 and c["c1"] % 64 == 0 and n_out % 8 == 0 and n_dst % 8 == 0 and \
            dst_ld % 8 == 0 and dst_ld >= n_dst and (not geglu or n_out % 64 == 0)
        ok = {12: lin and common and k >= 320 and k_pad == k,
              13: lin and common and k >= 320 and k_pad == k,
              14: lin and common and c["c1"] == 0 and k == 320 and n_pad % 320 == 0 and n_out == n_pad,
              19: lin and common and k >= 256 and k % 128 == 0,
              15: half and k_order == 1 and c["c0"] % 64 == 0 and c["c1"] % 64 == 0 and n_out % 4 == 0 and dst_ld % 4 == 0 and dst_ld >= n_dst and
              up != 1 and (c["ksize"] in (1, 3) and up == 0 or c["ksize"] == 2 and up >= 2) and not (geglu and n_out != n_pad) and
              not (res and up >= 2) and skinny_fits(c)}[req]
        return (req if ok else None), 1, None, None
    tile = req
    k_tiles = k_pad // bk
    splitk = max(1, min(splitk, k_tiles))
    use_bl = half and k_order == 1
    if tile >= 6 and not use_bl:
        tile = 2
    if tile == 18 and up:
        tile = 2
    if use_bl:
        cbs = k_tiles // taps
        eff = cdiv(cbs, cdiv(cbs, min(splitk, cbs)))
    else:
        eff = cdiv(k_tiles, cdiv(k_tiles, splitk))
    stage_epi = half and (eff > 1 or (not dst_f32 and n_dst % 8 == 0 and dst_ld % 8 == 0))
    if tile in (9, 10) and (not stage_epi or (tile == 10 and geglu)):
        tile = 7
    same = c["ksize"] == 3 and c.get("stride", 1) == 1 and c.get("pad", 1) == 1 and not up
    w_in = c.get("w", 1)
    if tile == 11 and not (use_bl and stage_epi and eff == 1 and same and halo_rows_for(w_in) <= 384 and
                           2 * halo_rows_for(w_in) * 128 + 3 * 128 * 128 + 128 + 1024 <= 160 * 1024):
        tile = 7
    if tile == 17 and not (use_bl and stage_epi and eff == 1 and same and c["c1"] == 0 and not geglu and
                           2 * halo_rows_for(w_in) * 128 + 2 * 320 * 128 + 128 + 1024 <= 160 * 1024):
        tile = 7
    if up >= 2:
        if not (use_bl and stage_epi):
            return None, eff, stage_epi, None
        if tile not in (7, 10):
            tile = 2
    if use_bl and up == 1 and tile != 7:
        tile = 2
    if tile == 18 and geglu:
        return None, eff, stage_epi, None          # igemm_xl.hip: tile 18 does not take the GEGLU epilogue
    reduce = None if eff == 1 else "vec" if half and not dst_f32 and n_dst % 8 == 0 and dst_ld % 8 == 0 else "scalar"
    return tile, eff, stage_epi, reduce


def attn_kernel(d, dtype, max_q_len=0, lse=False):
    """attention.hip attention_run -> the instantiation's name"""
    if d > 160:
        if dtype != F32 and d == 512 and not lse:
            return "dsplit<128>"
        nch = d // epc(dtype)
        assert nch <= 256
        return f"wide<{NAME[dtype]},{1 if nch <= 64 else 2 if nch <= 128 else 4}>"
    dp = (d + 15) // 16 * 16
    ones = dtype != F32 and d % 8 == 0 and d < dp
    return f"mfma<DP={dp},ONES={int(ones)},remap={int(max_q_len <= 2048)}>"


def gn_fused_plan(hw, c, groups, dtype, n_img):
    """norm.hip gn_fused_plan -> (span, nthr, kt); span 0: the two-launch path"""
    e, cpg = epc(dtype), c // groups
    if not (cpg >= e or (e % cpg == 0 and e // cpg == 2)):
        return 0, 0, 0
    base = cpg // math.gcd(cpg, e) * e
    if base > c or c % base:
        return 0, 0, 0
    best, m = (0, 0, 0), 0
    while base * (m + 1) <= c:
        m += 1
        span = base * m
        if c % span or span // cpg > 64:
            continue
        cps = span // e
        l = cps // math.gcd(cps, 64) * 64
        if l > 1024:
            continue
        n, chunks = max(l, 1024 // l * l), hw * cps
        while n > l and n - l >= chunks:
            n -= l
        k = cdiv(chunks, n)
        if k > 16:
            continue
        enough = n_img * (c // span) >= 512
        if best[0] == 0 or enough:
            best = (span, n, k)
        if not enough:
            break
    return best


def gn_kernel(n, c0, c1, h, w, groups, dtype):
    span, nthr, kt = gn_fused_plan(h * w, c0 + c1, groups, dtype, n)
    if span == 0:
        return "two_launch"
    return f"fused<KT={2 if kt <= 2 else 4 if kt <= 4 else 8 if kt <= 8 else 12 if kt <= 12 else 16}>"


def gn_slabs(n_img, hw):
    """norm.hip groupnorm_run, two-launch path -> (row slabs per image, rows per slab)"""
    nchunk = min(32, max(1, min(hw // 8, (1024 + n_img - 1) // n_img)))
    rpc = cdiv(hw, nchunk)
    return cdiv(hw, rpc), rpc


def ln_kernel(rows, c, dtype):
    """norm.hip layernorm_run"""
    ncc = c // epc(dtype)
    assert c % epc(dtype) == 0 and ncc <= 64 * 16
    if dtype != F32 and rows >= 1024:
        for cpl in (5, 4, 3):
            if ncc % cpl == 0 and ncc // cpl in (8, 16, 32):
                return f"rows<LPR={ncc // cpl},CPL={cpl}>"
    return f"wave<MAXCH={1 if ncc <= 64 else 2 if ncc <= 128 else 4 if ncc <= 256 else 8 if ncc <= 512 else 16}>"


# ------------------------------------------------------------------------------------------------ cases: igemm, Linear, skinny
CONV = dict(n=3, h=7, w=11)           # M = 231: ragged against every BM in {32, 64, 128, 192, 256}
SK_CONV = dict(n=5, h=3, w=4)         # tile 15 takes whole images of 48 / 64 / 192 rows per workgroup: 5 images of 12 pixels, groups of 4 are ragged
ROWS = (231, 1)


def _case(name, dtype, tile, want, **kw):
    c = dict(name=f"{name}-t{tile}-{NAME[dtype]}", dtype=dtype, tile=tile, want=want, ksize=3, c0=128, c1=0, n_out=200, epi=EPI_NONE, residual=True,
             splitk=1, **CONV)
    c.update(kw)
    n_dst = c["n_out"] // 2 if c["epi"] == EPI_GEGLU else c["n_out"]
    c.setdefault("dst_ld", n_dst + 16)
    return c


def _igemm_cases():
    out = []
    for dtype in DTYPES:
        tiles = (1, 2, 3, 4, 5) if dtype == F32 else (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 18, 11, 17, 12, 13, 14, 19, 15)
        for t in tiles:
            # 3x3 convs: one source (every tile that takes a conv), two sources where they are allowed
            if t not in (12, 13, 14, 19):
                out.append(_case("conv3", dtype, t, t, n_out=312 if t in (10, 17) else 200, **(SK_CONV if t == 15 else {})))
                if t in (2, 7, 11):
                    out.append(_case("conv3_2src", dtype, t, t, c0=64, c1=64))
            # Linears: 231 rows and 1 row
            for rows in ROWS:
                if t in (11, 17):                          # the halo tiles take 3x3 convs only: a Linear that asks for them runs tile 7
                    continue
                lin = dict(ksize=1, n=rows, h=1, w=1, c0=384 if t == 19 else 320)
                out.append(_case(f"lin{rows}", dtype, t, t, n_out=320 if t == 14 else 312 if t == 10 else 200, **lin))
                if t not in (10, 18):                      # (10: odd TN cannot pair GEGLU columns, 18 refuses the epilogue)
                    out.append(_case(f"geglu{rows}", dtype, t, t, n_out=640, epi=EPI_GEGLU, residual=False, **lin))
    # split-K = 3 through both reduce kernels (the lean loop splits whole channel blocks: 2 of them at 128 channels)
    for dtype in DTYPES:
        for t in (2,) if dtype == F32 else (2, 7):
            if dtype != F32:
                out.append(_case("splitk_vec", dtype, t, t, splitk=3, reduce="vec"))
                out.append(_case("splitk_scalar12", dtype, t, t, splitk=3, n_out=12, dst_ld=20, reduce="scalar"))
            out.append(_case("splitk_scalar_f32dst4", dtype, t, t, splitk=3, n_out=4, dst_ld=8, dst_f32=True, residual=False, reduce="scalar"))
    # nearest-2x gather form and the stride-2 forms, odd sizes
    for dtype in DTYPES:
        for t in (2,) if dtype == F32 else (2, 7):
            out.append(_case("up1", dtype, t, t, upsample=1))
            out.append(_case("stride2", dtype, t, t, stride=2))
            out.append(_case("stride2_vae", dtype, t, t, stride=2, pad=0, h=8, w=6))
        if dtype != F32:
            out.append(_case("stride2", dtype, 15, 15, stride=2, h=7, w=5))
            out.append(_case("stride2_vae", dtype, 15, 15, stride=2, pad=0, h=8, w=6))
    return out


IGEMM_CASES = _igemm_cases()
# 2x2 phase convs (16-bit only): tile -> the tile that runs; tile 15 has no split-K
PHASE_CASES = [dict(name=f"phase-t{t}-sk{sk}-{NAME[dtype]}", dtype=dtype, tile=t, want=t, ksize=2, c0=128, c1=0, n_out=312 if t == 10 else 200,
                    dst_ld=(312 if t == 10 else 200) + 16, epi=EPI_NONE, splitk=sk, pad=0, upsample=2,
                    reduce="vec" if sk == 2 else None, **(SK_CONV if t == 15 else CONV))
               for dtype in HALF for t in (2, 7, 10, 15) for sk in (1, 2) if not (t == 15 and sk == 2)]

# ------------------------------------------------------------------------------------------------ cases: attention
DP_WIDTHS = {BF16: [8, 24, 32, 40, 56, 64, 72, 88, 96, 104, 112, 120, 128, 136, 144, 152], F32: [4, 20, 96, 144]}
DP_WIDTHS[F16] = DP_WIDTHS[BF16]
DP_SEGS = ((129, 65), (63, 191), (1, 1))        # one row past BQ, +-1 around BKV, 1 x 1; q_len != kv_len both ways
GUARD_WIDTHS = [(BF16, 40), (BF16, 64), (BF16, 88), (BF16, 160), (F16, 40), (F16, 64), (F16, 88), (F16, 160), (F32, 20)]
SCALE_WIDTHS = [(t, d) for t in DTYPES for d in (40, 64)]
WIDE = [(BF16, 320, "wide<bf16,1>"), (F16, 320, "wide<f16,1>"), (F32, 200, "wide<f32,1>"), (F32, 320, "wide<f32,2>"), (F32, 768, "wide<f32,4>"),
        (BF16, 1032, "wide<bf16,4>")]
WIDE_SEGS = ((70, 33), (5, 1))
NOREMAP_SEGS = ((2100, 70), (3, 130))

# ------------------------------------------------------------------------------------------------ cases: norms
GN_CASES = {  # name: n, c0, c1, h, w, groups per dtype class (16-bit, f32), named for the kernel the mirror of gn_fused_plan gives
    "kt2": {2: (2, 512, 0, 5, 7, 2), 4: (2, 512, 0, 5, 5, 2)}, "kt4": {2: (2, 512, 0, 5, 23, 2), 4: (2, 512, 0, 7, 9, 2)},
    "kt8": {2: (2, 512, 0, 15, 17, 2), 4: (2, 512, 0, 11, 11, 2)}, "kt12": {2: (2, 512, 0, 19, 19, 2), 4: (2, 512, 0, 13, 13, 2)},
    "kt16": {2: (2, 512, 0, 21, 23, 2), 4: (2, 512, 0, 15, 17, 2)},
    "two_launch_short_slab": {2: (2, 512, 0, 23, 23, 2), 4: (2, 512, 0, 23, 23, 2)},
    "cpg4": {2: (3, 128, 0, 5, 7, 32), 4: (3, 128, 0, 5, 7, 32)}, "cpg1": {2: (3, 32, 0, 5, 7, 32), 4: (3, 32, 0, 5, 7, 32)},
    "concat_straddle": {2: (2, 320, 640, 5, 7, 32), 4: (2, 320, 640, 5, 7, 32)}}
GN_WANT = {"kt2": "fused<KT=2>", "kt4": "fused<KT=4>", "kt8": "fused<KT=8>", "kt12": "fused<KT=12>", "kt16": "fused<KT=16>",
           "two_launch_short_slab": "two_launch", "cpg4": "fused<KT=2>", "cpg1": "two_launch", "concat_straddle": "fused<KT=2>"}


def gn_shape(name, dtype):
    return GN_CASES[name][2 if dtype != F32 else 4]


LN_CASES = [(5, 4104, BF16), (5, 4104, F16), (5, 2052, F32)] + [(r, 320, t) for r in (1, 1023, 1024, 1027) for t in DTYPES]


def test_cases_reach_the_kernels_they_are_named_for(capsys):
    """CPU only: the restated launch rules put every case of this module on the kernel, tile or instantiation it is named for, and the
    source still states those rules.  Prints the number of cases per kernel (pytest -s)."""
    for name, text in RULES_IN_SOURCE:
        assert _squeeze(text) in _squeeze((CSRC / name).read_text()), f"{name} no longer states: {text}"
    count = Counter()
    # ---- igemm
    for c in IGEMM_CASES + PHASE_CASES:
        tile, eff, stage_epi, reduce = igemm_resolve(c)
        assert tile == c["want"], (c["name"], "resolves to tile", tile, "not", c["want"])
        assert reduce == c.get("reduce"), (c["name"], reduce)
        if c.get("splitk", 1) > 1:
            assert eff > 1, c["name"]
        count[f"igemm tile {tile}" + (f" + {reduce} reduce" if reduce else "") + (" phase" if c.get("upsample", 0) >= 2 or c["ksize"] == 2 else "")] += 1
    ran = {igemm_resolve(c)[0] for c in IGEMM_CASES}
    assert ran == {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 18, 11, 17, 12, 13, 14, 19, 15}
    assert {c["want"] for c in PHASE_CASES} == {2, 7, 10, 15}
    m = CONV["n"] * CONV["h"] * CONV["w"]
    assert m == 231 and all(m % bm for bm in (32, 64, 128, 192, 256)) and 200 % 64 == 8 and cdiv(312, 64) * 64 == 320
    # what the rules would do to a request they cannot keep (none of these is a case: the cases above keep their tiles)
    base = _case("x", BF16, 11, 7, splitk=2)
    assert igemm_resolve(base)[0] == 7 and igemm_resolve(dict(base, tile=17))[0] == 7                       # halo tiles: one K pass only
    assert igemm_resolve(_case("x", BF16, 9, 7, n_out=12, dst_ld=20))[0] == 7                                # 9 / 10 without stage_epi
    assert igemm_resolve(_case("x", BF16, 10, 7, ksize=1, c0=320, n_out=640, epi=EPI_GEGLU))[0] == 7         # tile 10 with GEGLU
    assert igemm_resolve(_case("x", F32, 7, 2))[0] == 2 and igemm_resolve(_case("x", BF16, 7, 2, c0=40))[0] == 2      # >= 6 without the lean loop
    assert igemm_resolve(_case("x", BF16, 18, 2, upsample=1))[0] == 2 and igemm_resolve(_case("x", BF16, 3, 2, upsample=1))[0] == 2
    assert igemm_resolve(_case("x", BF16, 17, 7, c0=64, c1=64))[0] == 7 and igemm_resolve(_case("x", BF16, 11, 7, stride=2))[0] == 7
    assert igemm_resolve(dict(PHASE_CASES[0], tile=9))[0] == 2 and igemm_resolve(dict(PHASE_CASES[0], tile=18, upsample=2))[0] == 2
    for t in (12, 13, 14, 19):                                                                             # dst_ld terms of the Linear tiles
        ok = _case("x", BF16, t, t, ksize=1, c0=384 if t == 19 else 320, n_out=320)
        assert igemm_resolve(ok)[0] == t and igemm_resolve(dict(ok, dst_ld=324))[0] is None and igemm_resolve(dict(ok, dst_ld=312))[0] is None
    assert igemm_resolve(_case("x", BF16, 15, None))[0] is None and 77 > 64 and 192 % 77          # tile 15 cannot take the 7 x 11 images: SK_CONV
    assert igemm_resolve(_case("x", BF16, 15, None, c0=64, c1=64, **SK_CONV))[0] is None            # ... nor a two-source 3x3
    ok = _case("x", BF16, 15, 15, **SK_CONV)
    assert igemm_resolve(dict(ok, dst_ld=204))[0] == 15 and igemm_resolve(dict(ok, dst_ld=202))[0] is None
    # ---- attention
    for dtype in DTYPES:
        for d in DP_WIDTHS[dtype]:
            count["attention " + attn_kernel(d, dtype, 129)] += 1
    assert {(d + 15) // 16 * 16 for d in DP_WIDTHS[BF16]} == set(range(16, 161, 16))
    assert [d for d in DP_WIDTHS[BF16] if "ONES=1" in attn_kernel(d, BF16)] == [8, 24, 40, 56, 72, 88, 104, 120, 136, 152]
    assert all("ONES=0" in attn_kernel(d, F32) for d in DP_WIDTHS[F32]) and {(d + 15) // 16 * 16 for d in DP_WIDTHS[F32]} == {16, 32, 96, 144}
    for dtype, d in GUARD_WIDTHS:
        count["attention guarded " + attn_kernel(d, dtype, 329)] += 1
    assert [attn_kernel(d, t) for t, d in GUARD_WIDTHS[:4]] == ["mfma<DP=48,ONES=1,remap=1>", "mfma<DP=64,ONES=0,remap=1>", "mfma<DP=96,ONES=1,remap=1>",
                                                               "mfma<DP=160,ONES=0,remap=1>"]
    for dtype, d, want in WIDE:
        assert attn_kernel(d, dtype) == want, (d, dtype)
        count["attention " + want] += 2            # plain and guarded
    assert attn_kernel(512, BF16) == "dsplit<128>" and attn_kernel(512, BF16, lse=True) == "wide<bf16,1>" and attn_kernel(512, F32) == "wide<f32,2>"
    for dtype in (BF16, F32):
        assert attn_kernel(16, dtype, 2100) == "mfma<DP=16,ONES=0,remap=0>" and attn_kernel(16, dtype, 2048).endswith("remap=1>")
        count["attention " + attn_kernel(16, dtype, 2100)] += 1
    assert max(s[0] for s in DP_SEGS) == 129 and {s[1] for s in DP_SEGS} >= {65, 191} and 191 == 3 * 64 - 1      # BQ = 128, BKV = 64
    # ---- GroupNorm
    for name in GN_CASES:
        for dtype in DTYPES:
            n, c0, c1, h, w, groups = gn_shape(name, dtype)
            assert gn_kernel(n, c0, c1, h, w, groups, dtype) == GN_WANT[name], (name, NAME[dtype], gn_fused_plan(h * w, c0 + c1, groups, dtype, n))
            assert h * w <= 1024
            count["groupnorm " + GN_WANT[name]] += 2          # plain and SiLU
    assert gn_fused_plan(21 * 23, 512, 2, BF16, 2) == (256, 1024, 16) and gn_fused_plan(15 * 17, 512, 2, F32, 2) == (256, 1024, 16)      # span, nthr, kt
    assert gn_fused_plan(35, 128, 32, BF16, 3) == (8, 64, 1) and gn_fused_plan(35, 960, 32, F32, 2) == (60, 960, 1)
    assert gn_fused_plan(32 * 32, 320, 32, BF16, 128) == (80, 960, 11) and gn_fused_plan(32 * 32, 320, 32, BF16, 9) == (40, 960, 6)     # >= 512 workgroups: a wider span
    n, c0, c1, h, w, groups = gn_shape("two_launch_short_slab", BF16)
    assert gn_slabs(n, h * w) == (32, 17) and h * w - 31 * 17 == 2                  # the last slab has 2 of 17 rows
    n, c0, c1, h, w, groups = gn_shape("cpg1", BF16)
    assert c0 // groups == 1 and gn_slabs(n, h * w) == (4, 9) and h * w - 3 * 9 == 8
    n, c0, c1, h, w, groups = gn_shape("cpg4", BF16)
    assert c0 // groups == 4 and gn_fused_plan(h * w, c0, groups, BF16, n)[0] == 8   # one 16-bit chunk = two groups
    n, c0, c1, h, w, groups = gn_shape("concat_straddle", BF16)
    cpg = (c0 + c1) // groups
    assert cpg == 30 and 10 * cpg < c0 < 11 * cpg and gn_fused_plan(h * w, c0 + c1, groups, BF16, n)[0] == 120    # group 10 has channels of both sources
    # ---- LayerNorm
    for rows, c, dtype in LN_CASES:
        count["layernorm " + ln_kernel(rows, c, dtype)] += 1
    assert ln_kernel(5, 4104, BF16) == "wave<MAXCH=16>" and ln_kernel(5, 2052, F32) == "wave<MAXCH=16>" and 4104 // 8 == 513 == 2052 // 4
    assert ln_kernel(5, 4096, BF16) == "wave<MAXCH=8>" and ln_kernel(5, 2048, F32) == "wave<MAXCH=8>"
    assert [ln_kernel(r, 320, BF16) for r in (1, 1023, 1024, 1027)] == ["wave<MAXCH=1>"] * 2 + ["rows<LPR=8,CPL=5>"] * 2
    assert [ln_kernel(r, 320, F32) for r in (1023, 1024)] == ["wave<MAXCH=2>"] * 2 and 1027 % 32 != 0 and 1024 % 32 == 0     # 4 waves x 8 rows per workgroup
    assert [ln_kernel(2000, c, BF16) for c in (192, 512, 1280, 640, 1024)] == ["rows<LPR=8,CPL=3>", "rows<LPR=16,CPL=4>", "rows<LPR=32,CPL=5>",
                                                                             "rows<LPR=16,CPL=5>", "rows<LPR=32,CPL=4>"]
    with capsys.disabled():
        print("\ncases per kernel:")
        for k in sorted(count):
            print(f"    {k:55s} {count[k]}")


# ------------------------------------------------------------------------------------------------ igemm, Linear, skinny
@functools.lru_cache(maxsize=None)
def igemm_ref(dtype, ksize, c0, c1, n_out, n, h, w, stride, pad, upsample, geglu):
    """dtype-rounded inputs and the fp64 result [M, n_dst] of bias + conv (+ GEGLU) + residual.  Shared: do not write to it."""
    k = c0 + c1
    x = rnd((n, k, h, w), 201, dtype)
    wt = rnd((n_out, k, ksize, ksize), 202, dtype, 1 / math.sqrt(k * ksize * ksize))
    b = torch.randn(n_out, generator=G(203)) * 0.1
    xr = x.double()
    if upsample == 1:
        xr = F.interpolate(xr, scale_factor=2.0, mode="nearest")
    if ksize == 3 and stride == 2 and pad == 0:
        xr = F.pad(xr, (0, 1, 0, 1))
    y = F.conv2d(xr, wt.double(), b.double(), stride=stride, padding=pad)
    if geglu:
        a, g = y.chunk(2, 1)
        y = a * F.gelu(g)
    y = y.permute(0, 2, 3, 1)
    ho, wo = y.shape[1:3]
    y = y.reshape(-1, y.shape[-1])
    res = rnd(tuple(y.shape), 204, dtype)
    return dict(x=x, wt=wt, b=b, y=y, res=res, ho=ho, wo=wo)


def to_nhwc(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


@gpu
@pytest.mark.parametrize("case", IGEMM_CASES, ids=[c["name"] for c in IGEMM_CASES])
def test_igemm_writes_stay_inside_a_wider_destination(ops, case):
    """every tile id a shape can keep, M = 231 (and 1) against every BM, 8 live columns in the last 64-wide tile: the output in columns
    [0, n_dst) of a buffer 16 columns wider (dst_ld > n_dst) with 256 guard rows; bias + contiguous residual, GEGLU, split-K reduces"""
    c, dtype = case, case["dtype"]
    pad = c.get("pad", c["ksize"] // 2)
    stride, up, geglu = c.get("stride", 1), c.get("upsample", 0), c["epi"] == EPI_GEGLU
    r = igemm_ref(dtype, c["ksize"], c["c0"], c["c1"], c["n_out"], c["n"], c["h"], c["w"], stride, pad, up, geglu)
    m, n_dst = r["y"].shape
    dst_dtype = F32 if c.get("dst_f32") else dtype
    buf = guarded(m, n_dst, dst_dtype, extra_cols=c["dst_ld"] - n_dst)
    assert buf.shape[1] == c["dst_ld"]
    pw = ops.pack_weight(r["wt"].cuda(), dtype, geglu=geglu, c_split=c["c0"] if c["c1"] else None)
    xg = to_nhwc(r["x"], dtype)
    x0, x1 = (xg[..., :c["c0"]].contiguous(), xg[..., c["c0"]:].contiguous()) if c["c1"] else (xg, None)
    res = r["res"].to(dtype).cuda() if c["residual"] else None
    ops.conv2d(x0, pw, r["b"].cuda(), x2=x1, stride=stride, pad=pad, upsample=up, residual=res, epilogue=c["epi"], out_dtype=dst_dtype,
               splitk=c["splitk"], tile=c["tile"], dst=buf[:m].view(c["n"], r["ho"], r["wo"], c["dst_ld"]))
    check_guard(buf, block(buf.shape, m, n_dst), 7.0, c["name"])
    close(buf[:m, :n_dst], r["y"] + (r["res"].double() if c["residual"] else 0.0), dtype, "igemm", c["name"])


@functools.lru_cache(maxsize=None)
def phase_ref(dtype, n_out, n, h, w):
    cin = 128
    x = rnd((n, cin, h, w), 211, dtype)
    wt = rnd((n_out, cin, 3, 3), 212, dtype, 1 / math.sqrt(cin * 9))
    b = torch.randn(n_out, generator=G(213)) * 0.1
    y = F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), wt.double(), b.double(), padding=1)
    return dict(x=x, wt=wt, b=b, y=y.permute(0, 2, 3, 1))


@gpu
@pytest.mark.parametrize("case", PHASE_CASES, ids=[c["name"] for c in PHASE_CASES])
def test_phase_convs_write_their_own_parity_only(ops, case):
    """upsample = 2..5: one phase at a time into a prefilled [n, 2h, 2w, dst_ld] buffer -- the pixels of the other three parities, the
    guard columns and the guard rows keep their fill; all four together equal interpolate + conv.  splitk = 2: the reduce kernel scatters"""
    c, dtype = case, case["dtype"]
    n, h, w, n_out, ld = c["n"], c["h"], c["w"], c["n_out"], c["dst_ld"]
    r = phase_ref(dtype, n_out, n, h, w)
    pws = [ops.pack_weight(t.cuda(), dtype) for t in ops.upsample_phase_weights(r["wt"])]
    xg, bias = to_nhwc(r["x"], dtype), r["b"].cuda()
    m2 = n * 4 * h * w
    for first in range(4):
        buf = guarded(m2, n_out, dtype)
        img = buf[:m2].view(n, 2 * h, 2 * w, ld)
        own = torch.zeros(buf.shape, dtype=torch.bool)
        order = [first] if first else [0, 1, 2, 3]            # phase 0 is followed by the other three
        for ph in order:
            ops.conv2d(xg, pws[ph], bias, pad=0, upsample=2 + ph, splitk=c["splitk"], tile=c["tile"], dst=img)
            own[:m2].view(n, 2 * h, 2 * w, ld)[:, ph >> 1::2, ph & 1::2, :n_out] = True
            check_guard(buf, own, 7.0, f"{c['name']} after phase {ph}")
        if not first:
            close(img[..., :n_out], r["y"], dtype, "igemm_phase", c["name"])
        else:
            py, px = first >> 1, first & 1
            close(img[:, py::2, px::2, :n_out], r["y"][:, py::2, px::2], dtype, "igemm_phase", f"{c['name']} phase {first} alone")


# ------------------------------------------------------------------------------------------------ attention
@functools.lru_cache(maxsize=None)
def attn_ref(heads, d, segs, dtype, scale=None, seed=300):
    """dtype-rounded q / k / v, the fp64 output [q rows, C] and the fp64 log2-domain log-sum-exp [heads, q rows].  Shared: do not write to it."""
    C_ = heads * d
    nq, nk = sum(s[0] for s in segs), sum(s[1] for s in segs)
    q, k, v = rnd((nq, C_), seed, dtype), rnd((nk, C_), seed + 1, dtype), rnd((nk, C_), seed + 2, dtype)
    sc = d ** -0.5 if scale is None else scale
    outs, lses, q0, k0 = [], [], 0, 0
    for ql, kl in segs:
        qq = q[q0:q0 + ql].double().view(ql, heads, d).transpose(0, 1)
        kk = k[k0:k0 + kl].double().view(kl, heads, d).transpose(0, 1)
        vv = v[k0:k0 + kl].double().view(kl, heads, d).transpose(0, 1)
        s = qq @ kk.transpose(1, 2) * sc
        outs.append((torch.softmax(s, -1) @ vv).transpose(0, 1).reshape(ql, C_))
        lses.append(torch.logsumexp(s, -1) / math.log(2))
        q0, k0 = q0 + ql, k0 + kl
    return dict(heads=heads, d=d, segs=segs, q=q, k=k, v=v, out=torch.cat(outs), lse=torch.cat(lses, 1), scale=scale)


# log-sum-exp, absolute, log2 domain.  16-bit: the project's 3e-2 (test_hip_ops.py::test_attention_long_cross_spike_and_lse).  f32: the
# statistic is max + log2(sum) of scores of magnitude <= 64 in the log2 domain, each a sum of <= 160 fp32 products: 64 x 2^-24 x
# sqrt(160) ~ 5e-5 of rounding in a score carries over one to one, hence 1e-4.
LSE_TOL = {F32: 1e-4, BF16: 3e-2, F16: 3e-2}


def run_attention(ops, c, dtype, what, guard=False, lse=True, extra_len=0):
    """plain: contiguous q / k / v / out.  guard: `out` is a column and row slice of a buffer of 7.0 with 8 guard columns (ld_o > heads*d), a gap
    of unowned rows after the first segment (q_row0 not contiguous), 256 tail rows; lse is [heads, lse_ld > rows] of -7.0; max_q_len is larger
    than every segment"""
    heads, d, segs = c["heads"], c["d"], c["segs"]
    C_, nq = heads * d, c["q"].shape[0]
    gap = 3 if guard else 0
    first = segs[0][0]
    rows_q = torch.cat([torch.arange(first), torch.arange(first, nq) + gap])          # logical q row -> device row
    table, q0, k0 = [], 0, 0
    for i, (ql, kl) in enumerate(segs):
        table.append([q0 + (gap if i else 0), ql, k0, kl])
        q0, k0 = q0 + ql, k0 + kl
    seg = torch.tensor(table, dtype=torch.int32, device="cuda")
    qd = torch.zeros(nq + gap, C_)
    qd[rows_q] = c["q"]
    n_rows = nq + gap
    buf = torch.full((n_rows + (GUARD_ROWS if guard else 0), C_ + (8 if guard else 0)), 7.0, dtype=dtype, device="cuda")
    lse_ld = n_rows + (40 if guard else 0)
    lse_buf = torch.full((heads, lse_ld), -7.0, device="cuda") if lse else None
    ops.attention(qd.to(dtype).cuda(), c["k"].to(dtype).cuda(), c["v"].to(dtype).cuda(), heads, d, seg, max(s[0] for s in segs) + extra_len,
                  scale=c["scale"], lse=lse_buf, out=buf[:n_rows, :C_])
    own = torch.zeros(buf.shape, dtype=torch.bool)
    own[rows_q, :C_] = True
    check_guard(buf, own, 7.0, f"{what} out")
    close(buf.cpu()[rows_q, :C_], c["out"], dtype, "attention", what)
    if lse:
        own = torch.zeros(lse_buf.shape, dtype=torch.bool)
        own[:, rows_q] = True
        check_guard(lse_buf, own, -7.0, f"{what} lse")
        e = record_err(f"attention/lse_abs/{NAME[dtype]}", float((lse_buf.double().cpu()[:, rows_q] - c["lse"]).abs().max()))
        assert e <= LSE_TOL[dtype], f"{what}: log-sum-exp off by {e:.3e} (tol {LSE_TOL[dtype]})"


ATTN_WIDTHS = [pytest.param(t, d, id=f"d{d}-{NAME[t]}") for t in DTYPES for d in DP_WIDTHS[t]]


@gpu
@pytest.mark.parametrize("dtype,d", ATTN_WIDTHS)
def test_attention_forward_every_head_width(ops, dtype, d):
    """every attention_kernel<T, DP, ONES> instantiation (DP = 16 ... 160, ONES for the 16-bit widths below their DP), two heads, segments
    around the 128-row and 64-key tiles: out and the log-sum-exp against fp64"""
    run_attention(ops, attn_ref(2, d, DP_SEGS, dtype), dtype, f"d{d}")


@gpu
@pytest.mark.parametrize("dtype,d", [pytest.param(t, d, id=f"d{d}-{NAME[t]}") for t, d in GUARD_WIDTHS])
def test_attention_forward_writes_stay_inside_the_segments(ops, dtype, d):
    """ONES accumulates the softmax denominator in output column head_dim: for the last head that is the first guard column.  Guard columns,
    the rows between two segments, the tail rows and the lse entries outside the segments keep their fill; max_q_len > every segment"""
    run_attention(ops, attn_ref(2, d, DP_SEGS, dtype), dtype, f"d{d} guarded", guard=True, extra_len=200)


@gpu
@pytest.mark.parametrize("dtype,d", [pytest.param(t, d, id=f"d{d}-{NAME[t]}") for t, d in SCALE_WIDTHS])
def test_attention_forward_with_a_scale_of_its_own(ops, dtype, d):
    run_attention(ops, attn_ref(2, d, DP_SEGS, dtype, scale=0.05), dtype, f"d{d} scale 0.05", guard=True)


@gpu
@pytest.mark.parametrize("dtype,d,kernel", WIDE, ids=[w[2] for w in WIDE])
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guarded"])
def test_attention_wide_kernel(ops, dtype, d, kernel, guard):
    """attention_wide_kernel<T, 1 / 2 / 4> in every type that reaches it (no log-sum-exp above head_dim 160)"""
    run_attention(ops, attn_ref(2, d, WIDE_SEGS, dtype), dtype, kernel, guard=guard, lse=False, extra_len=9 if guard else 0)


@gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_attention_forward_without_the_xcd_remap(ops, dtype):
    """max_q_len = 2100 > 2048: workgroups in launch order (p.remap = 0), 17 query tiles for the long segment, one for the 3-row one"""
    run_attention(ops, attn_ref(2, 16, NOREMAP_SEGS, dtype), dtype, "no remap")


# ------------------------------------------------------------------------------------------------ attention_merge
MERGE_EPS = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -22}       # one output rounding plus fp32 arithmetic


@functools.lru_cache(maxsize=None)
def merge_case(heads, d, tokens, dtype, n_img=3):
    """fp64 attention of the same queries over two disjoint key sets, each result rounded to its device type; the reference is the merge
    formula of include/mvldm.h in fp64 on those ROUNDED inputs.  In image 1 side A dominates by 2^40, in image 2 side B.  Shared."""
    rows, C_ = n_img * tokens, heads * d
    g = G(400 + heads + tokens)
    q = torch.randn(rows, heads, d, generator=g, dtype=torch.float64)
    res = []
    for nk in (13, 29):
        k, v = torch.randn(nk, heads, d, generator=g, dtype=torch.float64), torch.randn(nk, heads, d, generator=g, dtype=torch.float64)
        s = torch.einsum("rhd,khd->hrk", q, k) * d ** -0.5
        res += [torch.einsum("hrk,khd->rhd", torch.softmax(s, -1), v).reshape(rows, C_).to(dtype), (torch.logsumexp(s, -1) / math.log(2)).float()]
    oa, la, ob, lb = res
    if n_img > 1:
        la[:, tokens:2 * tokens] += 40.0
    if n_img > 2:
        lb[:, 2 * tokens:] += 40.0
    lse = torch.logaddexp(la.double() * math.log(2), lb.double() * math.log(2)) / math.log(2)
    wa, wb = torch.exp2(la.double() - lse), torch.exp2(lb.double() - lse)                       # [heads, rows]
    ref = oa.double().view(rows, heads, d) * wa.t()[:, :, None] + ob.double().view(rows, heads, d) * wb.t()[:, :, None]
    return dict(oa=oa, la=la, ob=ob, lb=lb, ref=ref.reshape(rows, C_))


def merge_check(got, k, dtype, tokens, what):
    got, ref, eps = got.double().cpu(), k["ref"], MERGE_EPS[dtype]
    err = (got - ref).abs()
    record_err(f"merge/err_over_bound/{NAME[dtype]}", float((err / (eps * ref.abs() + eps * 1e-3)).max()))
    assert bool((err <= eps * ref.abs() + eps * 1e-3).all()), f"{what}: worst {float((err / (eps * ref.abs() + eps * 1e-3)).max()):.2f} x the bound"
    # a side that dominates by 2^40 IS the result: exactly, where 2^-40 of the other side is below half an ulp of it
    for img, (dom, oth) in ((1, ("oa", "ob")), (2, ("ob", "oa"))):
        sl = slice(img * tokens, (img + 1) * tokens)
        a, b = k[dom][sl].double(), k[oth][sl].double()
        sure = a.abs() >= b.abs() * 2.0 ** -10 if dtype == F32 else torch.ones_like(a, dtype=torch.bool)
        assert torch.equal(got[sl][sure], a[sure]), f"{what}: image {img} is not its dominant side"


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("tokens", [1, 37])
@pytest.mark.parametrize("heads,d", [(5, 64), (8, 40)], ids=["5x64", "8x40"])
def test_attention_merge_alone(ops, heads, d, tokens, dtype):
    """attn_merge_kernel against the header's formula: image maps that permute, ld_a / ld_b / ld_o wider than C and lse_ld wider than the rows
    with guards, then in place (out = oa)"""
    n_img, C_ = 3, heads * d
    k = merge_case(heads, d, tokens, dtype)
    rows = n_img * tokens
    a_img, b_img, o_img = [2, 0, 1], [1, 2, 0], [0, 2, 1]

    def place(t, img_map, ld, fill=0.0):            # logical image i -> rows of image img_map[i] of a [rows, ld] buffer
        o = torch.full((rows, ld), fill, dtype=t.dtype)
        for i, j in enumerate(img_map):
            o[j * tokens:(j + 1) * tokens, :t.shape[1]] = t[i * tokens:(i + 1) * tokens]
        return o

    def place_lse(t, img_map, ld):                  # [heads, rows] -> [heads, ld > rows], images moved alike
        o = torch.zeros(heads, ld)
        for i, j in enumerate(img_map):
            o[:, j * tokens:(j + 1) * tokens] = t[:, i * tokens:(i + 1) * tokens]
        return o
    oa = place(k["oa"], a_img, C_ + 16).cuda()
    ob = place(k["ob"], b_img, C_ + 8).cuda()
    la, lb = place_lse(k["la"], a_img, rows + 5).cuda(), place_lse(k["lb"], b_img, rows + 11).cuda()
    maps = [torch.tensor(m, dtype=torch.int32, device="cuda") for m in (a_img, b_img, o_img)]
    buf = guarded(rows, C_, dtype, extra_cols=24)
    ops.attention_merge(oa[:, :C_], la, ob[:, :C_], lb, *maps, tokens, heads, d, out=buf[:rows, :C_])
    check_guard(buf, block(buf.shape, rows, C_), 7.0, "merge")
    got = torch.empty(rows, C_, dtype=dtype)
    for i, j in enumerate(o_img):
        got[i * tokens:(i + 1) * tokens] = buf[j * tokens:(j + 1) * tokens, :C_].cpu()
    merge_check(got, k, dtype, tokens, "permuted")
    # in place: out = oa, every image onto itself
    same = torch.arange(n_img, dtype=torch.int32, device="cuda")
    oa2 = torch.full((rows + GUARD_ROWS, C_ + 8), 7.0, dtype=dtype, device="cuda")
    oa2[:rows, :C_] = k["oa"].cuda()
    ops.attention_merge(oa2[:rows, :C_], k["la"].cuda(), k["ob"].cuda(), k["lb"].cuda(), same, same, same, tokens, heads, d, out=oa2[:rows, :C_])
    check_guard(oa2, block(oa2.shape, rows, C_), 7.0, "merge in place")
    merge_check(oa2[:rows, :C_], k, dtype, tokens, "in place")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_attention_merge_of_two_attention_launches(ops, dtype):
    """ops.attention over keys A and over keys B with their log-sum-exp, merged, against fp64 attention over A u B"""
    heads, d, tokens, n_img, ka, kb = 8, 40, 37, 3, 50, 77
    C_ = heads * d
    segs_ab = tuple((tokens, ka + kb) for _ in range(n_img))
    c = attn_ref(heads, d, segs_ab, dtype, seed=420)
    kv = c["k"].view(n_img, ka + kb, C_), c["v"].view(n_img, ka + kb, C_)
    qg = c["q"].to(dtype).cuda()
    outs, lses = [], []
    for lo, hi in ((0, ka), (ka, ka + kb)):
        kk, vv = (t[:, lo:hi].reshape(-1, C_).to(dtype).cuda() for t in kv)
        lse = torch.zeros(heads, n_img * tokens, device="cuda")
        outs.append(ops.attention(qg, kk, vv, heads, d, ops.make_segments([tokens] * n_img, [hi - lo] * n_img), tokens, lse=lse))
        lses.append(lse)
    same = torch.arange(n_img, dtype=torch.int32, device="cuda")
    got = ops.attention_merge(outs[0], lses[0], outs[1], lses[1], same, same, same, tokens, heads, d)
    # 16-bit: each of the two inputs was rounded once to the output type before the merge rounds again -- 2 x the worst-element bound
    close(got, c["out"], dtype, "merge_e2e", "A u B", worst_factor=1.0 if dtype == F32 else 2.0)


# ------------------------------------------------------------------------------------------------ gather_rows
@gpu
@pytest.mark.parametrize("n_rows", [1, 1000])
@pytest.mark.parametrize("row_bytes", [16, 48, 40960])
def test_gather_rows_is_exact(ops, row_bytes, n_rows):
    """src_index only, dst_index only, both, neither; the same buffer with disjoint rows; untouched destination rows keep their fill"""
    g = G(500 + n_rows)
    w = row_bytes // 4
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_rows + 7, w), generator=g, dtype=torch.int32)
    si = torch.randint(0, n_rows + 7, (n_rows,), generator=g, dtype=torch.int32)              # sources may repeat
    di = torch.randperm(n_rows + 13, generator=g)[:n_rows].to(torch.int32)                    # destinations are distinct
    srcg = src.cuda()
    for use_s, use_d in ((True, False), (False, True), (True, True), (False, False)):
        dst = torch.full((n_rows + 13, w), 7, dtype=torch.int32, device="cuda")
        ops.gather_rows(srcg, dst, si.cuda() if use_s else None, di.cuda() if use_d else None, n_rows=n_rows)
        want = torch.full((n_rows + 13, w), 7, dtype=torch.int32)
        want[di.long() if use_d else torch.arange(n_rows)] = src[si.long() if use_s else torch.arange(n_rows)]
        assert torch.equal(dst.cpu(), want), (use_s, use_d)
    both = torch.cat([src[:n_rows], torch.full((n_rows + 3, w), 7, dtype=torch.int32)]).cuda()          # rows [0, n): sources, [n, 2n): destinations
    perm = torch.randperm(n_rows, generator=g).to(torch.int32)
    ops.gather_rows(both, both, perm.cuda(), (torch.arange(n_rows, dtype=torch.int32) + n_rows).cuda(), n_rows=n_rows)
    want = torch.cat([src[:n_rows], src[:n_rows][perm.long()], torch.full((3, w), 7, dtype=torch.int32)])
    assert torch.equal(both.cpu(), want)


# ------------------------------------------------------------------------------------------------ GroupNorm
@functools.lru_cache(maxsize=None)
def gn_ref(name, dtype):
    n, c0, c1, h, w, groups = gn_shape(name, dtype)
    c = c0 + c1
    x = rnd((n, c, h, w), 600, dtype, 1.5) + rnd((1, c, 1, 1), 601, dtype, 0.5)
    x = x.to(dtype).float()
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=G(602)), 0.1 * torch.randn(c, generator=G(603))
    xd = x.double()
    y = F.group_norm(xd, groups, gamma.double(), beta.double(), 1e-5)
    xg = xd.view(n, groups, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    return dict(x=x, gamma=gamma, beta=beta, y=y, ys=F.silu(y), mean=mean, var=var)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("name", list(GN_CASES))
def test_groupnorm_forward_edges(ops, name, silu, dtype):
    """every gn_fused_kernel<T, KT> and the two-launch path (a short last slab; cpg = 1), two groups in one chunk, a group across the x / x2
    boundary: y into a buffer with guard rows, (mean, rstd) against fp64; the library's 2-or-3 passes answer agrees with the mirror"""
    from mv_ldm_amd import _lib as L
    n, c0, c1, h, w, groups = gn_shape(name, dtype)
    c, k = c0 + c1, gn_ref(name, dtype)
    fused = gn_kernel(n, c0, c1, h, w, groups, dtype) != "two_launch"
    assert L.load().mvldm_groupnorm_passes(n, h * w, c, groups, ops.dt(dtype)) == (2 if fused else 3)
    xg = to_nhwc(k["x"], dtype)
    xa, xb = (xg[..., :c0].contiguous(), xg[..., c0:].contiguous()) if c1 else (xg, None)
    rows = n * h * w
    buf = torch.full((rows + GUARD_ROWS, c), 7.0, dtype=dtype, device="cuda")
    stats = torch.full((n + 2, groups, 2), -7.0, device="cuda")
    ops.groupnorm(xa, k["gamma"].cuda(), k["beta"].cuda(), groups, 1e-5, silu, x2=xb, stats_out=stats[:n], out=buf[:rows])
    check_guard(buf, block(buf.shape, rows, c), 7.0, f"{name} y")
    assert bool((stats[n:] == -7.0).all()), "statistics past the last image written"
    close(buf[:rows].view(n, h, w, c).permute(0, 3, 1, 2), k["ys"] if silu else k["y"], dtype, "groupnorm", name)
    # statistics: 1e-5 relative -- fp32 / fp64 sums of exactly representable inputs in every dtype; the mean relative to the group's RMS
    # sqrt(mean^2 + var) (the scale of the sums it is formed from), rstd relative to itself
    st = stats[:n].double().cpu()
    rstd = (k["var"] + 1e-5).rsqrt()
    e_mean = record_err(f"groupnorm/mean_rel/{NAME[dtype]}", float(((st[..., 0] - k["mean"]).abs() / (k["mean"] ** 2 + k["var"]).sqrt()).max()))
    e_rstd = record_err(f"groupnorm/rstd_rel/{NAME[dtype]}", float(((st[..., 1] - rstd).abs() / rstd).max()))
    assert e_mean <= 1e-5 and e_rstd <= 1e-5, (name, e_mean, e_rstd)


# ------------------------------------------------------------------------------------------------ LayerNorm
@functools.lru_cache(maxsize=None)
def ln_ref(rows, c, dtype):
    x = rnd((rows, c), 700, dtype, 2.0)
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=G(701)), 0.1 * torch.randn(c, generator=G(702))
    return dict(x=x, gamma=gamma, beta=beta, y=F.layer_norm(x.double(), (c,), gamma.double(), beta.double(), 1e-5))


@gpu
@pytest.mark.parametrize("rows,c,dtype", [pytest.param(r, c, t, id=f"{r}x{c}-{NAME[t]}") for r, c, t in LN_CASES])
def test_layernorm_forward_edges(ops, rows, c, dtype):
    """MAXCH = 16 (513 chunk columns: one live lane in the last sweep), both sides of the rows >= 1024 switch with a ragged last row group,
    one row; guard rows after the last row"""
    k = ln_ref(rows, c, dtype)
    buf = torch.full((rows + GUARD_ROWS, c), 7.0, dtype=dtype, device="cuda")
    ops.layernorm(k["x"].to(dtype).cuda(), k["gamma"].cuda(), k["beta"].cuda(), out=buf[:rows])
    check_guard(buf, block(buf.shape, rows, c), 7.0, f"layernorm {rows}x{c}")
    close(buf[:rows], k["y"], dtype, "layernorm", f"{rows}x{c}")
