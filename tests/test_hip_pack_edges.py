"""The weight packers (csrc/pack.hip, `mvldm_pack_skinny` of csrc/skinny.hip) byte for byte: every body of `pack_job_kernel`, the scalar
fallback of each LDS-tiled body, the row guards, the zero padding, the grid-stride second pass and the job lookup of the batched launch,
against the layout of include/mvldm.h written out on the CPU (tests/pack_ref.py).  The sibling of test_hip_forward_edges.py,
test_hip_backward_edges.py, test_hip_glue_edges.py and test_hip_wgrad_edges.py.

No tolerance anywhere: a pack is a gather and one IEEE conversion, so the packed bits equal those of `torch.Tensor.to(dtype)` on the CPU
(`pack_ref.same_bits`: -0.0 is not 0.0; NaN is compared by position).  Every destination is the middle of a buffer of byte 0xAB with 64
rows of k_pad elements on either side; after a launch the guards still hold 0xAB and EVERY element of `[n_pad, k_pad]` has the reference's
bits, the zero padding included (`ops.pack_weight` allocates with torch.empty, the trainer re-packs in place).  The entry points are the C
ones (`mvldm_pack_weight`, `mvldm_pack_job_prepare` + `ops.PackBatch`), so that c_pad, n_pad and the source pointer are the test's.

Sources are seeded randn with planted values in the first and the last real row (PLANT: -0.0, round-to-even ties of bf16 and f16, f16
subnormals and subnormal ties, +-70000 -> f16 inf), lying in a larger fp32 buffer of 3.0 (a read past the weight would put a 3.0 where a 0
belongs); an "unaligned" source starts at element 1 of a 16-byte aligned address.  Nothing is placed at the end of an allocation: stray
reads are the business of the index predicates of the CPU test, which restates each body's reads and bounds them by the weight's size.

Only the four CPU tests are unmarked; every device test carries the gpu mark.

Found by this module (both through the C ABI only: no Python caller made such a pack):
  1. a 16-bit block-major 3x3 job with `geglu` went to pack_fwd_k3_body, which never interleaves rows: (128, 64, 3) with geglu came out in
     source row order, unlike its f32 pack.  pack_job_prepare now keeps the generic body for geglu with ksize != 1, so `k3_geglu` below is
     a PACK_GENERIC case (asserted in the CPU test).
  2. with `geglu` and n_pad > n_out, orig_col mapped padding rows back into the weight: (128, 64, 1) with n_pad = 256 had rows 128..159 and
     192..223 filled with copies of source rows 64..127 instead of zeros, in the forward 1x1 body (bf16 / f16) and in the generic body
     (f32 (128, 16, 1)).  Both bodies now write zero for np >= n_out before they consult orig_col.
"""
import ctypes as C
import functools
import time

import pytest
import torch

import pack_ref as R
from pack_ref import check_packed, guarded, interior, pack_ref, same_bits, skinny_ref

gpu = pytest.mark.gpu
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
HALF = [BF16, F16]
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
GENERIC, FWD_K1, FWD_K3, T_K3, T_K1 = 0, 1, 2, 3, 4        # csrc/pack.hip: enum { PACK_GENERIC ... PACK_T_K1 }
MAX_BLOCKS = 65535
JUNK, JUNK_ELEMS = 3.0, 64                                   # fp32 around every source
PLANT = (-0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,             # bf16 ties: down to 1.0 (even), up to 1 + 2^-6 (even)
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,                 # f16 ties: down to 1.0, up to 1 + 2^-9
         1e-6, 2.0 ** -25, 3 * 2.0 ** -25,                   # f16 subnormal; subnormal ties: to 0.0, to 2^-23
         70000.0, -70000.0)                                  # past f16's largest finite value


@pytest.fixture(scope="module")
def lib():
    from mv_ldm_amd import _lib as L
    return L.load()


def cdiv(a, b):
    return (a + b - 1) // b


def roundup(a, b):
    return cdiv(a, b) * b


def epc(dtype):
    return 4 if dtype == F32 else 8


# ------------------------------------------------------------------------------------------------ cases
def fwd(n_out, c_in, ks, *, c_pad=None, n_pad=None, geglu=False, unaligned=False):
    return dict(n_out=n_out, c_in=c_in, ks=ks, c_pad=c_pad, n_pad=n_pad, geglu=geglu, unaligned=unaligned, t=False, c_off=0, n_rows=n_out)


def tr(n_out, c_in, ks, c_off, n_rows, *, n_pad=None, unaligned=False):
    return dict(n_out=n_out, c_in=c_in, ks=ks, c_pad=None, n_pad=n_pad, geglu=False, unaligned=unaligned, t=True, c_off=c_off, n_rows=n_rows)


K1 = {      # pack_fwd_k1_body -> (quads on the 16-byte path, quads on the scalar path that read anything)
    "k1_straddle": (fwd(5, 70, 1, c_pad=128), (51, 39)),
    "k1_cin67": (fwd(64, 67, 1, c_pad=128), (256, 832)),
    "k1_unaligned": (fwd(8, 64, 1, unaligned=True), (0, 128)),
    "k1_geglu_pad": (fwd(128, 64, 1, geglu=True, n_pad=256), (2048, 0)),
    "k1_npad70": (fwd(70, 64, 1, n_pad=70), (1120, 0)),
}
K3 = {      # pack_fwd_k3_body -> per 64-channel block: F (16-byte loads) or S (per float)
    "k3_three_rows": (fwd(3, 128, 3), "FF"),
    "k3_partial_block": (fwd(70, 72, 3, c_pad=128), "FS"),
    "k3_cin66": (fwd(6, 66, 3, c_pad=128), "SS"),
    "k3_unaligned": (fwd(8, 64, 3, unaligned=True), "S"),
    "k3_npad70": (fwd(70, 64, 3, n_pad=70), "F"),
}
K3_GEGLU = {"k3_geglu": fwd(128, 64, 3, geglu=True)}         # finding 1: the generic body since the fix
T3 = {      # pack_t_body<3> -> per 8-row group: F or S
    "t3_coff3": (tr(128, 40, 3, 3, 21), "SSSSSSSS"),
    "t3_nout125": (tr(125, 32, 3, 0, 32), "FFFFSSSS"),
    "t3_cpad64": (tr(60, 16, 3, 8, 8), "FSSSSSSS"),
    "t3_cin30": (tr(64, 30, 3, 0, 30), "SSSSSSSS"),
    "t3_unaligned": (tr(64, 16, 3, 0, 16, unaligned=True), "SSSSSSSS"),
    "t3_npad20": (tr(64, 24, 3, 0, 20, n_pad=20), "FFS"),
}
T1 = {      # pack_t_body<1> -> per 64-row group
    "t1_coff2": (tr(192, 130, 1, 2, 128), "SS"),
    "t1_cin70": (tr(125, 70, 1, 0, 70), "SS"),
    "t1_unaligned": (tr(64, 64, 1, 0, 64, unaligned=True), "S"),
    "t1_npad100": (tr(64, 100, 1, 0, 100, n_pad=100), "FS"),
}
PHASES = [f"up_phase{i}" for i in range(4)]
GEN = {     # pack_generic_body -> the dtypes it runs in
    "g_ko1_3x3": (fwd(70, 96, 3), [F32]),
    "g_ko1_1x1": (fwd(70, 96, 1), [F32]),
    "g_t_3x3": (tr(40, 50, 3, 5, 33), [F32]),
    "g_t_1x1_ko1": (tr(96, 64, 1, 0, 64), [F32]),
    "g_tail": (fwd(70, 24, 3), [BF16]),
    "g_t_ko0": (tr(20, 24, 3, 4, 20), [BF16]),
    "g_geglu_pad": (fwd(128, 16, 1, geglu=True, n_pad=256), [F32]),
    **{p: (fwd(70, 64, 2), HALF) for p in PHASES},
}
TINY = {    # one workgroup each: the batched launch's first / last / adjacent jobs
    "tiny_fwd": fwd(4, 8, 1, n_pad=4),
    "tiny_t": tr(64, 64, 1, 0, 64),
}
BIG = {     # more than 65535 x 256 work items: the grid-stride second pass
    "big_generic": (fwd(4160, 4096, 1), F32),
    "big_k1": (fwd(8256, 8192, 1), BF16),
}
SPECS = {**{k: v[0] for k, v in K1.items()}, **{k: v[0] for k, v in K3.items()}, **K3_GEGLU, **{k: v[0] for k, v in T3.items()},
         **{k: v[0] for k, v in T1.items()}, **{k: v[0] for k, v in GEN.items()}, **TINY, **{k: v[0] for k, v in BIG.items()}}
GEN_RUNS = [(n, d) for n, (_, ds) in GEN.items() for d in ds]


def resolve(name, dtype):
    """the argument list of mvldm_pack_weight for a case: what `ops.pack_weight` / `ops.pack_weight_t` choose unless the case says otherwise"""
    s = SPECS[name]
    bk, taps = R.block_k(dtype), s["ks"] ** 2
    c_pad = s["c_pad"] or roundup(s["n_out"] if s["t"] else s["c_in"], epc(dtype))
    return dict(n_out=s["n_out"], c_in=s["c_in"], ksize=s["ks"], c_pad=c_pad, n_pad=s["n_pad"] or roundup(s["n_rows"], 64),
                k_pad=roundup(taps * c_pad, bk), geglu=int(s["geglu"]), k_order=int(c_pad % bk == 0), transpose=int(s["t"]),
                c_off=s["c_off"], n_rows=s["n_rows"])


def src_offset(name):
    """element offset of the weight from a 16-byte aligned address"""
    return 1 if SPECS[name]["unaligned"] else 0


def rule(a, dtype):
    """pack_job_prepare restated -> (kind, blocks)"""
    taps = a["ksize"] ** 2
    kind, blocks = GENERIC, min(cdiv(a["n_pad"] * a["k_pad"], 256), MAX_BLOCKS)
    tiled = dtype != F32 and a["k_order"] == 1 and a["c_pad"] % 64 == 0 and a["k_pad"] == taps * a["c_pad"] and a["ksize"] in (1, 3)
    if tiled and not (a["geglu"] and a["ksize"] != 1):
        if a["transpose"]:
            kind, blocks = (T_K3, a["c_pad"] // 64 * cdiv(a["n_pad"], 8)) if a["ksize"] == 3 else (T_K1, a["c_pad"] // 64 * cdiv(a["n_pad"], 64))
        elif a["ksize"] == 3:
            kind, blocks = FWD_K3, a["c_pad"] // 64 * cdiv(a["n_pad"], 4)
        else:
            kind, blocks = FWD_K1, min(cdiv(a["n_pad"] * (a["k_pad"] // 4), 256), MAX_BLOCKS)
    return kind, blocks


def plant(w, spec):
    w3 = w.reshape(w.shape[0], w.shape[1], -1)
    n_out, _, taps = w3.shape
    if spec["t"]:       # the first and the last row of the pack are input channels c_off and c_off + n_rows - 1
        m = min(len(PLANT), n_out // 2)
        w3[:m, spec["c_off"], 0] = torch.tensor(PLANT[:m])
        w3[n_out - m:, spec["c_off"] + spec["n_rows"] - 1, taps - 1] = torch.tensor(PLANT[:m])
    else:
        flat = w3.reshape(n_out, -1)
        m = min(len(PLANT), flat.shape[1])
        flat[0, :m] = torch.tensor(PLANT[:m])
        flat[n_out - 1, flat.shape[1] - m:] = torch.tensor(PLANT[:m])
    return w


@functools.lru_cache(maxsize=None)
def source(name):
    """the fp32 weight of a case on the CPU.  Shared: do not write to it."""
    assert name not in BIG
    s = SPECS[name]
    g = torch.Generator().manual_seed(9000 + list(SPECS).index(name))
    if name in PHASES:
        from mv_ldm_amd import ops
        w = ops.upsample_phase_weights(torch.randn(s["n_out"], s["c_in"], 3, 3, generator=torch.Generator().manual_seed(9000)))[PHASES.index(name)]
        w = w.clone()
    elif s["ks"] == 1:
        w = torch.randn(s["n_out"], s["c_in"], generator=g)
    else:
        w = torch.randn(s["n_out"], s["c_in"], s["ks"], s["ks"], generator=g)
    return plant(w, s)


def ref_args(a):
    return dict(c_pad=a["c_pad"], n_pad=a["n_pad"], k_pad=a["k_pad"], geglu=bool(a["geglu"]), k_order=a["k_order"], transpose=bool(a["transpose"]),
                c_off=a["c_off"], n_rows=a["n_rows"])


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """the packed tensor of a case on the CPU.  Shared: do not write to it."""
    return pack_ref(source(name), dtype, **ref_args(resolve(name, dtype)))


def fill_job(L, a, src_ptr, dst_ptr):
    j = L.PackJob()
    j.src, j.dst = src_ptr, dst_ptr
    for f in ("n_out", "c_in", "ksize", "c_pad", "n_pad", "k_pad", "geglu", "k_order", "transpose", "c_off", "n_rows"):
        setattr(j, f, a[f])
    return j


def prepared(lib, name, dtype):
    """the case as a prepared job with dummy pointers (host only) -> (status, kind, blocks)"""
    from mv_ldm_amd import _lib as L
    from mv_ldm_amd import ops
    j = fill_job(L, resolve(name, dtype), 0x10000 + 4 * src_offset(name), 0x20000)
    rc = lib.mvldm_pack_job_prepare(C.byref(j), ops.dt(dtype))
    return rc, j.kind, j.blocks


# ---- the reads of the LDS-tiled bodies, restated: which path a quad / block / row group takes and the largest source index it reads
def k1_paths(a, off):
    fast = slow = 0
    top = -1
    for np_ in range(a["n_pad"]):
        if np_ >= a["n_out"]:
            continue
        n = int(R.geglu_row(torch.tensor(np_), a["n_out"])) if a["geglu"] else np_
        assert 0 <= n < a["n_out"]
        for k in range(0, a["k_pad"], 4):
            if k + 3 < a["c_in"] and (n * a["c_in"] + k) % 4 == 0 and off % 4 == 0:
                fast, top = fast + 1, max(top, n * a["c_in"] + k + 3)
            elif k < a["c_in"]:
                slow, top = slow + 1, max(top, n * a["c_in"] + min(k + 3, a["c_in"] - 1))
    return fast, slow, top


def k3_paths(a, off):
    paths, top = "", -1
    for cb in range(a["c_pad"] // 64):
        f = cb * 64 + 64 <= a["c_in"] and a["c_in"] % 4 == 0 and off % 4 == 0
        paths += "F" if f else "S"
        last_c = cb * 64 + 63 if f else min(cb * 64 + 63, a["c_in"] - 1)
        if last_c >= cb * 64:
            top = max(top, ((a["n_out"] - 1) * a["c_in"] + last_c) * 9 + 8)
    return paths, top


def t_paths(a, off):
    taps = a["ksize"] ** 2
    rb = 8 if a["ksize"] == 3 else 64
    paths, top = "", -1
    for r0 in range(0, a["n_pad"], rb):
        f = r0 + rb <= a["n_rows"] and a["c_in"] % 4 == 0 and a["c_off"] % 4 == 0 and off % 4 == 0
        paths += "F" if f else "S"
        last_r = r0 + rb - 1 if f else min(r0 + rb - 1, a["n_rows"] - 1)
        if last_r >= r0:
            top = max(top, ((a["n_out"] - 1) * a["c_in"] + a["c_off"] + last_r) * taps + taps - 1)
    return paths, top


# ------------------------------------------------------------------------------------------------ CPU tests
def test_cases_reach_the_bodies_and_paths_they_are_named_for(lib):
    """CPU only: mvldm_pack_job_prepare puts every case on the body its table says, with the workgroups of the restated rule, and the
    restated path tests of each body say what the case is named for -- on the element offset the device test gives the source"""
    for table, kind in ((K1, FWD_K1), (K3, FWD_K3), (T3, T_K3), (T1, T_K1)):
        for name in table:
            for dtype in HALF:
                a = resolve(name, dtype)
                assert prepared(lib, name, dtype) == (0, kind, rule(a, dtype)[1]) and rule(a, dtype)[0] == kind, (name, NAME[dtype])
                assert a["k_order"] == 1 and a["k_pad"] == a["ksize"] ** 2 * a["c_pad"]
    numel = lambda a: a["n_out"] * a["c_in"] * a["ksize"] ** 2
    # forward 1x1
    for name, (_, want) in K1.items():
        a = resolve(name, BF16)
        fast, slow, top = k1_paths(a, src_offset(name))
        assert (fast, slow) == want and top == numel(a) - 1, (name, fast, slow, top)
    a = resolve("k1_straddle", BF16)
    assert (a["c_pad"], a["n_pad"], a["k_pad"]) == (128, 64, 128) and rule(a, BF16)[1] == 8
    assert [(n * 70) % 4 for n in range(5)] == [0, 2, 0, 2, 0]                            # rows alternate aligned / unaligned
    assert 68 < a["c_in"] <= 68 + 3 and 64 + 3 < a["c_in"]                                # the quad at k = 68 straddles c_in = 70; k = 64 is whole
    a = resolve("k1_cin67", BF16)
    assert a["c_in"] & 3 and [n for n in range(8) if (n * 67) % 4 == 0] == [0, 4] and 64 < a["c_in"] <= 64 + 3
    assert resolve("k1_unaligned", BF16)["c_in"] % 4 == 0 and src_offset("k1_unaligned") == 1
    a = resolve("k1_geglu_pad", BF16)       # finding 2: the interleave alone maps padding rows 128..159 and 192..223 onto source rows 64..127
    back = [np_ for np_ in range(a["n_out"], a["n_pad"]) if int(R.geglu_row(torch.tensor(np_), a["n_out"])) < a["n_out"]]
    assert back == list(range(128, 160)) + list(range(192, 224)) and a["n_pad"] == 256
    a = resolve("k1_npad70", BF16)
    assert a["n_pad"] == 70 and a["n_pad"] * (a["k_pad"] // 4) == 1120 and rule(a, BF16)[1] == 5 and 1120 % 256       # a ragged last workgroup
    # forward 3x3
    for name, (_, want) in K3.items():
        a = resolve(name, BF16)
        paths, top = k3_paths(a, src_offset(name))
        assert paths == want and top == numel(a) - 1, (name, paths, top)
    assert resolve("k3_three_rows", BF16)["n_out"] < 4
    a = resolve("k3_partial_block", BF16)
    assert a["c_in"] - 64 == 8 and a["c_in"] % 4 == 0 and a["n_out"] % 4 == 2 and a["n_pad"] == 128 and rule(a, BF16)[1] == 64     # block 1 partial
    assert resolve("k3_cin66", BF16)["c_in"] & 3 == 2                                      # slow because c_in & 3
    a = resolve("k3_npad70", BF16)
    assert a["n_pad"] == 70 and rule(a, BF16)[1] == 18 and 17 * 4 < a["n_pad"] < 18 * 4     # np0 + r < n_pad cuts the last group only
    # finding 1: geglu with a 3x3 kernel stays on the generic body
    for dtype in HALF:
        a = resolve("k3_geglu", dtype)
        assert a["k_order"] == 1 and a["geglu"] and prepared(lib, "k3_geglu", dtype) == (0, GENERIC, 288) and rule(a, dtype) == (GENERIC, 288)
    # transposed
    for table in (T3, T1):
        for name, (_, want) in table.items():
            a = resolve(name, BF16)
            paths, top = t_paths(a, src_offset(name))
            assert paths == want, (name, paths)
            last = ((a["n_out"] - 1) * a["c_in"] + a["c_off"] + a["n_rows"] - 1) * a["ksize"] ** 2 + a["ksize"] ** 2 - 1
            assert top == last < numel(a), (name, top, last)
    a = resolve("t3_coff3", BF16)
    assert a["c_off"] & 3 and a["c_in"] % 4 == 0 and 16 + 8 > a["n_rows"] > 16 and a["c_pad"] == 128 and rule(a, BF16)[1] == 16    # slow because c_off & 3
    a = resolve("t3_nout125", BF16)
    assert a["c_pad"] == 128 and a["n_out"] % 2 == 1 and a["n_rows"] % 8 == 0               # the pair (124, 125) is whole, (126, 127) padding
    assert resolve("t3_cpad64", BF16)["c_pad"] == 64 and resolve("t3_cin30", BF16)["c_in"] & 3 == 2
    a = resolve("t3_npad20", BF16)
    assert a["n_pad"] == a["n_rows"] == 20 and rule(a, BF16)[1] == 3                        # r0 + rl < n_pad cuts the last group only
    a = resolve("t1_coff2", BF16)
    assert a["c_off"] & 3 == 2 and a["c_pad"] == 192 and a["n_pad"] == 128 and rule(a, BF16)[1] == 6
    a = resolve("t1_cin70", BF16)
    assert a["c_in"] & 3 == 2 and a["c_pad"] == 128 and 64 < a["n_rows"] < 128
    a = resolve("t1_npad100", BF16)
    assert a["n_pad"] == 100 and rule(a, BF16)[1] == 2 and 64 + 64 > a["n_pad"]
    # n_out not a multiple of 64 under a c_pad that is: output-channel pairs that are half real, half padding do not exist for even n_out;
    # 125 is the odd one (pair 124 / 125 real, 126 / 127 padding) and 60 leaves pairs 60..63 padding
    assert resolve("t1_cin70", BF16)["n_out"] == 125 and resolve("t3_cpad64", BF16)["n_out"] == 60
    # the generic body
    for name, dtype in GEN_RUNS + [("tiny_fwd", BF16), ("tiny_fwd", F32)]:
        a = resolve(name, dtype)
        assert prepared(lib, name, dtype) == (0,) + rule(a, dtype) and rule(a, dtype)[0] == GENERIC, (name, NAME[dtype])
    want = {"g_ko1_3x3": (96, 1, 0, 864), "g_ko1_1x1": (96, 1, 0, 96), "g_t_3x3": (40, 0, 1, 384), "g_t_1x1_ko1": (96, 1, 1, 96),
            "g_geglu_pad": (16, 0, 0, 32)}
    for name, w in want.items():
        a = resolve(name, F32)
        assert (a["c_pad"], a["k_order"], a["transpose"], a["k_pad"]) == w, (name, a)
    a = resolve("g_tail", BF16)
    assert (a["k_order"], a["k_pad"], 9 * a["c_pad"]) == (0, 256, 216)                      # tap = k / c_pad reaches 9 and 10 in the tail
    a = resolve("g_t_ko0", BF16)
    assert (a["k_order"], a["transpose"], a["c_pad"], a["k_pad"]) == (0, 1, 24, 256)
    for dtype in HALF:
        a = resolve("up_phase0", dtype)
        assert (a["ksize"], a["k_order"], a["c_pad"], a["k_pad"], a["n_pad"]) == (2, 1, 64, 256, 128)    # block-major, but neither 1x1 nor 3x3
    # the second pass: more work items than 65535 workgroups of 256, and the last 64 rows belong to the second pass alone
    a = resolve("big_generic", F32)
    assert prepared(lib, "big_generic", F32) == (0, GENERIC, MAX_BLOCKS) and a["n_pad"] * a["k_pad"] == 17039360 > MAX_BLOCKS * 256
    assert MAX_BLOCKS * 256 // a["k_pad"] == 4095 and a["n_out"] == a["n_pad"] == 4160
    a = resolve("big_k1", BF16)
    assert prepared(lib, "big_k1", BF16) == (0, FWD_K1, MAX_BLOCKS) and a["n_pad"] * (a["k_pad"] // 4) == 16908288 > MAX_BLOCKS * 256
    assert MAX_BLOCKS * 256 // (a["k_pad"] // 4) == 8191 and a["n_out"] == a["n_pad"] == 8256
    # one workgroup each
    assert prepared(lib, "tiny_fwd", BF16)[1:] == (GENERIC, 1) and prepared(lib, "tiny_t", BF16)[1:] == (T_K1, 1)
    # the planted values do what they are there for
    p = torch.tensor(PLANT)
    assert p.to(BF16).float().tolist()[1:3] == [1.0, 1 + 2.0 ** -6] and p.to(F16).float().tolist()[3:5] == [1.0, 1 + 2.0 ** -9]
    assert 0 < float(p.to(F16)[5]) < 2.0 ** -14 and p.to(F16).float().tolist()[6:8] == [0.0, 2.0 ** -23]
    assert torch.isinf(p.to(F16)[8:]).all() and torch.isfinite(p.to(BF16)).all() and R.bits(p.to(BF16))[0] == -32768


def test_the_reference_is_the_layout_the_existing_tests_spell_out():
    """CPU only: pack_ref equals the permute / reshape expressions of test_hip_ops.py::test_block_major_packers_bit_exact and
    ::test_pack_weight_layout on those tests' own shapes"""
    g = torch.Generator().manual_seed(77)
    for dtype in HALF:
        w = torch.randn(70, 128, 3, 3, generator=g)
        ref = torch.zeros(128, 2, 9, 64)
        ref[:70] = w.reshape(70, 2, 64, 9).permute(0, 1, 3, 2)
        same_bits(pack_ref(w, dtype, c_pad=128, n_pad=128, k_pad=1152, k_order=1), ref.reshape(128, -1).to(dtype), "forward 3x3")
        wl = torch.randn(256, 192, generator=g)
        rows = torch.arange(256)
        blk, wi = rows // 32, rows % 32
        orig = torch.where(blk % 2 == 1, 128 + (blk // 2) * 32 + wi, (blk // 2) * 32 + wi)
        same_bits(pack_ref(wl, dtype, c_pad=192, n_pad=256, k_pad=192, k_order=1, geglu=True), wl[orig].to(dtype), "geglu 1x1")
        for wt, c_off, n_rows in ((torch.randn(128, 200, 3, 3, generator=g), 8, 150), (torch.randn(192, 96, generator=g), 0, 96)):
            n_out = wt.shape[0]
            taps = 9 if wt.ndim == 4 else 1
            n_pad = roundup(n_rows, 64)
            ref = torch.zeros(n_pad, n_out // 64, taps, 64)
            src = wt.reshape(n_out, wt.shape[1], taps)[:, c_off:c_off + n_rows].flip(-1)
            ref[:n_rows] = src.permute(1, 0, 2).reshape(n_rows, n_out // 64, 64, taps).permute(0, 1, 3, 2)
            got = pack_ref(wt, dtype, c_pad=n_out, n_pad=n_pad, k_pad=taps * n_out, k_order=1, transpose=True, c_off=c_off, n_rows=n_rows)
            same_bits(got, ref.reshape(n_pad, -1).to(dtype), f"transposed {tuple(wt.shape)}")
    w = torch.randn(70, 24, 3, 3, generator=g)
    ref = torch.zeros(128, 224)
    ref[:70, :9 * 24] = w.permute(0, 2, 3, 1).reshape(70, -1)
    same_bits(pack_ref(w, F32, c_pad=24, n_pad=128, k_pad=224, k_order=0), ref, "f32 tap-major")
    w2 = torch.randn(8, 128, 3, 3, generator=g)
    ref2 = torch.zeros(64, 2, 9, 64)
    ref2[:8] = w2.reshape(8, 2, 64, 9).permute(0, 1, 3, 2)
    same_bits(pack_ref(w2, BF16, c_pad=128, n_pad=64, k_pad=1152, k_order=1), ref2.reshape(64, -1).to(BF16), "bf16 block-major")
    wl = torch.randn(128, 16, generator=g)
    pg = pack_ref(wl, F32, c_pad=16, n_pad=128, k_pad=32, k_order=0, geglu=True)
    assert torch.equal(pg[0:32, :16], wl[0:32]) and torch.equal(pg[32:64, :16], wl[64:96])
    assert torch.equal(pg[64:96, :16], wl[32:64]) and torch.equal(pg[96:128, :16], wl[96:128]) and not pg[:, 16:].any()


def test_the_checks_can_fail():
    """CPU only: check_packed raises for one flipped low bit of the interior, for -0.0 against 0.0, for a number where a NaN belongs and
    for one touched guard byte on either side; a NaN of another payload passes"""
    for dtype in (BF16, F16, F32):
        want = torch.randn(8, 64, generator=torch.Generator().manual_seed(1)).to(dtype)
        want[3, 5], want[4, 4] = 0.0, float("nan")
        buf = guarded(8, 64, dtype, "cpu")
        assert buf.numel() == (8 + 128) * 64 * want.element_size() and bool((buf == 0xAB).all())
        interior(buf, 8, 64, dtype).copy_(want)
        check_packed(buf, want, "selftest")
        flipped = buf.clone()
        R.bits(interior(flipped, 8, 64, dtype))[2, 7] ^= 1
        with pytest.raises(AssertionError, match="1 of 512 packed elements differ, first at \\[2, 7\\]"):
            check_packed(flipped, want, "selftest")
        negz = buf.clone()
        interior(negz, 8, 64, dtype)[3, 5] = -0.0
        assert bool((interior(negz, 8, 64, dtype).float() == want.float())[3, 5])          # the comparison the older tests make cannot see it
        with pytest.raises(AssertionError, match="first at \\[3, 5\\]"):
            check_packed(negz, want, "selftest")
        nan = buf.clone()
        R.bits(interior(nan, 8, 64, dtype))[4, 4] |= 1                                      # another payload: still a NaN
        check_packed(nan, want, "selftest")
        interior(nan, 8, 64, dtype)[4, 4] = 1.0
        with pytest.raises(AssertionError, match="first at \\[4, 4\\]"):
            check_packed(nan, want, "selftest")
        g = 64 * 64 * want.element_size()
        for at in (0, g - 1, buf.numel() - g, buf.numel() - 1):
            bad = buf.clone()
            bad[at] ^= 1
            with pytest.raises(AssertionError, match="1 guard bytes written"):
                check_packed(bad, want, "selftest")


def test_prepare_refuses(lib):
    """CPU only: mvldm_pack_job_prepare returns a negative status and says why through mvldm_last_error()"""
    from mv_ldm_amd import _lib as L
    from mv_ldm_amd import ops
    ok = dict(n_out=64, c_in=64, ksize=3, c_pad=64, n_pad=64, k_pad=576, geglu=0, k_order=1, transpose=0, c_off=0, n_rows=64)

    def status(dtype=L.BF16, src=0x10000, dst=0x20000, **change):
        lib.mvldm_pack_job_prepare(None, L.BF16)                # a known last error to tell a fresh one from
        assert b"null job" in lib.mvldm_last_error()
        j = fill_job(L, {**ok, **change}, src, dst)
        return lib.mvldm_pack_job_prepare(C.byref(j), dtype), lib.mvldm_last_error().decode()

    assert status()[0] == 0 and status(transpose=1)[0] == 0 and status(geglu=1, ksize=1, k_pad=64)[0] == 0
    refused = {
        "an unknown dtype": (dict(dtype=7), "bad dtype 7"),
        "k_order 1 with c_pad % bk != 0": (dict(c_pad=72, k_pad=648), "k_order 1 needs c_pad"),
        "k_order 1 with c_pad % 32 != 0 in f32": (dict(dtype=ops.dt(F32), c_pad=80, k_pad=720), "k_order 1 needs c_pad"),
        "geglu with transpose": (dict(geglu=1, transpose=1), "(transpose): bad dims"),
        "geglu with n_out % 64 != 0": (dict(geglu=1, n_out=32), "GEGLU needs n_out"),
        "c_off + n_rows > c_in": (dict(transpose=1, c_off=8, n_rows=57), "(transpose): bad dims"),
        "n_pad < n_out": (dict(n_pad=63), "pack_weight: bad dims"),
        "n_pad < n_rows": (dict(transpose=1, n_pad=63), "(transpose): bad dims"),
        "k_pad < taps * c_pad": (dict(k_pad=575), "pack_weight: bad dims"),
        "k_pad < taps * c_pad, transposed": (dict(transpose=1, k_pad=575), "(transpose): bad dims"),
        "null src": (dict(src=None), "pack_weight: bad dims"),
        "null dst": (dict(dst=None), "pack_weight: bad dims"),
        "null src, transposed": (dict(src=None, transpose=1), "(transpose): bad dims"),
    }
    for what, (change, says) in refused.items():
        rc, msg = status(**change)
        assert rc < 0 and says in msg, (what, rc, msg)


# ------------------------------------------------------------------------------------------------ device launch
def device_source(w, off):
    """`w` at element offset `off` of a 16-byte aligned address, inside a larger fp32 buffer of JUNK"""
    buf = torch.full((w.numel() + 2 * JUNK_ELEMS,), JUNK, device="cuda")
    view = buf[JUNK_ELEMS + off:JUNK_ELEMS + off + w.numel()].view(w.shape)
    view.copy_(w)
    assert view.data_ptr() % 16 == 4 * off
    return view


def launch_single(lib, a, dtype, src, dst):
    from mv_ldm_amd import ops
    return lib.mvldm_pack_weight(src.data_ptr(), dst.data_ptr(), a["n_out"], a["c_in"], a["ksize"], a["c_pad"], a["n_pad"], a["k_pad"], a["geglu"],
                                 a["k_order"], ops.dt(dtype), a["transpose"], a["c_off"], a["n_rows"], ops.stream())


def run_single(lib, name, dtype):
    from mv_ldm_amd import _lib as L
    a = resolve(name, dtype)
    src = device_source(source(name), src_offset(name))
    buf = guarded(a["n_pad"], a["k_pad"], dtype, "cuda")
    L.check(launch_single(lib, a, dtype, src, interior(buf, a["n_pad"], a["k_pad"], dtype)))
    torch.cuda.synchronize()
    check_packed(buf.cpu(), reference(name, dtype), f"{name} {NAME[dtype]}")
    assert torch.equal(src.cpu(), source(name)), "the source changed"


@gpu
@pytest.mark.parametrize("dtype", HALF, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(K1))
def test_forward_1x1_body(lib, name, dtype):
    run_single(lib, name, dtype)


@gpu
@pytest.mark.parametrize("dtype", HALF, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(K3) + list(K3_GEGLU))
def test_forward_3x3_body(lib, name, dtype):
    run_single(lib, name, dtype)


@gpu
@pytest.mark.parametrize("dtype", HALF, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(T3) + list(T1))
def test_transposed_bodies(lib, name, dtype):
    run_single(lib, name, dtype)


@gpu
@pytest.mark.parametrize("name,dtype", GEN_RUNS, ids=[f"{n}-{NAME[d]}" for n, d in GEN_RUNS])
def test_generic_body(lib, name, dtype):
    run_single(lib, name, dtype)


@gpu
def test_nan_and_inf_keep_their_places(lib):
    """one small case: NaN and +-inf in the source arrive at their packed positions in every dtype, through the tiled and the generic body"""
    from mv_ldm_amd import _lib as L
    w = torch.randn(8, 64, generator=torch.Generator().manual_seed(5))
    w[0, 0], w[0, 1], w[3, 17], w[7, 62], w[7, 63] = float("nan"), float("inf"), float("nan"), float("-inf"), float("nan")
    for dtype in (BF16, F16, F32):
        a = dict(n_out=8, c_in=64, ksize=1, c_pad=64, n_pad=64, k_pad=64, geglu=0, k_order=1, transpose=0, c_off=0, n_rows=8)
        want = pack_ref(w, dtype, **ref_args(a))
        assert int(torch.isnan(want).sum()) == 3 and int(torch.isinf(want).sum()) == 2
        buf = guarded(64, 64, dtype, "cuda")
        L.check(launch_single(lib, a, dtype, device_source(w, 0), interior(buf, 64, 64, dtype)))
        torch.cuda.synchronize()
        check_packed(buf.cpu(), want, f"nan / inf {NAME[dtype]}")


# ------------------------------------------------------------------------------------------------ the second pass
@gpu
@pytest.mark.parametrize("name", list(BIG))
def test_grid_stride_second_pass(lib, name):
    """more work items than 65535 workgroups x 256 threads: the last 64 rows are written by the second trip of the grid-stride loop alone.
    Compared on the device against pack_ref evaluated there; the time of the launch is printed, not asserted"""
    from mv_ldm_amd import _lib as L
    dtype = BIG[name][1]
    a = resolve(name, dtype)
    assert prepared(lib, name, dtype)[2] == MAX_BLOCKS
    w = torch.randn(a["n_out"], a["c_in"], device="cuda", generator=torch.Generator(device="cuda").manual_seed(31))
    w[-1, :len(PLANT)] = torch.tensor(PLANT, device="cuda")
    w[-1, -len(PLANT):] = torch.tensor(PLANT, device="cuda").flip(0)
    w[0, :len(PLANT)] = torch.tensor(PLANT, device="cuda")
    want = pack_ref(w, dtype, **ref_args(a))
    buf = guarded(a["n_pad"], a["k_pad"], dtype, "cuda")
    dst = interior(buf, a["n_pad"], a["k_pad"], dtype)
    assert w.data_ptr() % 16 == 0
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    start.record()
    L.check(launch_single(lib, a, dtype, w, dst))
    stop.record()
    torch.cuda.synchronize()
    print(f"\n{name} {NAME[dtype]}: launch {start.elapsed_time(stop):.3f} ms on the device, {1e3 * (time.perf_counter() - t0):.1f} ms wall")
    check_packed(buf, want, f"{name} {NAME[dtype]}")
    same_bits(dst[-1], w[-1].to(dtype), f"{name}: the last row")


# ------------------------------------------------------------------------------------------------ the batched launch
BATCH = {
    BF16: ["tiny_t", "k1_straddle", "k3_partial_block", "tiny_fwd", "tiny_t", "t3_coff3", "t1_coff2", "g_tail", "g_t_ko0", "up_phase2",
           "k1_geglu_pad", "k3_npad70", "t3_npad20", "k3_geglu", "tiny_fwd"],
    F32: ["tiny_fwd", "g_ko1_3x3", "g_ko1_1x1", "tiny_fwd", "tiny_fwd", "g_t_3x3", "g_t_1x1_ko1", "g_geglu_pad", "g_tail", "tiny_fwd"],
}


@gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_batch_finds_every_job(lib, dtype):
    """one PackBatch over jobs of every kind -- a one-workgroup job first, one last, two adjacent -- run with the workgroup -> job table,
    with the binary search over block0, and as single launches: all three write the reference's bytes into guarded destinations.  Then
    a batch of one job, and an empty one"""
    from mv_ldm_amd import _lib as L
    from mv_ldm_amd import ops
    names = BATCH[dtype]
    srcs = [device_source(source(n), src_offset(n)) for n in names]

    def jobs_into_fresh_buffers(which):
        bufs, jobs = [], []
        for i in which:
            a = resolve(names[i], dtype)
            bufs.append(guarded(a["n_pad"], a["k_pad"], dtype, "cuda"))
            j = fill_job(L, a, srcs[i].data_ptr(), interior(bufs[-1], a["n_pad"], a["k_pad"], dtype).data_ptr())
            L.check(lib.mvldm_pack_job_prepare(C.byref(j), ops.dt(dtype)))
            jobs.append(j)
        return bufs, jobs

    def check(bufs, which, way):
        torch.cuda.synchronize()
        for i, buf in zip(which, bufs):
            check_packed(buf.cpu(), reference(names[i], dtype), f"{way}: job {i} {names[i]} {NAME[dtype]}")

    everything = list(range(len(names)))
    _, jobs = jobs_into_fresh_buffers(everything)
    blocks = [j.blocks for j in jobs]
    assert blocks[0] == 1 and blocks[-1] == 1 and blocks[3] == blocks[4] == 1 and max(blocks) > 32
    if dtype == BF16:
        assert {j.kind for j in jobs} == {GENERIC, FWD_K1, FWD_K3, T_K3, T_K1}
    for way in ("table", "search", "singles"):
        bufs, jobs = jobs_into_fresh_buffers(everything)
        if way == "singles":
            for i in everything:
                a = resolve(names[i], dtype)
                L.check(launch_single(lib, a, dtype, srcs[i], interior(bufs[i], a["n_pad"], a["k_pad"], dtype)))
        else:
            pb = ops.PackBatch(jobs, dtype, "cuda")
            assert pb.total_blocks == sum(blocks) and pb.block_job.numel() == sum(blocks)
            table = torch.frombuffer(bytearray(pb.table.cpu().numpy().tobytes()), dtype=torch.int32).view(len(jobs), -1)
            assert table[:, -1].tolist() == [sum(blocks[:i]) for i in everything]          # block0: the exclusive prefix sum
            if way == "search":
                pb.block_job = None
            pb.run()
        check(bufs, everything, way)
    for way in ("table", "search"):
        bufs, jobs = jobs_into_fresh_buffers([2])
        pb = ops.PackBatch(jobs, dtype, "cuda")
        assert pb.n == 1
        if way == "search":
            pb.block_job = None
        pb.run()
        check(bufs, [2], f"one job, {way}")
    empty = ops.PackBatch([], dtype, "cuda")
    assert empty.n == 0 and empty.total_blocks == 0 and empty.block_job is None
    empty.run()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the fragment-order pack
@gpu
@pytest.mark.parametrize("dtype", HALF, ids=["bf16", "f16"])
@pytest.mark.parametrize("n_out,c_in,ks,geglu", [(64, 64, 1, False), (80, 128, 3, False), (128, 64, 1, True)], ids=["64x64", "80x128x3x3", "geglu"])
def test_pack_skinny(lib, n_out, c_in, ks, geglu, dtype):
    """mvldm_pack_skinny against the header's 16-byte-unit formula, into a guarded destination; its source pack (made by pack_ref, not
    by a kernel) stays as it was"""
    from mv_ldm_amd import _lib as L
    from mv_ldm_amd import ops
    g = torch.Generator().manual_seed(600 + n_out)
    w = torch.randn(n_out, c_in, ks, ks, generator=g) if ks > 1 else torch.randn(n_out, c_in, generator=g)
    n_pad, k_pad = roundup(n_out, 64), ks * ks * c_in
    packed = pack_ref(w, dtype, c_pad=c_in, n_pad=n_pad, k_pad=k_pad, k_order=1, geglu=geglu)
    want = skinny_ref(packed, geglu)
    assert sorted(R.bits(want).flatten().tolist()) == sorted(R.bits(packed).flatten().tolist())      # a permutation of 16-byte units
    src = packed.cuda()
    buf = guarded(n_pad, k_pad, dtype, "cuda")
    L.check(lib.mvldm_pack_skinny(src.data_ptr(), interior(buf, n_pad, k_pad, dtype).data_ptr(), n_pad, k_pad, int(geglu), ops.dt(dtype), ops.stream()))
    torch.cuda.synchronize()
    check_packed(buf.cpu(), want, f"skinny {n_out}x{c_in}x{ks} geglu={geglu} {NAME[dtype]}")
    same_bits(src.cpu(), packed, "the source pack")


# ------------------------------------------------------------------------------------------------ refusal
@gpu
def test_a_refused_pack_writes_nothing(lib):
    """a mvldm_pack_weight call that prepare refuses returns a negative status and leaves a sentinel-filled destination untouched"""
    src = device_source(source("k1_unaligned"), 0)
    buf = guarded(64, 64, BF16, "cuda")
    a = dict(resolve("k1_unaligned", BF16), geglu=1, transpose=1)
    rc = launch_single(lib, a, BF16, src, interior(buf, 64, 64, BF16))
    torch.cuda.synchronize()
    assert rc < 0 and b"pack_weight" in lib.mvldm_last_error()
    assert bool((buf == R.GUARD_BYTE).all())
