"""what the crop shim's per-image mirror flag costs on the device (csrc/cropshim.hip, `mvldm_crop_shim_flip`):
    python tools/cropshim_flip_time.py [n=30] [--parent-lib PATH/libmvldm_hip.so] [--json OUT]
n uint8 frames of 360 x 640 -> 256 x 256 (a micro-batch of 6 scenes x 5 views), tables warm.  Variants, timed ALTERNATING in one process: the
unflagged entry `mvldm_crop_shim`, the flagged one with a null pointer, with all flags zero, all set, every other one set -- and, with
`--parent-lib`, `mvldm_crop_shim` of a library built from the parent commit (loaded beside this build's; it shares nothing with it).
Per variant: microseconds a call from windows of back-to-back calls between device events ("hot": the source stays in the caches) and
from single calls behind a 640 MB cache-evicting fill ("cold"); median, minimum and maximum over the rounds, so that a difference can
be read against the spread of the same code.  All variants are checked to give the same bytes as expected before anything is timed.
No threshold: the figures go to DESIGN.md and profiles/."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mv_ldm_amd import _lib as L, ops

args = [int(a) for a in sys.argv[1:] if a.isdigit()]
n = (args + [30])[0]
h, w, shape = 360, 640, (256, 256)
ROUNDS, HOT_CALLS, COLD_CALLS = 11, 200, 5
lib = L.load()
src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
need = ops.crop_shim_workspace_bytes(n, h, w, shape)
ws = torch.empty(need, dtype=torch.uint8, device="cuda")
dst = torch.empty(n, 3, *shape, dtype=torch.float32, device="cuda")
flags = {"flip_zero": torch.zeros(n, dtype=torch.uint8, device="cuda"), "flip_all": torch.ones(n, dtype=torch.uint8, device="cuda"),
         "flip_alternating": (torch.arange(n, device="cuda") % 2).to(torch.uint8)}
flush = torch.empty(640 << 20, dtype=torch.uint8, device="cuda")


def plain(which):
    return lambda: L.check(which.mvldm_crop_shim(src.data_ptr(), 1, dst.data_ptr(), n, h, w, shape[0], shape[1], ws.data_ptr(), need, None, ops.stream()))


def flagged(f):
    return lambda: L.check(lib.mvldm_crop_shim_flip(src.data_ptr(), 1, dst.data_ptr(), n, h, w, shape[0], shape[1], None if f is None else f.data_ptr(),
                                                    ws.data_ptr(), need, None, ops.stream()))


variants = {"shim": plain(lib), "flip_null": flagged(None), **{k: flagged(v) for k, v in flags.items()}}
if "--parent-lib" in sys.argv:
    parent = C.CDLL(sys.argv[sys.argv.index("--parent-lib") + 1])
    parent.mvldm_crop_shim.restype = C.c_int
    parent.mvldm_crop_shim.argtypes = lib.mvldm_crop_shim.argtypes
    variants = {"parent_shim": plain(parent), **variants}

# the same bytes first: every unflagged variant equals the parent's / this build's shim, the flagged ones the shim of the reversed source
variants["shim"]()
base = dst.clone()
variants["flip_all"]()
mirrored = dst.clone()
assert torch.equal(mirrored, ops.crop_shim(src.flip(2).contiguous(), shape)[0]) and not torch.equal(mirrored, base)
for name in ("parent_shim", "flip_null", "flip_zero"):
    if name in variants:
        dst.zero_()
        variants[name]()
        assert torch.equal(dst, base), name
variants["flip_alternating"]()
assert torch.equal(dst[0::2], base[0::2]) and torch.equal(dst[1::2], mirrored[1::2])


def event_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


for fn in variants.values():
    event_us(fn, 20)
hot, cold = {k: [] for k in variants}, {k: [] for k in variants}
for _ in range(ROUNDS):
    for name, fn in variants.items():
        hot[name].append(event_us(fn, HOT_CALLS))
for _ in range(ROUNDS):
    for name, fn in variants.items():
        one = []
        for _ in range(COLD_CALLS):
            flush.fill_(1)
            one.append(event_us(fn, 1))
        cold[name].append(sorted(one)[COLD_CALLS // 2])
stats = lambda v: {"median": round(sorted(v)[len(v) // 2], 3), "min": round(min(v), 3), "max": round(max(v), 3)}
rec = {"n": n, "source": [h, w], "shape": list(shape), "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
       "note": f"us per call of n uint8 images; {ROUNDS} rounds alternating the variants; hot = a window of {HOT_CALLS} back-to-back calls, cold = the median "
               f"of {COLD_CALLS} single calls each behind a 640 MB fill; outputs checked equal before timing",
       "hot_us_per_call": {k: stats(v) for k, v in hot.items()}, "cold_us_per_call": {k: stats(v) for k, v in cold.items()}}
for k in variants:
    print(f"{k:18s} hot {rec['hot_us_per_call'][k]}  cold {rec['cold_us_per_call'][k]}")
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(rec, f, indent=1)
print(json.dumps(rec))
