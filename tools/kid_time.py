"""time Clean-KID on the device (mv_ldm_amd/cleanfid.py, csrc/kid.hip):  python tools/kid_time.py [n=1000] [d=2048] [subsets=100] [--out FILE]
at the package's default size (n1 = n2 = 1000 features of width 2048, 100 subsets of 1000) on random non-negative features:
  * the device work of `kernel_distance` (`ops.kid_compute`; the draw of the subsets is host work and is timed apart);
  * beside it, on the same device, the straightforward route -- torch fp64 `x @ x.T` per subset, the estimator as the package writes it.
    That route is a yardstick of this tool only; it is never on the product path.
One warm-up and five runs each between device events; the median and the spread are printed and, with --out, written to a text file."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mv_ldm_amd import ops
from mv_ldm_amd.cleanfid import kid_subsets

args = [int(a) for a in sys.argv[1:] if a.isdigit()]
n, d, S = (args + [1000, 2048, 100][len(args):])[:3]
LIMIT_S = 240.0                                 # the whole tool gives up past this
t_start = time.time()

g = torch.Generator("cuda").manual_seed(0)
w = torch.linspace(0.2, 2.0, d, dtype=torch.float64, device="cuda")
f1 = torch.rand(n, d, dtype=torch.float64, device="cuda", generator=g) * w
f2 = torch.rand(n, d, dtype=torch.float64, device="cuda", generator=g) * w + 0.05
t0 = time.time()
idx1, idx2 = kid_subsets(n, n, S, 1000, seed=0)
draw_ms = (time.time() - t0) * 1e3
m = idx1.shape[1]
idx1, idx2 = idx1.cuda(), idx2.cuda()
out = torch.empty(1, device="cuda")
info = torch.empty(ops.KID_INFO, dtype=torch.float64, device="cuda")
ws = torch.empty(ops.kid_workspace_bytes(m, S), dtype=torch.uint8, device="cuda")


def kernel():
    ops.kid_compute(f1, f2, idx1, idx2, out, info, None, ws)
    return out


def torch_route():
    t = torch.zeros((), dtype=torch.float64, device="cuda")
    i1, i2 = idx1.long(), idx2.long()
    for s in range(S):
        x, y = f2[i2[s]], f1[i1[s]]
        a = (x @ x.T / d + 1) ** 3 + (y @ y.T / d + 1) ** 3
        b = (x @ y.T / d + 1) ** 3
        t += (a.sum() - a.diagonal().sum()) / (m - 1) - b.sum() * 2 / m
    return t / S / m


def timed(fn, runs=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        if time.time() - t_start > LIMIT_S:
            raise SystemExit(f"kid_time: over {LIMIT_S:.0f} s, giving up")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms), float(r)


k_ms, k_val = timed(kernel)
t_ms, t_val = timed(torch_route)
flops = 3 * 2.0 * m * m * d * S
T = (m + 63) // 64
kflops = (T * (T + 1) + T * T) * 64 * 64 * 2.0 * d * S          # the tiles it launches, padding included
lines = [f"Clean-KID, n1 = n2 = {n}, d = {d}, {S} subsets of m = {m}; fp64; one warm-up, five runs between device events",
         f"kernel_distance (csrc/kid.hip, fp64 MFMA, tile pairs a <= b): median {k_ms[2]:.2f} ms (min {k_ms[0]:.2f}, max {k_ms[-1]:.2f}); "
         f"{kflops / (k_ms[2] * 1e-3) / 1e12:.2f} Tflop/s over the tiles it launches",
         f"torch fp64 x @ x.T per subset (three full products, m x m matrices in memory): median {t_ms[2]:.2f} ms (min {t_ms[0]:.2f}, max {t_ms[-1]:.2f}); "
         f"{flops / (t_ms[2] * 1e-3) / 1e12:.2f} Tflop/s",
         f"kid: kernel {float(info[0]):.12e}, torch route {t_val:.12e}; drawing the subsets on the host {draw_ms:.1f} ms"]
print("\n".join(lines))
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write("\n".join(lines) + "\n")
