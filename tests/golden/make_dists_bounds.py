#!/usr/bin/env python3
"""Writes tests/golden/dists_cpu_emulation.json: what CPU arithmetic alone does to the DISTS score on exactly the inputs of
tests/test_hip_dists.py's whole-metric parity test (tests/dists_ref.py CASES, seeded random weights), so that the test's bounds come
from the CPU and never from the kernels under test.

    python tests/golden/make_dists_bounds.py

Per pair kind: the worst relative error |got - want| / want against the fp64 restatement (the package's `1 - sum` form) of
  * "float32": the trunk in fp32 (another summation order, fp32 round-off through 13 layers), statistics and fold in fp64, direct form,
  * "float16" / "bfloat16": weights and every stored activation rounded to that type, arithmetic in fp32, statistics in fp64.
"want" holds the fp64 scores of every case (the GPU test recomputes the small ones and takes the 256 x 256 one from here).
CPU only, a few minutes.
"""
import json
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import dists_ref as R  # noqa: E402

EMULATIONS = {"float32": dict(dtype=torch.float32), "float16": dict(emulate=torch.float16), "bfloat16": dict(emulate=torch.bfloat16)}


def main():
    sd = R.make_weights(R.WEIGHT_SEED)
    worst = {name: {} for name in EMULATIONS}
    want_all = {}
    for n, h, w in R.CASES:
        for kind in R.KINDS:
            if kind == "identical":
                continue
            gt, pred = R.make_pair(kind, n, h, w, seed=R.case_seed(n, h, w))
            want = R.dists(gt, pred, sd)
            want_all[R.case_key(kind, n, h, w)] = want.tolist()
            for name, kw in EMULATIONS.items():
                if name != "float32" and kind not in R.KINDS_16BIT:
                    continue
                got = R.dists(gt, pred, sd, **kw)
                e = float(((got - want).abs() / want).max())
                worst[name][kind] = max(e, worst[name].get(kind, 0.0))
                print(f"{n}x3x{h}x{w} {kind} {name}: rel err {e:.3e} (value {float(want.mean()):.4e})", flush=True)
    out = {"weights_seed": R.WEIGHT_SEED, "cases": [list(c) for c in R.CASES], "worst_rel_err": worst, "want": want_all}
    (HERE / "dists_cpu_emulation.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(json.dumps(worst, indent=1))


if __name__ == "__main__":
    main()
