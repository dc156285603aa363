#!/usr/bin/env python3
"""Writes tests/golden/fid_cpu_emulation.json: what CPU arithmetic alone does to the FID score on exactly the inputs of
tests/test_hip_fid.py (tests/fid_ref.py CASES and synthetic_cases, seeded random weights), so that the tests' bounds come from the CPU
and never from the kernels under test.

    python tests/golden/make_fid_bounds.py

Every error is |got - want| / (|mu1 - mu2|^2 + tr Sigma1 + tr Sigma2) with the scale taken from the fp64 states: the score itself can
be ~ 0.  Per kind of pair, the worst error against the fp64 restatement (`frechet_sym` of the fp64 features) of the device's route
(`jacobi_emulation`) on the features of
  * "float32": the stem in fp32 (another summation order, fp32 round-off through three layers), folded BatchNorm,
  * "float16" / "bfloat16": the folded weights and every stored activation rounded to that type, arithmetic in fp32.
"want" / "scale": the fp64 score and scale of every case (the GPU test recomputes the small ones and takes the 256 x 256 one from here).
"jacobi": per class of synthetic state pair (full rank / rank-deficient) the worst error of `jacobi_emulation` against `frechet_sym`
(against the analytic value where there is one), and each case's own.  "sym_vs_pkg": |frechet_sym - frechet_pkg| of every case, the
distance between the symmetric form and the package's `eigvals` route.  CPU only, a few minutes.
"""
import json
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import fid_ref as R  # noqa: E402

EMULATIONS = {"float32": dict(dtype=torch.float32), "float16": dict(emulate=torch.float16), "bfloat16": dict(emulate=torch.bfloat16)}


def synthetic():
    worst, each, sym_pkg = {"full": 0.0, "deficient": 0.0}, {}, {}
    for name, (cls, s1, s2, c) in R.synthetic_cases().items():
        sc = R.scale(s1, s2)
        want = R.frechet_sym(s1, s2) if c is None else sc - 2 * c
        got, info = R.jacobi_emulation(s1, s2)
        assert info[4] == 0, (name, info)
        each[name] = {"class": cls, "err": abs(got - want) / sc, "want": want, "scale": sc, "sweeps": [info[0], info[2]]}
        worst[cls] = max(worst[cls], each[name]["err"])
        sym_pkg[f"synthetic/{name}"] = abs(R.frechet_sym(s1, s2) - R.frechet_pkg(s1, s2)) / sc
        print(f"{name} ({cls}): jacobi err {each[name]['err']:.3e}, sym - pkg {sym_pkg[f'synthetic/{name}']:.3e}, sweeps {info[0]} + {info[2]}", flush=True)
    return worst, each, sym_pkg


def main():
    sd = R.make_weights(R.WEIGHT_SEED)
    jac_worst, jac_each, sym_pkg = synthetic()
    worst = {name: {} for name in EMULATIONS}
    want_all, scale_all = {}, {}
    for n_real, n_fake, h, w in R.CASES:
        for pair in R.PAIRS:
            real, fake = R.make_sets(pair, n_real, n_fake, h, w, seed=R.case_seed(n_real, n_fake, h, w))
            key = R.case_key(pair, n_real, n_fake, h, w)
            want, s1, s2 = R.fid(real, fake, sd)
            sc = R.scale(s1, s2)
            want_all[key], scale_all[key] = want, sc
            sym_pkg[key] = abs(want - R.frechet_pkg(s1, s2)) / sc
            jac_worst["deficient"] = max(jac_worst["deficient"], abs(R.jacobi_emulation(s1, s2)[0] - want) / sc)
            for name, kw in EMULATIONS.items():
                got, _, _ = R.fid(real, fake, sd, route=lambda a, b: R.jacobi_emulation(a, b)[0], **kw)
                e = abs(got - want) / sc
                worst[name][pair] = max(e, worst[name].get(pair, 0.0))
                print(f"{key} {name}: err {e:.3e} (fid {want:.4e}, scale {sc:.4e}, sym - pkg {sym_pkg[key]:.2e})", flush=True)
    out = {"weights_seed": R.WEIGHT_SEED, "cases": [list(c) for c in R.CASES], "worst_err": worst, "want": want_all, "scale": scale_all,
           "jacobi": {"worst": jac_worst, "cases": jac_each}, "sym_vs_pkg": sym_pkg}
    (HERE / "fid_cpu_emulation.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(json.dumps({"worst_err": worst, "jacobi": jac_worst, "sym_vs_pkg_max": max(sym_pkg.values())}, indent=1))


if __name__ == "__main__":
    main()
