"""Writes tests/golden/cleanfid_cpu_emulation.json and tests/golden/cleanfid_features.npz: what the bounds of tests/test_hip_cleanfid.py
come from, computed on the CPU on exactly that test's inputs (tests/cleanfid_ref.py), never from the kernels.

    python tests/golden/make_cleanfid_bounds.py          (about a quarter of an hour on 8 cores: fp64 Inception-v3 and scipy's sqrtm at 2048)

  want / scale      the fp64 restatement's score and |mu1 - mu2|^2 + tr Sigma1 + tr Sigma2 of every case; the score in its factored form
                    (`frechet_factored`: singular values of an n1 x n2 matrix), which has no null-space round-off; sym_vs_factored records
                    how far numpy's eigh-twice route is from it (1.1e-6 of the scale: more than the f32 bound)
  worst_err         per dtype and kind of pair: |emulation - want| / scale, the emulation being the network in fp32, or folded weights and
                    every stored activation rounded to f16 / bf16 with fp32 arithmetic
  feature_err       per dtype: the worst |f_emulation - f| of a feature, relative to the RMS of that image's feature vector
  map_err           per dtype and map: the same for every entry of the maps `features(return_maps=...)` returns
  conv_err          per dtype: the same for the unit cases of the unfolded convolutions
  sym_vs_pkg        per case: |symmetric route - scipy sqrtm route| / scale, the metric's own ambiguity
  solve             the numpy emulation of the device's one-sided Jacobi against `frechet_sym` (or the analytic value) at d = 128 and 192, per
                    class of states; at d = 2048 the expectation and sym_vs_pkg only
cleanfid_features.npz: the fp64 features and 512 seeded entries of each map for the `other` pair of each case (the restatement takes
seconds per image: the GPU test reads them)."""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import cleanfid_ref as R      # noqa: E402

KINDS = {"float32": (torch.float32, None), "float16": (torch.float32, torch.float16), "bfloat16": (torch.float32, torch.bfloat16)}


def rel_rms(got: torch.Tensor, want: torch.Tensor) -> float:
    """the worst entry error of each image, relative to the RMS of that image's entries"""
    n = want.shape[0]
    g, w = got.double().reshape(n, -1), want.double().reshape(n, -1)
    return float(((g - w).abs().amax(1) / w.pow(2).mean(1).sqrt()).max())


def alive(name: str, t: torch.Tensor):
    """a dead network tests nothing: spread within [1e-3, 1e3] x the mean magnitude, fewer than half the entries exactly 0"""
    n = t.shape[0]
    flat = t.double().reshape(n, -1)
    ratio = flat.std(1) / flat.abs().mean(1)
    assert bool(((ratio >= 1e-3) & (ratio <= 1e3)).all()), (name, ratio)
    if name == "features":
        assert bool(((flat == 0).double().mean(1) < 0.5).all()), (name, (flat == 0).double().mean(1))


if __name__ == "__main__":
    t0 = time.time()
    sd = R.make_weights()
    rec = {"want": {}, "scale": {}, "sym_vs_pkg": {}, "sym_vs_factored": {}, "worst_err": {k: {p: 0.0 for p in R.PAIRS} for k in KINDS},
           "feature_err": {k: 0.0 for k in KINDS}, "map_err": {k: {m: 0.0 for m in R.MAPS} for k in KINDS}, "conv_err": {k: 0.0 for k in KINDS}}
    cache, npz = {}, {}

    def feats(imgs, kind):
        key = (kind, imgs.shape, hash(imgs.numpy().tobytes()))
        if key not in cache:
            dtype, emulate = (torch.float64, None) if kind == "float64" else KINDS[kind]
            cache[key] = R.features(imgs, sd, dtype, emulate, maps=R.MAPS)
            print(f"  {kind} {tuple(imgs.shape)}: {time.time() - t0:.0f} s", flush=True)
        return cache[key]

    for case in R.CASES:
        for pair in R.PAIRS:
            key = R.case_key(pair, *case)
            real, fake = R.case_sets(pair, *case)
            (fr, mr), (ff, mf) = feats(real, "float64"), feats(fake, "float64")
            for name, t in [("features", torch.cat([fr, ff]))] + [(m, torch.cat([mr[m], mf[m]])) for m in R.MAPS]:
                alive(name, t)
            s1, s2 = R.state(fr), R.state(ff)
            want, sc = R.frechet_factored(fr, ff), R.scale(s1, s2)
            sym = R.frechet_sym(s1, s2)
            rec["want"][key], rec["scale"][key] = want, sc
            rec["sym_vs_factored"][key] = abs(sym - want) / sc
            rec["sym_vs_pkg"][key] = abs(R.frechet_sqrtm(s1, s2) - sym) / sc
            print(f"{key}: fid {want:.6e} of scale {sc:.4e}; sym vs pkg {rec['sym_vs_pkg'][key]:.2e}; {time.time() - t0:.0f} s", flush=True)
            if pair == "other":
                npz[f"{key}/real"], npz[f"{key}/fake"] = fr.numpy(), ff.numpy()
                for m in R.MAPS:
                    full = torch.cat([mr[m], mf[m]])
                    npz[f"{key}/{m}"] = full.reshape(full.shape[0], -1)[:, R.map_sample(m, full.shape[1:])].numpy()
            for kind in KINDS:
                (er, emr), (ef, emf) = feats(real, kind), feats(fake, kind)
                got = R.frechet_factored(er, ef)
                rec["worst_err"][kind][pair] = max(rec["worst_err"][kind][pair], abs(got - want) / sc)
                rec["feature_err"][kind] = max(rec["feature_err"][kind], rel_rms(torch.cat([er, ef]), torch.cat([fr, ff])))
                for m in R.MAPS:
                    rec["map_err"][kind][m] = max(rec["map_err"][kind][m], rel_rms(torch.cat([emr[m], emf[m]]), torch.cat([mr[m], mf[m]])))
    for k, pad in R.CONV_KERNELS:
        for hw in R.CONV_MAPS[k]:
            x, w, b = R.conv_case(k, hw)
            want = R.conv_want(x, w, b, pad)
            for kind, (dtype, emulate) in KINDS.items():
                rec["conv_err"][kind] = max(rec["conv_err"][kind], rel_rms(R.conv_want(x, w, b, pad, emulate, dtype), want))
    solve = {"cases": {}, "worst": {}}
    for d in (128, 192, 2048):
        worst = {}
        for name, (cls, s1, s2, c) in R.synthetic_cases(d).items():
            sc = R.scale(s1, s2)
            want = R.frechet_sym(s1, s2) if c is None else sc - 2 * c
            row = {"class": cls, "d": d, "want": want, "scale": sc, "sym_vs_pkg": abs(R.frechet_sqrtm(s1, s2) - want) / sc}
            if d <= 192:
                got, info = R.hestenes_emulation(s1, s2)
                assert info[4] == 0, (name, d, info)
                row.update(emu_err=abs(got - want) / sc, sweeps=[info[0], info[2]])
                worst[cls] = max(worst.get(cls, 0.0), row["emu_err"])
            solve["cases"][f"{name}/{d}"] = row
            print(f"solve {name}/{d}: {row}; {time.time() - t0:.0f} s", flush=True)
        if worst:
            solve["worst"][str(d)] = worst
    rec["solve"] = solve
    (HERE / "cleanfid_cpu_emulation.json").write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")
    np.savez_compressed(HERE / "cleanfid_features.npz", **npz)
    print("written;", (HERE / "cleanfid_features.npz").stat().st_size, "bytes of features;", f"{time.time() - t0:.0f} s")
