#!/usr/bin/env python3
"""Records what the four metric networks must keep through a refactor of their shared code:

    metric_state_keys.json     per module, the ordered `state_dict()` keys with their shapes
    metric_reset_sha256.json   per module, sha256 over the bytes of every `state_dict()` tensor, in order, after `reset_parameters(seed=7)`

    python tests/golden/make_metric_nets_golden.py --tree CHECKOUT --commit HASH

The committed files were recorded from a checkout of commit 4caf6c456d72 ("Train on real scenes: RE10K training loader, samplers, flagged
flip"), the parent of the commit that introduced `mv_ldm_amd/_metric_nets.py`: LPIPS, DISTS, FrechetInceptionDistance and InceptionPool3
were four separate files there.  Both files name the commit they were run on.  tests/test_metric_nets_cpu.py compares the tree against them;
run this script on the tree itself only to record a change that is meant (a new key, another init).  No GPU is needed.
"""
import argparse
import hashlib
import json
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
SEED = 7


def modules():
    from mv_ldm_amd.cleanfid import InceptionPool3
    from mv_ldm_amd.dists import DISTS
    from mv_ldm_amd.fid import FrechetInceptionDistance
    from mv_ldm_amd.lpips import LPIPS
    return {cls.__name__: cls(allow_random_init=True) for cls in (LPIPS, DISTS, FrechetInceptionDistance, InceptionPool3)}


def keys_and_shapes(module) -> list:
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def reset_sha256(module, seed: int = SEED) -> str:
    module.reset_parameters(seed=seed)
    h = hashlib.sha256()
    for v in module.state_dict().values():
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", type=Path, default=HERE.parent.parent, help="the checkout whose mv_ldm_amd is recorded")
    ap.add_argument("--commit", default=None, help="its commit (default: git rev-parse HEAD in --tree)")
    ap.add_argument("--out", type=Path, default=HERE)
    a = ap.parse_args()
    sys.path.insert(0, str(a.tree.resolve()))
    commit = a.commit or subprocess.run(["git", "-C", str(a.tree), "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    mods = modules()
    (a.out / "metric_state_keys.json").write_text(json.dumps({"commit": commit, "modules": {n: keys_and_shapes(m) for n, m in mods.items()}}, indent=0))
    (a.out / "metric_reset_sha256.json").write_text(json.dumps({"commit": commit, "seed": SEED, "modules": {n: reset_sha256(m) for n, m in mods.items()}}, indent=1))
    print(f"recorded {sorted(mods)} of {commit} under {a.out}")
