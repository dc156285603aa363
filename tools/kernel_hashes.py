#!/usr/bin/env python3
"""Hash the device code of every kernel of the library, so that a refactor can show it moved code without changing it.

    python tools/kernel_hashes.py -o after.json                    # this tree, product flags
    python tools/kernel_hashes.py --experiments -o after_exp.json  # with -DMVLDM_EXPERIMENTS
    python tools/kernel_hashes.py --csrc OTHER/mv_ldm_amd/csrc -o before.json
    python tools/kernel_hashes.py --compare before.json after.json

Every csrc/*.hip is compiled to gfx950 assembly (device only).  A function is the text from `.type NAME,@function` to its
`.Lfunc_endN` plus its `.amdhsa_kernel` block; the per-file function index in labels is dropped, so a kernel may change
files (and its position in one) and keep its hash.
"""
import argparse
import hashlib
import json
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from mv_ldm_amd._build import FLAGS, _hipcc  # noqa: E402

LABEL = re.compile(r"(\.L[A-Za-z_]+?|BB)\d+(_\d+)")          # .LBB3_7 / BB3_7 / .LJTI3_0 -> .LBB_7 / BB_7 / .LJTI_0
FUNC_END = re.compile(r"\.L(func_begin|func_end|post_getpc)\d+")      # per-file counters


def functions(asm: str) -> dict:
    out, cur, name = {}, None, None
    for line in asm.splitlines():
        if "__hip_cuid_" in line:
            continue
        line = FUNC_END.sub(r".L\1", LABEL.sub(r"\1\2", line))
        line = " ".join(line.split())      # (the comment column moves with the width of the function index)
        m = re.match(r"\s*\.type\s+(\S+),@function", line) or re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m and cur is None:
            name, cur = m.group(1), []
        if cur is not None:
            cur.append(line)
            if re.match(r"\s*\.size\s+" + re.escape(name) + r",", line) or ".end_amdhsa_kernel" in line:
                out.setdefault(name, []).extend(cur)
                cur = None
    return {k: hashlib.sha256("\n".join(v).encode()).hexdigest() for k, v in out.items()}


def hash_tree(csrc: Path, experiments: bool) -> dict:
    flags = [f for f in FLAGS if not f.startswith("-Rpass")] + (["-DMVLDM_EXPERIMENTS"] if experiments else [])
    merged = {}
    with tempfile.TemporaryDirectory() as tmp:
        def one(src):
            s = Path(tmp) / (src.stem + ".s")
            r = subprocess.run([_hipcc(), *flags, "-x", "hip", "--cuda-device-only", "-S", str(src), "-o", str(s)], capture_output=True, text=True)
            if r.returncode:
                raise SystemExit(f"hipcc failed on {src.name}:\n{r.stderr}")
            return src.name, functions(s.read_text())
        with ThreadPoolExecutor(max_workers=8) as ex:
            for fname, fns in ex.map(one, sorted(csrc.glob("*.hip"))):
                for k, h in fns.items():
                    if k in merged:
                        raise SystemExit(f"{k} is compiled twice (second time in {fname})")
                    merged[k] = h
    return merged


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", type=Path, default=Path(__file__).resolve().parent.parent / "mv_ldm_amd" / "csrc")
    ap.add_argument("--experiments", action="store_true")
    ap.add_argument("-o", "--out", type=Path)
    ap.add_argument("--compare", nargs=2, type=Path)
    a = ap.parse_args()
    if a.compare:
        x, y = (json.loads(q.read_text()) for q in a.compare)
        bad = sorted(k for k in x.keys() | y.keys() if x.get(k) != y.get(k))
        print(f"{len(x)} / {len(y)} functions, {len(bad)} differ")
        for k in bad:
            print(("changed " if k in x and k in y else "only in " + str(a.compare[k not in x])) + " " + k)
        sys.exit(1 if bad else 0)
    text = json.dumps(hash_tree(a.csrc, a.experiments), indent=0, sort_keys=True)
    a.out.write_text(text) if a.out else print(text)
