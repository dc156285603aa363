#!/usr/bin/env python3
"""Dump every op descriptor of a few recorded plans, so that a refactor of the host code can show the plans did not change.

    python tools/plan_dump.py --cpu -o after_cpu.json                 # the plans tests/test_plan_build_cpu.py records (no GPU)
    python tools/plan_dump.py -o after.json                           # + one sampler plan and one TrainPlan (needs the GPU)
    python tools/plan_dump.py --cpu --tree OTHER_CHECKOUT -o before_cpu.json
    python tools/plan_dump.py --compare before.json after.json

Per op: name, kind, FLOPs, bytes and every field of its descriptor.  A pointer field holds the index of that pointer value's
first appearance in the plan (null stays null): pool reuse and view offsets are compared, addresses are not.  The GPU plans are
recorded with MVLDM_AUTOTUNE=0 MVLDM_TRAIN_AUTOTUNE=0 (rules only: nothing is timed, nothing runs but the weight packing).
"""
import argparse
import ctypes as C
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def member_of(L) -> dict:
    """op kind -> name of its member of the mvldm_op union (the lane markers carry none)"""
    names = dict(OP_IGEMM="igemm", OP_GROUPNORM="groupnorm", OP_LAYERNORM="layernorm", OP_ATTENTION="attention", OP_TIMESTEP_EMBED="temb",
                 OP_ELTWISE="eltwise", OP_DDIM_STEP="ddim", OP_DDIM_ADVANCE="advance", OP_NCHW_TO_NHWC="layout", OP_NHWC_TO_NCHW="layout",
                 OP_MEMCPY="memcpy_", OP_RAY_ENCODE="rays", OP_POSTERIOR_SAMPLE="posterior", OP_WGRAD="wgrad", OP_ATTENTION_BWD="attention_bwd",
                 OP_GROUPNORM_BWD="groupnorm_bwd", OP_LAYERNORM_BWD="layernorm_bwd", OP_COLSUM="colsum", OP_TRAIN_ELTWISE="train_eltwise",
                 OP_POOL2X2="resample", OP_ZERO_INSERT="resample", OP_ADD_NOISE="add_noise", OP_MSE_LOSS="mse", OP_FILL_ZERO="fill",
                 OP_GATHER_ROWS="gather", OP_ATTN_MERGE="attn_merge", OP_PAR_BEGIN=None, OP_PAR_NEXT=None, OP_PAR_END=None)
    return {getattr(L, k): v for k, v in names.items()}


def dump_plan(L, ops, meta) -> list:
    member, seen, out = member_of(L), {}, []
    for op, m in zip(ops, meta):
        fields = {}
        u = member[op.kind] and getattr(op.u, member[op.kind])
        for name, ctype in (u._fields_ if u else ()):
            v = getattr(u, name)
            if ctype is C.c_void_p:
                v = None if not v else seen.setdefault(v, len(seen))
            fields[name] = v
        out.append(dict(name=m.name, kind=int(op.kind), flops=float(m.flops), nbytes=float(m.bytes), desc=fields))
    return out


def cpu_plans(L) -> dict:
    """the plans of tests/test_plan_build_cpu.py, built the way its `cpu_record` fixture builds them"""
    import torch
    sys.path.append(str(ROOT / "tests"))
    import test_plan_build_cpu as T
    from mv_ldm_amd import modules, mvunet, ops, plan, runtime, vae
    saved = [(ops, "pack_weight", ops.pack_weight)] + [(mod, "require_gpu", mod.require_gpu) for mod in (modules, mvunet, runtime, vae)
                                                       if hasattr(mod, "require_gpu")]
    ops.pack_weight = T.fake_pack_weight
    for mod, name, _ in saved[1:]:
        setattr(mod, name, lambda t: None)
    L.load()
    out = {}
    try:
        _, b, _ = T.build_unet_plan(5, [3, 2], 8, widths=(64, 128, 256, 256))
        out["cpu/unet"] = dump_plan(L, b.ops, b.meta)
        v = vae.AutoencoderKL.from_pretrained("x")
        for name, emit, shape in (("decoder", v.decoder.emit, (1, 32, 32, 8)), ("encoder", v.encoder.emit, (1, 256, 256, 8))):
            b = plan.Builder("cpu", torch.bfloat16, record=True, splitk_ws_bytes=1 << 20)
            emit(b, torch.zeros(*shape, dtype=torch.bfloat16))
            out[f"cpu/vae_{name}"] = dump_plan(L, b.ops, b.meta)
    finally:
        for mod, name, fn in saved:
            setattr(mod, name, fn)
    return out


def gpu_plans(L) -> dict:
    """one sampler plan (with its loader and context-prefix plans) and one TrainPlan of the small model tests/test_hip_train.py trains"""
    import numpy as np
    import torch
    import mv_ldm_amd
    from mv_ldm_amd import plan
    from mv_ldm_amd.mvunet import MultiViewUNet, MultiViewUNetCfg, UNet2DModelCfg
    from mv_ldm_amd.pipeline import MVLDMPipeline, SamplerCfg
    from mv_ldm_amd.scheduler import DDIMScheduler
    from mv_ldm_amd.train import MVLDMTrainer
    from mv_ldm_amd.vae import AutoencoderKL
    g = np.load(ROOT / "tests" / "golden" / "g9_training_step.npz", allow_pickle=False)
    widths = tuple(int(v) for v in g["widths"])
    over = dict(block_out_channels=widths, attention_head_dim=tuple(max(1, c // 64) for c in widths))
    den = MultiViewUNet(MultiViewUNetCfg(autoencoder=UNet2DModelCfg(block_out_channels=widths), pretrained_from="sd21",
                                         pretrained_overrides=over, allow_random_init=True), 11, 4).cuda()
    vae = AutoencoderKL.from_pretrained("x", config_overrides=dict(block_out_channels=tuple(int(v) for v in g["vae_widths"]), layers_per_block=1),
                                        allow_random_init=True).cuda()
    b, views, _, h, w = g["c0_image"].shape
    plan.Plan.capture = lambda self: None          # (a dump records; it does not need the graph)
    dtype = torch.bfloat16
    mv_ldm_amd.set_compute_dtype(dtype)
    out = {}
    pipe = MVLDMPipeline(den, vae, DDIMScheduler(clip_sample=False), SamplerCfg(True, 3.0, 3))
    pipe.set_timesteps(3)
    hl, wl = h // pipe.latent_downscale, w // pipe.latent_downscale
    st = pipe._compile(int(b), 2, int(views) - 2, hl, wl, dtype, 3)
    for name in ("plan", "loader", "const_plan"):
        if st[name] is not None:
            out[f"gpu/sampler/{name}"] = dump_plan(L, st[name].ops, st[name].meta)
    tr = MVLDMTrainer(den, vae, DDIMScheduler(clip_sample=False), dtype=dtype)
    tp = tr.plan_for(int(b), 2, int(views) - 2, hl, wl)
    out["gpu/train"] = dump_plan(L, tp.plan.ops, tp.plan.meta)
    torch.cuda.synchronize()
    return out


def compare(a: dict, b: dict) -> int:
    bad = 0
    for name in sorted(a.keys() | b.keys()):
        x, y = a.get(name), b.get(name)
        if x is None or y is None:
            print(f"{name}: only in {'the first' if y is None else 'the second'} dump")
            bad += 1
            continue
        diff = [i for i in range(max(len(x), len(y))) if i >= len(x) or i >= len(y) or x[i] != y[i]]
        print(f"{name}: {len(x)} / {len(y)} ops, {len(diff)} differ")
        for i in diff[:8]:
            p, q = (x[i] if i < len(x) else None), (y[i] if i < len(y) else None)
            if p is None or q is None:
                print(f"  op {i}: only in one dump: {(p or q)['name']}")
                continue
            what = [k for k in ("name", "kind", "flops", "nbytes") if p[k] != q[k]] + \
                   [f"desc.{k}: {p['desc'].get(k)} -> {q['desc'].get(k)}" for k in sorted(p["desc"].keys() | q["desc"].keys()) if p["desc"].get(k) != q["desc"].get(k)]
            print(f"  op {i} {p['name']}: " + "; ".join(map(str, what)))
        bad += len(diff)
    return bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true", help="only the plans that record without a GPU")
    ap.add_argument("--tree", type=Path, default=ROOT, help="import the package from this checkout")
    ap.add_argument("-o", "--out", type=Path)
    ap.add_argument("--compare", nargs=2, type=Path)
    a = ap.parse_args()
    if a.compare:
        sys.exit(1 if compare(*(json.loads(p.read_text()) for p in a.compare)) else 0)
    os.environ["MVLDM_AUTOTUNE"] = os.environ["MVLDM_TRAIN_AUTOTUNE"] = "0"
    sys.path.insert(0, str(a.tree.resolve()))
    from mv_ldm_amd import _lib
    plans = cpu_plans(_lib)
    if not a.cpu:
        plans.update(gpu_plans(_lib))
    print("; ".join(f"{k}: {len(v)} ops" for k, v in plans.items()), file=sys.stderr)
    text = json.dumps(plans, indent=0)
    a.out.write_text(text) if a.out else print(text)
