"""Image quality of sampled views on the device: the counterpart of `src/evaluation/metrics.py` (`compute_psnr` :17-24,
`compute_ssim` :58-73) and of `metric_computer.test_step`, which walks the PNG tree `test_step` wrote.

The reference pulls every image to the host and runs skimage one image at a time; here both scores of a whole batch come from
one launch of `csrc/metrics.hip` (`ops.image_metrics`).  LPIPS (`compute_lpips`, :43-54) runs on the device too -- its VGG-16 trunk
through the implicit GEMM, the distance in `csrc/lpips.hip` (`mv_ldm_amd.lpips.LPIPS`) -- with the weight files the user brings: none
ships with the package and none is fetched.  DISTS (`compute_dists`, :27-40) runs the same trunk with L2 pooling and per-channel
statistics (`csrc/dists.hip`, `mv_ldm_amd.dists.DISTS`), again with the user's files.  FID (`metric_computer.py:22,65-68`:
`FrechetInceptionDistance(feature=64, normalize=True)`, one value per scene) runs the three convolutions of the Inception-v3 stem through
the same kernels and the Frechet distance in `csrc/fid.hip` (`mv_ldm_amd.fid.FrechetInceptionDistance`), with the user's Inception file.

    python -m mv_ldm_amd.metrics --pred DIR --gt DIR [--json OUT] [--lpips VGG.pth [--lpips-lin LIN.pth]]
                                 [--dists VGG_OR_FULL.pth [--dists-weights WEIGHTS.pt]] [--fid INCEPTION.pth]

pairs `DIR/<scene>/color/<index>.png` of the two trees by scene and frame index and prints per-scene and overall means.
`--lpips`: a full `lpips.LPIPS(net="vgg").state_dict()`, or torchvision's VGG-16 with the package's `vgg.pth` as `--lpips-lin`.
`--dists`: a full `DISTS_pytorch.DISTS().state_dict()`, or torchvision's VGG-16 with the package's `weights.pt` as `--dists-weights`.
`--fid`: torch-fidelity's `pt_inception` state dict, or a torchmetrics FID state dict; adds one `fid` per scene (scenes of 2 frames or more).
"""
from __future__ import annotations

import argparse
import json
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops


def image_metrics(ground_truth: torch.Tensor, predicted: torch.Tensor, use_sample_covariance: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(psnr, ssim) of `[batch, c, h, w]` -> `[batch]`, or of `[b, v, c, h, w]` -> `[b, v]`, fp32 on the inputs' device, one launch"""
    if ground_truth.shape != predicted.shape:
        raise ValueError(f"ground truth {tuple(ground_truth.shape)} against prediction {tuple(predicted.shape)}")
    if ground_truth.dim() not in (4, 5):
        raise ValueError(f"expected [batch, c, h, w] or [b, v, c, h, w], got {tuple(ground_truth.shape)}")
    if not (ground_truth.is_contiguous() and predicted.is_contiguous()):
        raise ValueError("image_metrics: inputs must be contiguous (call .contiguous() first)")
    lead = ground_truth.shape[:-3]
    flat = lambda t: t.reshape(-1, *t.shape[-3:])
    psnr, ssim = ops.image_metrics(flat(predicted), flat(ground_truth), use_sample_covariance)
    return psnr.reshape(lead), ssim.reshape(lead)


def compute_psnr(ground_truth: torch.Tensor, predicted: torch.Tensor) -> torch.Tensor:
    """src/evaluation/metrics.py:17-24: both clipped to [0, 1], -10 log10 of the mean squared difference; `+inf` for identical images"""
    return image_metrics(ground_truth, predicted)[0]


def compute_ssim(ground_truth: torch.Tensor, predicted: torch.Tensor, use_sample_covariance: bool = True) -> torch.Tensor:
    """src/evaluation/metrics.py:58-73: skimage's Gaussian-window SSIM (win_size 11, data_range 1.0, not clipped), mean over channels.
    `use_sample_covariance` is skimage's default `True` (variances scaled by 121 / 120): DESIGN.md §5, "parity unpinned"."""
    return image_metrics(ground_truth, predicted, use_sample_covariance)[1]


def compute_lpips(ground_truth: torch.Tensor, predicted: torch.Tensor, model) -> torch.Tensor:
    """src/evaluation/metrics.py:43-54: `model.forward(ground_truth, predicted, normalize=True)[:, 0, 0, 0]` with `model` an
    `mv_ldm_amd.lpips.LPIPS` on the inputs' device; `[batch, 3, h, w]` -> `[batch]`, or `[b, v, 3, h, w]` -> `[b, v]`, fp32"""
    if ground_truth.shape != predicted.shape:
        raise ValueError(f"ground truth {tuple(ground_truth.shape)} against prediction {tuple(predicted.shape)}")
    if ground_truth.dim() not in (4, 5):
        raise ValueError(f"expected [batch, c, h, w] or [b, v, c, h, w], got {tuple(ground_truth.shape)}")
    if not (ground_truth.is_contiguous() and predicted.is_contiguous()):
        raise ValueError("compute_lpips: inputs must be contiguous (call .contiguous() first)")
    lead = ground_truth.shape[:-3]
    flat = lambda t: t.reshape(-1, *t.shape[-3:])
    value = model(flat(ground_truth), flat(predicted), normalize=True)
    return value[:, 0, 0, 0].reshape(lead)


def load_lpips(weights, lin=None, device="cuda", dtype: torch.dtype = torch.float32):
    """the `--lpips VGG.pth [--lpips-lin LIN.pth]` of the command lines: an `LPIPS` with the user's weights on `device`"""
    from .lpips import LPIPS
    return LPIPS(net="vgg", weights=weights, lin=lin, dtype=dtype).to(device)


def compute_dists(ground_truth: torch.Tensor, predicted: torch.Tensor, model) -> torch.Tensor:
    """src/evaluation/metrics.py:27-40: `model.forward(ground_truth, predicted)` with `model` an `mv_ldm_amd.dists.DISTS` on the
    inputs' device; `[batch, 3, h, w]` -> `[batch]`, or `[b, v, 3, h, w]` -> `[b, v]`, fp32"""
    if ground_truth.shape != predicted.shape:
        raise ValueError(f"ground truth {tuple(ground_truth.shape)} against prediction {tuple(predicted.shape)}")
    if ground_truth.dim() not in (4, 5):
        raise ValueError(f"expected [batch, c, h, w] or [b, v, c, h, w], got {tuple(ground_truth.shape)}")
    if not (ground_truth.is_contiguous() and predicted.is_contiguous()):
        raise ValueError("compute_dists: inputs must be contiguous (call .contiguous() first)")
    lead = ground_truth.shape[:-3]
    flat = lambda t: t.reshape(-1, *t.shape[-3:])
    return model(flat(ground_truth), flat(predicted)).reshape(lead)


def load_dists(weights, alpha_beta=None, device="cuda", dtype: torch.dtype = torch.float32):
    """the `--dists VGG_OR_FULL.pth [--dists-weights WEIGHTS.pt]` of the command lines: a `DISTS` with the user's weights on `device`"""
    from .dists import DISTS
    return DISTS(weights=weights, alpha_beta=alpha_beta, dtype=dtype).to(device)


def compute_fid(ground_truth: torch.Tensor, predicted: torch.Tensor, model) -> torch.Tensor:
    """src/evaluation/metric_computer.py:65-68: `update(ground_truth, real=True)`, `update(predicted, real=False)`, `compute()`,
    `reset()` with `model` an `mv_ldm_amd.fid.FrechetInceptionDistance` on the inputs' device: one score per SET of views.
    `[v, 3, h, w]` -> 0-d, `[b, v, 3, h, w]` -> `[b]`, fp32.  Whatever the model had accumulated before is dropped."""
    if ground_truth.shape != predicted.shape:
        raise ValueError(f"ground truth {tuple(ground_truth.shape)} against prediction {tuple(predicted.shape)}")
    if ground_truth.dim() not in (4, 5):
        raise ValueError(f"expected [v, c, h, w] or [b, v, c, h, w], got {tuple(ground_truth.shape)}")
    if not (ground_truth.is_contiguous() and predicted.is_contiguous()):
        raise ValueError("compute_fid: inputs must be contiguous (call .contiguous() first)")

    def one(g, p):
        model.reset()
        model.update(g, real=True)
        model.update(p, real=False)
        value = model.compute()
        model.reset()
        return value

    if ground_truth.dim() == 4:
        return one(ground_truth, predicted)
    return torch.stack([one(ground_truth[i], predicted[i]) for i in range(ground_truth.shape[0])]) if ground_truth.shape[0] \
        else torch.empty(0, dtype=torch.float32, device=ground_truth.device)


def load_fid(weights, device="cuda", dtype: torch.dtype = torch.float32):
    """the `--fid INCEPTION.pth` of the command lines: a `FrechetInceptionDistance(feature=64, normalize=True)` with the user's weights on `device`"""
    from .fid import FrechetInceptionDistance
    return FrechetInceptionDistance(feature=64, normalize=True, weights=weights, dtype=dtype).to(device)


def metric_names(lpips=None, dists=None) -> Tuple[str, ...]:
    """the columns of a per-frame row scored with these networks: psnr, ssim, then lpips, then dists"""
    return ("psnr", "ssim") + (() if lpips is None else ("lpips",)) + (() if dists is None else ("dists",))


# ---- PNG trees ---------------------------------------------------------------------------------------------------
def scan_tree(root) -> Dict[str, Dict[int, Path]]:
    """{scene: {frame index: path}} of `root/<scene>/color/<index>.png`; the index is the file stem as an integer (`000012.png`
    and `12.png` are both frame 12), files whose stem is no integer are ignored"""
    out: Dict[str, Dict[int, Path]] = {}
    root = Path(root)
    if not root.is_dir():
        return out
    for scene in sorted(p for p in root.iterdir() if (p / "color").is_dir()):
        frames = {int(f.stem): f for f in sorted((scene / "color").glob("*.png")) if f.stem.isdigit()}
        if frames:
            out[scene.name] = frames
    return out


def pair_trees(pred: Dict[str, Dict[int, object]], gt: Dict[str, Dict[int, object]]):
    """Pair two `scan_tree` results by scene and frame index.  Returns (pairs, missing): pairs = {scene: [(index, pred item, gt
    item), ...]} in index order for every scene both sides have with at least one common frame; missing = a sorted list of
    ("scene" | "frame", scene, index | None, side that lacks it)."""
    pairs, missing = {}, []
    for scene in sorted(set(pred) | set(gt)):
        if scene not in pred or scene not in gt:
            missing.append(("scene", scene, None, "pred" if scene not in pred else "gt"))
            continue
        p, g = pred[scene], gt[scene]
        for i in sorted(set(p) ^ set(g)):
            missing.append(("frame", scene, i, "pred" if i not in p else "gt"))
        both = [(i, p[i], g[i]) for i in sorted(set(p) & set(g))]
        if both:
            pairs[scene] = both
    return pairs, missing


def summarize(per_frame: Dict[str, Dict[int, List[float]]], names: Optional[Sequence[str]] = None) -> dict:
    """{scene: {index: [psnr, ssim]}} -> the report: per-scene means, the overall mean over all frames.  Rows scored with an LPIPS
    network are [psnr, ssim, lpips]: the report then carries "lpips" next to "psnr" and "ssim".  `names`: the rows' columns, said
    outright (a run with a DISTS network passes them); without it they are inferred from the row length as above."""
    mean = lambda v: sum(v) / len(v) if v else float("nan")
    every = [v for f in per_frame.values() for v in f.values()]
    if names is None:
        names = ("psnr", "ssim", "lpips") if every and all(len(v) == 3 for v in every) else ("psnr", "ssim")
    elif any(len(v) != len(names) for v in every):
        raise ValueError(f"summarize: rows of other lengths than the {len(names)} columns {list(names)}")
    means = lambda rows: {k: mean([v[j] for v in rows]) for j, k in enumerate(names)}
    scenes = {s: {**means(list(f.values())), "frames": len(f), "per_frame": f} for s, f in per_frame.items()}
    return {"scenes": scenes, "overall": {**means(every), "frames": len(every)}}


def score_trees(pred_dir, gt_dir, device="cuda", batch: int = 64, lpips=None, dists=None, fid=None, inflate: str = "host") -> dict:
    """`metric_computer.test_step` over two PNG trees: every paired frame scored on the device, `batch` frames per launch.
    `lpips`: an `LPIPS` network on `device`; the per-frame rows then grow from [psnr, ssim] to [psnr, ssim, lpips].  `dists`: a `DISTS`
    network on `device` appends a dists column after that, and the report names its columns under "columns".  `fid`: a
    `FrechetInceptionDistance` on `device`; FID is one value per scene, so the per-frame rows do not change: every scene entry gains
    "fid" (None for a scene of fewer than 2 paired frames) and "overall" the mean over the scored scenes, as the reference's running
    table averages its per-scene values.  `inflate="device"`: the files' IDAT is inflated on the device too (`ops.png_decode`; opt-in,
    the same pixels)."""
    from concurrent.futures import ThreadPoolExecutor
    from .image_io import load_images
    pairs, missing = pair_trees(scan_tree(pred_dir), scan_tree(gt_dir))
    pool = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))      # the frames' inflate (zlib releases the GIL); the rest is the device's
    per_frame: Dict[str, Dict[int, List[float]]] = {}
    scene_fid: Dict[str, Optional[torch.Tensor]] = {}
    try:
        for scene, items in pairs.items():
            per_frame[scene] = {}
            if fid is not None:
                fid.reset()
            for i0 in range(0, len(items), batch):
                chunk = items[i0:i0 + batch]
                p = load_images([a for _, a, _ in chunk], device, pool, inflate=inflate)     # any PNG: Pillow's filtered rows, RGBA, grey, palette (ops.png_decode)
                g = load_images([b for _, _, b in chunk], device, pool, inflate=inflate)
                psnr, ssim = image_metrics(g, p)
                rows = [psnr.tolist(), ssim.tolist()] + ([] if lpips is None else [compute_lpips(g, p, lpips).tolist()]) \
                    + ([] if dists is None else [compute_dists(g, p, dists).tolist()])
                for (i, _, _), *row in zip(chunk, *rows):
                    per_frame[scene][i] = row
                if fid is not None and len(items) >= 2:
                    fid.update(g, real=True)
                    fid.update(p, real=False)
            if fid is not None:
                scene_fid[scene] = fid.compute() if len(items) >= 2 else None
                fid.reset()
    finally:
        pool.shutdown()
    if dists is None:
        rep = summarize(per_frame)
    else:
        rep = summarize(per_frame, names=metric_names(lpips, dists))
        rep["columns"] = list(metric_names(lpips, dists))
    if fid is not None:
        for scene, value in scene_fid.items():
            rep["scenes"][scene]["fid"] = None if value is None else float(value)
        scored = [v["fid"] for v in rep["scenes"].values() if v["fid"] is not None]
        rep["overall"]["fid"] = sum(scored) / len(scored) if scored else None
    rep["missing"] = [list(m) for m in missing]
    return rep


def main(argv=None):
    ap = argparse.ArgumentParser(description="PSNR / SSIM (/ LPIPS / DISTS / FID) of DIR/<scene>/color/<index>.png against a ground-truth tree of the same layout")
    ap.add_argument("--pred", required=True)
    ap.add_argument("--gt", required=True)
    ap.add_argument("--json", default=None, help="write the full report (per frame) here")
    ap.add_argument("--lpips", default=None, help="LPIPS(net='vgg') weights: the package's full state dict, or torchvision's VGG-16 (then --lpips-lin too); adds lpips")
    ap.add_argument("--lpips-lin", default=None, help="the lpips package's vgg.pth (lin layers), with a torchvision VGG-16 as --lpips")
    ap.add_argument("--dists", default=None, help="DISTS weights: the package's full state dict, or torchvision's VGG-16 (then --dists-weights too); adds dists")
    ap.add_argument("--dists-weights", default=None, help="the DISTS_pytorch package's weights.pt (alpha, beta), with a torchvision VGG-16 as --dists")
    ap.add_argument("--fid", default=None, help="Inception-v3 weights (torch-fidelity's pt_inception state dict or a torchmetrics FID state dict); "
                                                "adds fid (feature=64), one value per scene")
    ap.add_argument("--device-inflate", action="store_true", help="inflate the frames' IDAT on the device as well (the default inflates on the host); the same pixels")
    args = ap.parse_args(argv)
    if args.lpips_lin and not args.lpips:
        ap.error("--lpips-lin goes with --lpips")
    if args.dists_weights and not args.dists:
        ap.error("--dists-weights goes with --dists")
    if not torch.cuda.is_available():
        raise SystemExit("metrics needs a GPU (the HIP path has no CPU fallback)")
    rep = score_trees(args.pred, args.gt, lpips=load_lpips(args.lpips, args.lpips_lin) if args.lpips else None,
                      dists=load_dists(args.dists, args.dists_weights) if args.dists else None, fid=load_fid(args.fid) if args.fid else None,
                      inflate="device" if args.device_inflate else "host")
    for kind, scene, index, side in rep["missing"]:
        print(f"skipped {kind} {scene}" + ("" if index is None else f"/{index}") + f": missing in --{side}")
    extra = lambda r: (f" lpips {r['lpips']:.6f}" if "lpips" in r else "") + (f" dists {r['dists']:.6f}" if "dists" in r else "") \
        + ("" if "fid" not in r else " fid -" if r["fid"] is None else f" fid {r['fid']:.6f}")
    for s, r in rep["scenes"].items():
        print(f"{s}: psnr {r['psnr']:.4f} ssim {r['ssim']:.6f}{extra(r)} ({r['frames']} frames)")
    o = rep["overall"]
    print(f"overall: psnr {o['psnr']:.4f} ssim {o['ssim']:.6f}{extra(o)} ({o['frames']} frames)")
    if args.json:
        Path(args.json).write_text(json.dumps(rep, indent=1))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
