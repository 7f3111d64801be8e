"""Whole-call time of the multi-view SAM mask refinement (opengaussian_amd.sam_refine) against the per-pair loop a user had
before it: the reference's structure, one P = 1 pass of the drop-in rasterizer per (Gaussian, camera) pair followed by the
full-frame post-processing (tests/refine_restatement.py: uint8 frame, weight map, weighted bincount).

  python scripts/sam_refine_bench.py [--gaussians 500000] [--cameras 32] [--runs 5] [--sample 2000]
                                     [--out profiles/sam_refine_bench.json]

Scene (C3 class): 500 k Gaussians in a slab (a surface with some depth, so that the reference's depth test keeps a share of
them), 32 general-pose cameras on a fan around it at 988 x 731, two levels of block-structured label images per camera.

Kernel path: the whole ``refine_sam_masks`` call, host clock around a device synchronise, one warm-up call, median of --runs.
Loop: the per-pair body (render + fix_image + weight map + dominant id; the expansion step is NOT included, which favours the
loop) timed in the same process over a fixed seeded sample of --sample visible pairs and EXTRAPOLATED to the pair count of the
scene -- 2 x 10^6 rasterizer calls are not run.  Per-kernel times come from a separate profiled call (HIP events per launch).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opengaussian_amd import _lib  # noqa: E402
from opengaussian_amd.sam_refine import MultiViewSAMMaskRefiner  # noqa: E402
from tests import refine_restatement as rr  # noqa: E402
from tests.golden import sam_refine_cases as sc  # noqa: E402

W, H, FOCAL = 988, 731, 780.0


def build_scene(P, ncam, seed=3):
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)
    xyz = torch.stack([rand(P) * 4.4 - 2.2, rand(P) * 3.2 - 1.6, rand(P) * 0.3 - 0.15], dim=1)
    scaling = torch.exp(torch.randn(P, 3, generator=g) * 0.5 - 5.0)
    q = torch.randn(P, 4, generator=g)
    opacity = torch.sigmoid(torch.randn(P, 1, generator=g) * 2.0 + 2.0)
    opacity[::3] = 0.99 + 0.009 * rand(opacity[::3].shape[0], 1)
    features = torch.cat([0.5 * torch.randn(P, 1, 3, generator=g), 0.1 * torch.randn(P, 15, 3, generator=g)], dim=1)
    model = sc.Model(xyz.contiguous(), opacity.contiguous(), scaling.contiguous(),
                     (q / q.norm(dim=1, keepdim=True)).contiguous(), features.contiguous())
    cams, masks = [], []
    for k in range(ncam):
        ang = 2 * math.pi * k / ncam
        eye = (1.6 * math.cos(ang), 1.0 * math.sin(ang), -4.0 + 0.4 * math.cos(3 * ang))
        cams.append(sc.make_camera(W, H, FOCAL, eye, 0.5 * math.sin(2 * ang)))
        levels = []
        for lvl, block in enumerate((64, 160)):
            ny, nx = -(-H // block), -(-W // block)
            ids = torch.randperm(ny * nx, generator=g).reshape(ny, nx) + 1 + 1000 * lvl + 7 * k
            level = ids.repeat_interleave(block, 0).repeat_interleave(block, 1)[:H, :W].clone()
            level[:24, :] = -1
            level[-16:, :40] = 0
            levels.append(level)
        masks.append(torch.stack(levels).to(torch.int32).contiguous())
    return model, cams, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--cameras", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_refine_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sam_refine_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    model, cams, masks = build_scene(args.gaussians, args.cameras)
    model, cams, masks = model.to(dev), [c.to(dev) for c in cams], [m.to(dev) for m in masks]

    def call(keep=False):
        refiner = MultiViewSAMMaskRefiner()
        refiner.keep_intermediates = keep
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = refiner.refine_sam_masks(cams, masks, model, sam_level=0)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, refiner, out

    _, warm, out = call(keep=True)                                   # warm-up: library load, allocator, every shape
    vis = warm.last["visibility"]
    refined = warm.last["refined_masks"]
    changed = sum(int((o[0] != r[0]).sum()) for o, r in zip(out, refined))
    stats = dict(warm.stats)
    pairs = stats["pairs"]
    times = [call()[0] for _ in range(args.runs)]
    kernel_s = statistics.median(times)

    # per-kernel times: one profiled call of its own
    _lib.prof_enable(1)
    call()
    prof = {k: v for k, v in _lib.prof_collect().items() if k.startswith("refine_")}
    _lib.prof_enable(0)

    # the per-pair loop on a fixed sample of the visible pairs
    rasterize = sc.hip_rasterize(model)
    idx = torch.nonzero(vis).cpu()
    pick = idx[torch.randperm(idx.shape[0], generator=torch.Generator().manual_seed(11))[:args.sample]].tolist()

    def loop(sample):
        for g, c in sample:
            image, _ = rasterize(cams[c], [g], True)
            q, weight, seen = rr.footprint(image)
            if seen:
                rr.dominant_id(refined[c][0], weight)

    loop(pick[:50])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop(pick)
    torch.cuda.synchronize()
    loop_s = time.perf_counter() - t0
    per_pair = loop_s / max(len(pick), 1)

    result = {
        "device": torch.cuda.get_device_name(0), "ogs_version": int(_lib.lib().ogs_version()),
        "scene": {"gaussians": args.gaussians, "cameras": args.cameras, "W": W, "H": H,
                  "labels_per_camera": int(torch.unique(refined[0][0]).numel())},
        "pairs": pairs, "stage1_pairs": stats["stage1_pairs"], "expand_pairs": stats["expand_pairs"],
        "pixels_changed": changed,
        "kernel_path": {"seconds_median": round(kernel_s, 4), "seconds_runs": [round(t, 4) for t in times],
                        "pairs_per_second": round(pairs / kernel_s, 1)},
        "per_pair_loop": {"sampled_pairs": len(pick), "sample_seconds": round(loop_s, 4),
                          "ms_per_pair": round(per_pair * 1e3, 4), "pairs_per_second": round(1.0 / per_pair, 1),
                          "seconds_extrapolated_to_all_pairs": round(per_pair * pairs, 1),
                          "note": "extrapolation from the sample; expansion step not included"},
        "kernel_ms_one_call": {k: round(v["total_ms"], 3) for k, v in sorted(prof.items())},
        "kernel_launches_one_call": {k: v["calls"] for k, v in sorted(prof.items())},
        "accumulator_bytes": stats["accumulator_bytes"], "slow_path_pairs": stats["slow_path_pairs"],
        "large_rect_pairs": stats["large_rect_pairs"],
    }
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    if not per_pair * pairs > kernel_s:
        raise SystemExit("the kernel path is not faster than the extrapolated per-pair loop")


if __name__ == "__main__":
    main()
