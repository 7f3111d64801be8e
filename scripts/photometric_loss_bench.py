"""Stage-0 loss (1 - lambda) L1 + lambda (1 - SSIM), forward + backward: the fused HIP kernels of opengaussian_amd.losses
against the fp32 torch composition a user had before them (tests/loss_restatement.py: the reference's five depthwise 11 x 11
conv2d calls and elementwise kernels, and their autograd twins).

  python scripts/photometric_loss_bench.py [--iters 200] [--repeats 3] [--warmup 20] [--out profiles/photometric_loss_bench.json]

Sizes: 1080 x 1920, 800 x 800 and 484 x 648 (the S1M, C2 and C4 configurations of bench.py).  Two things are timed at each:
the loss alone on a leaf image, and the full stage-0 step (RGB render of the bench scene + loss + backward through the
rasterizer).  Fused and torch legs alternate in one process after a warm-up of both; every leg is --iters iterations between
two device events; the pair is repeated --repeats times and every repeat is reported, so the spread is in the file.
Per-kernel times come from a separate profiled loop (HIP events per launch) and are set against each kernel's algorithmic
bytes (include/ogs_loss.h) and the HBM peak.  Nothing is measured without a GPU.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opengaussian_amd import _lib, losses  # noqa: E402
from opengaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from opengaussian_amd.synthetic import make_scene, orbit_camera  # noqa: E402
from tests import loss_restatement as lr  # noqa: E402

HBM_PEAK_GBPS = 8000.0          # MI355X HBM3E spec; about 6300 achievable
LAMBDA = 0.2
# (H, W, Gaussians, focal): bench.py's S1M-1080p, C2-100k-800 and C4-2M-648
SIZES = [(1080, 1920, 1_000_000, 1000.0), (800, 800, 100_000, 700.0), (484, 648, 2_000_000, 500.0)]


def algorithmic_bytes(H, W, C=3):
    n = C * H * W
    tiles = C * math.ceil(H / 32) * math.ceil(W / 32)
    return {"loss_photometric_forward_kernel": 8 * n + 16 * tiles, "loss_photometric_backward_kernel": 12 * n}


def images(H, W, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(1, 3, H // 8 + 2, W // 8 + 2, generator=g)
    gt = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[0]
    gt = (gt + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1).to(dev)
    img = (gt + 0.03 * torch.randn(3, H, W, generator=g).to(dev)).clamp(0, 1)
    return img.contiguous(), gt.contiguous()


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fused, torch_leg, args):
    for _ in range(args.warmup):
        fused(); torch_leg()
    torch.cuda.synchronize()
    f, t = [], []
    for _ in range(args.repeats):
        f.append(timed(fused, args.iters))
        t.append(timed(torch_leg, args.iters))
    spread = max(max(f) - min(f), max(t) - min(t))
    return {"fused_ms": [round(v, 4) for v in f], "torch_ms": [round(v, 4) for v in t],
            "fused_ms_median": round(sorted(f)[len(f) // 2], 4), "torch_ms_median": round(sorted(t)[len(t) // 2], 4),
            "spread_ms": round(spread, 4), "fused_faster_by_more_than_spread": bool(min(t) - max(f) > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="skip the full stage-0 step (render + loss + backward)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric_loss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photometric_loss_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "ogs_version": int(_lib.lib().ogs_version()), "lambda_dssim": LAMBDA,
              "iters_per_leg": args.iters, "repeats": args.repeats, "hbm_peak_gbps": HBM_PEAK_GBPS, "sizes": []}
    for H, W, P, f in SIZES:
        img, gt = images(H, W, dev)
        x = img.clone().requires_grad_(True)

        def loss_leg(fn):
            def run():
                x.grad = None
                fn(x, gt, LAMBDA)[0].backward()
            return run

        entry = {"H": H, "W": W, "loss_forward_backward": alternate(loss_leg(losses.photometric_loss),
                                                                     loss_leg(lr.photometric_loss), args)}
        # the two must agree before their times are compared
        x.grad = None
        lf = losses.photometric_loss(x, gt, LAMBDA)[0]; lf.backward(); gf = x.grad.clone()
        x.grad = None
        lt = lr.photometric_loss(x, gt, LAMBDA)[0]; lt.backward()
        lf, lt = float(lf.detach()), float(lt.detach())
        entry["agreement"] = {"loss_rel": abs(lf - lt) / abs(lt),
                              "grad_rel_of_max": float((gf - x.grad).abs().max() / x.grad.abs().max())}

        # per-kernel times: a profiled loop of its own
        _lib.prof_enable(1)
        for _ in range(20):
            loss_leg(losses.photometric_loss)()
        torch.cuda.synchronize()
        prof = {k: v for k, v in _lib.prof_collect().items() if k.startswith("loss_")}
        _lib.prof_enable(0)
        nbytes = algorithmic_bytes(H, W)
        entry["kernels"] = {}
        for k, v in sorted(prof.items()):
            ms = v["total_ms"] / max(v["calls"], 1)
            row = {"ms": round(ms, 5), "calls": v["calls"]}
            if k in nbytes:
                gbps = nbytes[k] / (ms * 1e-3) / 1e9
                row.update(algorithmic_bytes=nbytes[k], gbps=round(gbps, 1), share_of_hbm_peak=round(gbps / HBM_PEAK_GBPS, 4))
            entry["kernels"][k] = row

        if not args.no_step:
            scene = make_scene(P, W, H, f, f, seed=0).to(dev)
            cam = orbit_camera(W, H, f, f, view_index=0, num_views=8).to(dev)
            rs = GaussianRasterizationSettings(
                image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
                bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
                projmatrix=cam.full_proj_transform, sh_degree=3, campos=cam.camera_center, prefiltered=False, debug=False)
            rast = GaussianRasterizer(rs)
            leaves = [scene.means3D, scene.opacities, scene.shs, scene.scales, scene.rotations]
            for v in leaves:
                v.requires_grad_(True)

            def step_leg(fn):
                def run():
                    for v in leaves:
                        v.grad = None
                    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
                    color = rast(means3D=scene.means3D, means2D=m2, opacities=scene.opacities, shs=scene.shs,
                                 scales=scene.scales, rotations=scene.rotations)[0]
                    fn(color, gt, LAMBDA)[0].backward()
                return run

            entry["gaussians"] = P
            entry["stage0_step"] = alternate(step_leg(losses.photometric_loss), step_leg(lr.photometric_loss), args)
            del scene, rast, leaves
            torch.cuda.empty_cache()
        result["sizes"].append(entry)
        print(json.dumps(entry), flush=True)
    result["fused_loss_faster_at_every_size"] = all(e["loss_forward_backward"]["fused_faster_by_more_than_spread"]
                                                    for e in result["sizes"])
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
