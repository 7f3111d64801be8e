"""One whole stage-1 training iteration as train.py:352-358,425-456,594-611 wires it, at the bench size (1 M Gaussians,
1920x1080, 96 SAM-like masks, 8 cameras cycled): render() (fused RGB + 6-D ins_feat pass, geometry detached) ->
mask_feature_mean weighted by the silhouette -> separation + 0.1 * cohesion -> backward through the rasterizer's
features-only path -> FusedAdam on the instance features.  Prints one JSON line: ms per iteration and the split between
the render (forward + backward kernels) and everything else.

`--masks stack|onehot|labels` (default stack; a comma-separated list alternates the modes in one process, `--rounds R` times
each, and prints one line per mode with the spread over the rounds) says where the masks of an iteration come from:
  stack    a bool [N,H,W] stack built once, outside the timed loop
  onehot   the reference's per-iteration construction (utils/opengs_utlis.py:146-148,181) inside the timed loop:
           F.one_hot(mask_id.long(), N + 1).permute(2, 0, 1)[1:], handed to the loss functions as it is
  labels   mask_ops.get_SAM_mask_and_feat (one int32 label image, no one-hot) inside the timed loop"""
import argparse
import json
import math
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opengaussian_amd import _lib, mask_ops as mk  # noqa: E402
from opengaussian_amd.optim import FusedAdam  # noqa: E402
from opengaussian_amd.renderer import render  # noqa: E402
from opengaussian_amd.synthetic import make_scene, orbit_camera  # noqa: E402


def alternate(iteration, modes, rounds, NM):
    """the modes in turn, `rounds` times each; one JSON line per mode"""
    K = 100
    ms = {m: [] for m in modes}
    for m in modes:
        for it in range(10):
            iteration(it, m)
    for _ in range(rounds):
        for m in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for it in range(K):
                iteration(10 + it, m)
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) / K * 1e3)
    for m in modes:
        _lib.prof_enable(1)
        for it in range(16):
            iteration(200 + it, m)
        torch.cuda.synchronize()
        pr = _lib.prof_collect()
        _lib.prof_enable(0)
        kern = {k: v["total_ms"] / 16 for k, v in pr.items()}
        loss_k = ("mask_", "label_", "separation", "adam")
        xs = sorted(ms[m])
        print(json.dumps({"masks_mode": m, "stage1_iteration_ms": xs[len(xs) // 2], "min_ms": xs[0], "max_ms": xs[-1],
                          "rounds": rounds, "masks": NM, "hip_kernel_ms_per_iteration": sum(kern.values()),
                          "rasterizer_kernels_ms": sum(v for k, v in kern.items() if not k.strip("(").startswith(loss_k)),
                          "loss_and_optimizer_kernels_ms": {k: round(v, 4) for k, v in kern.items()
                                                            if k.strip("(").startswith(loss_k)}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masks", default="stack")
    ap.add_argument("--rounds", type=int, default=1)
    args = ap.parse_args()
    modes = args.masks.split(",")
    assert all(m in ("stack", "onehot", "labels") for m in modes), modes
    dev = torch.device("cuda:0")
    P, W, H, f, V, NM = 1_000_000, 1920, 1080, 1000.0, 8, 96
    sc = make_scene(P, W, H, f, f, seed=0).to(dev)
    cams = [orbit_camera(W, H, f, f, v, V).to(dev) for v in range(V)]
    ins = torch.nn.Parameter((sc.ins_feat * 2 - 1).clone())
    geo = types.SimpleNamespace(
        get_xyz=sc.means3D, get_scaling=sc.scales, get_rotation=sc.rotations, get_opacity=sc.opacities,
        get_features=sc.shs, get_ins_feat=lambda origin=False: torch.nn.functional.normalize(ins, dim=1),
        active_sh_degree=3, max_sh_degree=3)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = torch.zeros(3, device=dev)
    # SAM-like label image: 12 x 8 blocky regions, label 0 = invalid
    lab = (torch.arange(H, device=dev)[:, None] // 135) * 12 + (torch.arange(W, device=dev)[None, :] // 160) + 1
    lab[:, :16] = 0
    masks = torch.stack([lab == (n + 1) for n in range(NM)])
    # the same labels as the level-3 plane of a [4,H,W] SAM id stack (ids continue after the previous level's maximum, -1 = none)
    gt_sam = torch.stack([torch.full_like(lab, lvl) for lvl in range(3)] + [torch.where(lab > 0, lab + 2, -1)])
    opt = FusedAdam([{"params": [ins], "lr": 1e-3, "name": "ins_feat"}], lr=0.0, eps=1e-15)

    def iteration(it, mode="stack"):
        out = render(cams[it % V], geo, pipe, bg, iteration=it, rescale=False)
        feat, sil = out["ins_feat"], out["silhouette"]
        if mode == "onehot":
            m = torch.nn.functional.one_hot(lab.long(), NM + 1).permute(2, 0, 1)[1:]
        elif mode == "labels":
            _, m, _ = mk.get_SAM_mask_and_feat(gt_sam, level=3)
        else:
            m = masks
        mean = mk.mask_feature_mean(feat, m, image_mask=sil)
        loss = mk.separation_loss(mean, it) + 0.1 * mk.cohesion_loss(feat, m, mean)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    if modes != ["stack"] or args.rounds != 1:
        return alternate(iteration, modes, args.rounds, NM)
    for it in range(10):
        iteration(it)
    torch.cuda.synchronize()
    K = 100
    t0 = time.perf_counter()
    for it in range(K):
        iteration(10 + it)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / K * 1e3
    _lib.prof_enable(1)
    for it in range(16):
        iteration(200 + it)
    torch.cuda.synchronize()
    pr = _lib.prof_collect()
    _lib.prof_enable(0)
    kern = {k: v["total_ms"] / 16 for k, v in pr.items()}
    raster = sum(v for k, v in kern.items() if not k.startswith(("mask_", "separation", "adam")))
    print(json.dumps({"stage1_iteration_ms": ms, "masks": NM, "hip_kernel_ms_per_iteration": sum(kern.values()),
                      "rasterizer_kernels_ms": raster,
                      "loss_and_optimizer_kernels_ms": {k: round(v, 4) for k, v in kern.items() if k.startswith(("mask_", "separation", "adam"))}}))


if __name__ == "__main__":
    main()
