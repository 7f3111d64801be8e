"""Stage-0 step (render(), photometric_loss, backward) through a model with the reference's getters -- exp / F.normalize /
sigmoid / cat as torch operations in front of the rasterizer, autograd behind it (scene/gaussian_model.py:122-159) -- against
the same model with ``pipe.raw_model_pass``: the activations inside the rasterizer's per-Gaussian kernels, gradients with
respect to the raw parameters (include/ogs_model.h).

  python scripts/raw_model_bench.py [--iters 80] [--repeats 3] [--warmup 16] [--sizes S1M,C4,C2] [--out profiles/raw_model_bench.json]
  python scripts/raw_model_bench.py --trace [--sizes C2] [--out profiles/raw_model_trace.json]

Sizes: S1M (1 M Gaussians, 1920 x 1080), C4-class (2 M, 648 x 484), C2 (100 k, 800 x 800); SH degree 3; 8 cameras cycled.  The two
ways alternate in one process after a warm-up of both; a leg is --iters steps between two device events (the second one waited
for), the pair is repeated --repeats times and every repeat is in the file.  The raw pass "wins" at a size when its median
lies below the getter path's and outside its spread (min .. max of the repeats).  Before the timing the images, radii and
raw-parameter gradients of the two ways are compared on every camera and the worst differences recorded.
--trace: a run of its own (no timing): the device kernels of a few steps of either way by name (torch.profiler), and the names
that only the getter path launches.  Nothing is measured without a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opengaussian_amd import _lib, losses  # noqa: E402
from opengaussian_amd import rasterizer as R  # noqa: E402
from opengaussian_amd.renderer import render  # noqa: E402
from opengaussian_amd.synthetic import make_scene, orbit_camera  # noqa: E402

LAMBDA = 0.2
NUM_CAMERAS = 8
# name -> (W, H, Gaussians, focal): bench.py's S1M-1080p, C4-2M-648 and C2-100k-800
SIZES = {"S1M": (1920, 1080, 1_000_000, 1000.0), "C4": (648, 484, 2_000_000, 500.0), "C2": (800, 800, 100_000, 700.0)}
PARAMS = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")


class GetterModel:
    """The part of scene/gaussian_model.py:GaussianModel that a stage-0 render() reads: raw parameters, the reference's getters."""

    def __init__(self, sc, dev):
        g = torch.Generator().manual_seed(1)
        op = sc.opacities.clamp(1e-4, 1 - 1e-4)
        leaf = lambda t: t.contiguous().to(dev).requires_grad_(True)
        self._xyz = leaf(sc.means3D)
        self._features_dc, self._features_rest = leaf(sc.shs[:, :1]), leaf(sc.shs[:, 1:])
        self._scaling = leaf(torch.log(sc.scales))
        self._rotation = leaf(sc.rotations * (0.5 + torch.rand(sc.rotations.shape[0], 1, generator=g)))
        self._opacity = leaf(torch.log(op / (1 - op)))
        self.active_sh_degree = self.max_sh_degree = 3

    get_xyz = property(lambda s: s._xyz)
    get_scaling = property(lambda s: torch.exp(s._scaling))
    get_rotation = property(lambda s: torch.nn.functional.normalize(s._rotation))
    get_opacity = property(lambda s: torch.sigmoid(s._opacity))
    get_features = property(lambda s: torch.cat((s._features_dc, s._features_rest), dim=1))

    def zero_grad(self):
        for n in PARAMS:
            getattr(self, n).grad = None


def pipes():
    base = dict(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    return types.SimpleNamespace(**base), types.SimpleNamespace(raw_model_pass=True, **base)


def make_step(pc, cams, gts, bg, pipe):
    state = {"i": 0}

    def step():
        k = state["i"] % len(cams)
        state["i"] += 1
        pc.zero_grad()
        out = render(cams[k], pc, pipe, bg, 1, rescale=False, render_feat_map=False)
        losses.photometric_loss(out["render"], gts[k], LAMBDA)[0].backward()
        return out
    return step


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def compare(pc, cams, gts, bg, p_get, p_raw):
    """worst differences between the two ways over the cameras: images (absolute), radii (rows), gradients (of the family maximum)"""
    worst = {"image_abs": 0.0, "depth_abs": 0.0, "alpha_abs": 0.0, "radii_rows_different": 0, "grad_rel_of_family_max": {}}
    for k in range(len(cams)):
        res = []
        for pipe in (p_get, p_raw):
            step = make_step(pc, cams[k:k + 1], gts[k:k + 1], bg, pipe)
            out = step()
            res.append((out, {n: getattr(pc, n).grad.clone() for n in PARAMS}, out["viewspace_points"].grad.clone()))
        (oa, ga, va), (ob, gb, vb) = res
        worst["image_abs"] = max(worst["image_abs"], float((oa["render"] - ob["render"]).abs().max()))
        worst["depth_abs"] = max(worst["depth_abs"], float((oa["depth"] - ob["depth"]).abs().max()))
        worst["alpha_abs"] = max(worst["alpha_abs"], float((oa["alpha"] - ob["alpha"]).abs().max()))
        worst["radii_rows_different"] = max(worst["radii_rows_different"], int((oa["radii"] != ob["radii"]).sum()))
        ga["viewspace_points"], gb["viewspace_points"] = va, vb
        for n in ga:
            rel = float((ga[n] - gb[n]).abs().max() / ga[n].abs().max().clamp_min(1e-30))
            worst["grad_rel_of_family_max"][n] = max(worst["grad_rel_of_family_max"].get(n, 0.0), rel)
    return worst


def kernel_names(step, steps):
    from torch.profiler import ProfilerActivity, profile
    for _ in range(NUM_CAMERAS):
        step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        dev_us = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
        if dev_us > 0:
            out[ev.key] = {"calls_per_step": round(ev.count / steps, 2), "us_per_step": round(dev_us / steps, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--sizes", default="S1M,C4,C2")
    ap.add_argument("--trace", action="store_true", help="kernel names of either way instead of the timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raw_model_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    out_path = args.out or os.path.join(ROOT, "profiles", "raw_model_trace.json" if args.trace else "raw_model_bench.json")
    result = {"device": torch.cuda.get_device_name(0), "ogs_version": int(_lib.lib().ogs_version()), "lambda_dssim": LAMBDA,
              "cameras": NUM_CAMERAS, "iters_per_leg": args.iters, "repeats": args.repeats, "sizes": []}
    p_get, p_raw = pipes()
    bg = torch.zeros(3, device=dev)
    for name in args.sizes.split(","):
        W, H, P, f = SIZES[name]
        pc = GetterModel(make_scene(P, W, H, f, f, seed=0), dev)
        cams = [orbit_camera(W, H, f, f, view_index=v, num_views=NUM_CAMERAS).to(dev) for v in range(NUM_CAMERAS)]
        with torch.no_grad():
            gts = [(render(c, pc, p_get, bg, 1, rescale=False, render_feat_map=False)["render"] * 0.9 + 0.05).clamp(0, 1).contiguous()
                   for c in cams]
        getter, raw = make_step(pc, cams, gts, bg, p_get), make_step(pc, cams, gts, bg, p_raw)
        entry = {"size": name, "W": W, "H": H, "gaussians": P}
        if args.trace:
            kg, kr = kernel_names(getter, NUM_CAMERAS), kernel_names(raw, NUM_CAMERAS)
            entry["getter_path_kernels"], entry["raw_pass_kernels"] = kg, kr
            entry["only_in_getter_path"] = sorted(set(kg) - set(kr))
            entry["only_in_raw_pass"] = sorted(set(kr) - set(kg))
            entry["launches_per_step"] = {"getter_path": round(sum(v["calls_per_step"] for v in kg.values()), 1),
                                          "raw_pass": round(sum(v["calls_per_step"] for v in kr.values()), 1)}
        else:
            entry["agreement"] = compare(pc, cams, gts, bg, p_get, p_raw)
            n0 = R.PASS_STATS["raw_model"]
            for _ in range(args.warmup):
                getter(); raw()
            torch.cuda.synchronize()
            assert R.PASS_STATS["raw_model"] - n0 == args.warmup, "the opted-in leg did not take the raw pass"
            tg, tr = [], []
            for _ in range(args.repeats):
                tg.append(timed(getter, args.iters))
                tr.append(timed(raw, args.iters))
            med = lambda v: sorted(v)[len(v) // 2]
            entry.update(getter_path_ms=[round(v, 4) for v in tg], raw_pass_ms=[round(v, 4) for v in tr],
                         getter_path_ms_median=round(med(tg), 4), raw_pass_ms_median=round(med(tr), 4),
                         getter_path_spread_ms=[round(min(tg), 4), round(max(tg), 4)],
                         raw_pass_wins=bool(med(tr) < min(tg)), saved_ms=round(med(tg) - med(tr), 4))
        result["sizes"].append(entry)
        print(json.dumps(entry), flush=True)
        del pc, cams, gts, getter, raw
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
    print("written:", out_path)


if __name__ == "__main__":
    main()
