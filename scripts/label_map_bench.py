"""Label map, measured (run on the MI355X; writes profiles/label_map_bench.json).

The query bench scene (500 k Gaussians, 988 x 731, 320 random leaves), one kept 12-channel pass, three legs in one process,
alternating, 3 repeats after a warm-up of each:
  (a) label_map   rasterizer.label_map on the kept pass: ONE launch of ogs_raster_label_map
  (b) one_hot     what a user had before: ceil(320 / 12) = 27 twelve-channel ogs_raster_forward_reblend launches over one-hot
                  colours, a running argmax between them (the runner-up weight, which (a) also returns, is not computed)
  (c) reblend     one forward re-blend of the same pass: the yardstick for "one walk over the streams"
(a) and (c) are also run with spatially coherent leaves (a grid over the image): random leaves are the worst case of (a).
The kernel times of (a) and (c) are read once more with HIP events around the launches, outside the timed window.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opengaussian_amd import _lib                                # noqa: E402
from opengaussian_amd import rasterizer as R                     # noqa: E402
from opengaussian_amd.synthetic import make_camera, make_scene   # noqa: E402

REPEATS = 3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(legs, repeats=REPEATS):
    for fn in legs.values():
        fn()
    times = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            times[name].append(timed(fn)[0])
    return {name: dict(ms=[round(t, 3) for t in ts], median=round(statistics.median(ts), 3), min=round(min(ts), 3),
                       max=round(max(ts), 3)) for name, ts in times.items()}


def kernel_ms(fn):
    _lib.prof_enable(1)
    fn()
    torch.cuda.synchronize()
    k = _lib.prof_collect()
    _lib.prof_enable(0)
    return {name: round(v["total_ms"], 3) for name, v in sorted(k.items(), key=lambda kv: -kv[1]["total_ms"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_map_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    import math
    P, W, H, f, K, C = 500_000, 988, 731, 800.0, 320, 12
    sc = make_scene(P, W, H, f, f, seed=0).to(dev)
    cam = make_camera(W, H, f, f).to(dev)
    g = torch.Generator().manual_seed(0)
    leaf = torch.randint(0, K, (P,), generator=g).to(dev)
    rs = R.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        bg=torch.zeros(C, device=dev), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=0, campos=cam.camera_center, prefiltered=False, debug=False)
    feats = torch.zeros(P, C, device=dev)
    sink: list = []
    with torch.no_grad():
        _, _, _, alpha = R._RasterizeGaussians.apply(sc.means3D, torch.zeros_like(sc.means3D), None, feats, sc.opacities, sc.scales,
                                                      sc.rotations, None, rs, 0, None, None, 1, sink)
    kp = R.KeptPasses(budget_bytes=8 << 30)
    assert sink and kp.admit("view", "key", None, sink[0])
    entry = kp.slots["view"]
    del sink

    def label_map():
        return R.label_map(entry, leaf, K)

    def reblend():
        with torch.no_grad():
            return R._ReblendKept.apply(feats, entry, rs)

    def one_hot():
        best = torch.zeros(H, W, device=dev)
        label = torch.full((H, W), -1, dtype=torch.int64, device=dev)
        ids = torch.arange(C, device=dev)
        with torch.no_grad():
            for c0 in range(0, K, C):
                onehot = (leaf[:, None] == (ids + c0)[None, :]).to(torch.float32)
                color = R._ReblendKept.apply(onehot, entry, rs)[0]
                w, i = color.max(0)
                better = w > best
                best = torch.where(better, w, best)
                label = torch.where(better, i + c0, label)
        return label, best

    res = alternate({"label_map": label_map, "one_hot": one_hot, "reblend": reblend})
    # the same call with spatially coherent leaves (a 20 x 16 grid over the image: a tile sees a handful of labels, one walk) --
    # random leaves put nearly all 320 labels into every tile, five walks of 64 labels each
    tanx, tany = W / (2 * f), H / (2 * f)
    u = sc.means3D[:, 0] / (sc.means3D[:, 2].abs().clamp_min(0.2) * tanx)
    v = sc.means3D[:, 1] / (sc.means3D[:, 2].abs().clamp_min(0.2) * tany)
    grid = ((u + 1.1) / 2.2 * 20).floor().clamp(0, 19) + 20 * ((v + 1.1) / 2.2 * 16).floor().clamp(0, 15)
    leaf_grid = grid.to(torch.int64)
    coherent = alternate({"label_map": lambda: R.label_map(entry, leaf_grid, K), "reblend": reblend})
    a, b = label_map(), one_hot()
    out = {"device": torch.cuda.get_device_properties(0).name, "ogs_version": int(_lib.lib().ogs_version()), "repeats": REPEATS,
           "scene": dict(P=P, W=W, H=H, leaves=K, kept_records=int(entry.D), kept_channels=C),
           "wall_ms": res,
           "one_hot_launches": (K + C - 1) // C,
           "labels_equal_one_hot": bool(torch.equal(a[0].to(torch.int64), b[0])),
           "weights_equal_one_hot": bool(torch.equal(a[1], b[1])),
           "alpha_equal_pass": bool(torch.equal(a[3], alpha[0])),
           "one_hot_over_label_map": round(res["one_hot"]["median"] / res["label_map"]["median"], 2),
           "label_map_over_reblend": round(res["label_map"]["median"] / res["reblend"]["median"], 2),
           "kernels_ms": {"label_map": kernel_ms(label_map), "reblend": kernel_ms(reblend)},
           "coherent_leaves": {"wall_ms": coherent,
                               "label_map_over_reblend": round(coherent["label_map"]["median"] / coherent["reblend"]["median"], 2),
                               "kernels_ms": kernel_ms(lambda: R.label_map(entry, leaf_grid, K))},
           "extra_memory_bytes": {"label_map": 4 * 4 * W * H, "one_hot_per_launch": (C + 2) * 4 * W * H + 4 * P * C,
                                  "grouped_pass_of_all_leaves": K * 5 * 4 * W * H}}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
