"""Label votes, measured (run on the MI355X; writes profiles/label_votes_bench.json).

The query bench scene (500 k Gaussians, 988 x 731, 320 random leaves), one kept 9-channel pass, three legs in one process,
alternating, 3 repeats after a warm-up of each, wall ms with a sync:
  (a) label_votes   rasterizer.label_votes on the kept pass: ONE launch of ogs_raster_label_votes, accumulating into a table
                    that is allocated (and cleared) outside the timed window
  (b) one_hot       what a user had before: ceil((L + 1) / 9) features-only backward launches over the same kept pass, each with
                    its nine one-hot [H, W] upstream planes, the nine columns copied into a [P, L + 1] fp32 table (and, with rows,
                    one index_add of that table over the leaf ids); the one forward re-blend the graph needs is made outside the
                    timed window
  (c) backward      one features-only backward of the pass with dense upstream planes: the unit
for L = 20 and L = 200, each with a coherent label image (blocks of 32 px) and with per-pixel noise, rows = None and rows = leaf.
The kernel time of (a) is read once more from the library's own event timer, outside the timed window.

--votes-only: leg (a) alone (for the -DOGS_EXPERIMENTS ablation builds named by OGS_LIB_PATH, whose tables are wrong by
construction: OGS_VOTES_WALK_ONLY, OGS_VOTES_NO_ATOMICS).
"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_votes_bench.json"))
    ap.add_argument("--votes-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    P, W, H, f, K, C = 500_000, 988, 731, 800.0, 320, 9
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

    cols = torch.zeros(P, C, device=dev, requires_grad=True)
    color = R._ReblendKept.apply(cols, entry, rs)[0]                   # the graph the backward legs differentiate
    dense = torch.rand(C, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    ids = torch.arange(C, device=dev)[:, None, None]
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")

    def backward():
        return torch.autograd.grad(color, cols, dense, retain_graph=True)[0]

    results = {}
    for L in (20, 200):
        images = {"coherent": (((y // 32) * ((W + 31) // 32) + x // 32) % L).to(dev),
                  "noise": torch.randint(0, L, (H, W), generator=g).to(dev)}
        for kind, img in images.items():
            lab32 = img.to(torch.int32)
            for rows_name, rows, Rn in (("none", None, P), ("leaf", leaf.to(torch.int32), K)):
                table = torch.zeros(Rn, L + 1, dtype=torch.int64, device=dev)
                dense_table = torch.zeros(P, L + 1, device=dev)

                def votes():
                    return R.label_votes(entry, lab32, L, rows=rows, num_rows=Rn, out=table)

                def one_hot():
                    for c0 in range(0, L + 1, C):
                        planes = (img[None] == ids + c0).to(torch.float32)
                        grad = torch.autograd.grad(color, cols, planes, retain_graph=True)[0]
                        n = min(C, L + 1 - c0)
                        dense_table[:, c0:c0 + n] = grad[:, :n]
                    if rows is None:
                        return dense_table
                    return torch.zeros(Rn, L + 1, device=dev).index_add_(0, leaf, dense_table)

                legs = {"label_votes": votes} if args.votes_only else {"label_votes": votes, "one_hot": one_hot, "backward": backward}
                res = alternate(legs)
                rec = {"wall_ms": res, "kernels_ms": kernel_ms(votes)}
                if not args.votes_only:
                    table.zero_()
                    a = votes().to(torch.float64) * 2.0 ** -32
                    b = one_hot().to(torch.float64)
                    rec.update(one_hot_launches=(L + 1 + C - 1) // C,
                               one_hot_over_label_votes=round(res["one_hot"]["median"] / res["label_votes"]["median"], 2),
                               label_votes_over_backward=round(res["label_votes"]["median"] / res["backward"]["median"], 2),
                               max_difference_over_table_max=float((a - b).abs().max() / b.max()),
                               sum_of_table=float(a.sum()), sum_of_alpha=float(alpha.to(torch.float64).sum()),
                               extra_memory_bytes={"label_votes": 8 * Rn * (L + 1) + 4 * W * H,
                                                   "one_hot": 4 * P * (L + 1) + (4 * Rn * (L + 1) if rows is not None else 0)
                                                   + 2 * 4 * C * W * H + 2 * 4 * P * C})
                results[f"L{L}_{kind}_rows_{rows_name}"] = rec
                print(f"L{L}_{kind}_rows_{rows_name}", json.dumps(rec), flush=True)
                del table, dense_table
    out = {"device": torch.cuda.get_device_properties(0).name, "ogs_version": int(_lib.lib().ogs_version()), "repeats": REPEATS,
           "library": os.path.basename(os.environ.get("OGS_LIB_PATH", "default")),
           "scene": dict(P=P, W=W, H=H, leaves=K, kept_records=int(entry.D), kept_channels=C), "cases": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
