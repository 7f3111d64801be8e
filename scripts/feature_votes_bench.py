"""Feature votes, measured (run on the MI355X; writes profiles/feature_votes_bench.json).

The query bench scene of scripts/label_votes_bench.py (500 k Gaussians, 988 x 731, 320 random leaves), one kept 9-channel pass,
three legs in one process, alternating, 3 repeats after a warm-up of each, wall ms with a sync:
  (a) feature_votes  rasterizer.feature_votes on the kept pass: ONE call of ogs_raster_feature_votes, accumulating into a table
                     that is allocated (and cleared) outside the timed window
  (b) backward_route what a user had before: ceil((D + 1) / 9) features-only backward launches over the same kept pass with the
                     planes F[c] and the valid plane as upstream gradients, the nine columns copied into a [P, D + 1] fp32 table
                     (and, with rows, one index_add of that table over the leaf ids); the one forward re-blend the graph needs
                     is made outside the timed window
  (c) backward       one features-only backward of the pass with dense upstream planes: the unit
for D = 6, 16, 64 and 512 (seeded normal features, no mask), rows = None and rows = leaf.  The kernel time of (a) is read once
more from the library's own event timer, outside the timed window.

--votes-only: leg (a) alone, for the -DOGS_EXPERIMENTS variant builds named by OGS_LIB_PATH: another block width
(-DOGS_FEATURE_VOTES_DB=16 / 32 / 64) or the ablations whose tables are wrong by construction (OGS_VOTES_WALK_ONLY,
OGS_VOTES_NO_ATOMICS).
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
CHANNELS = (6, 16, 64, 512)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_votes_bench.json"))
    ap.add_argument("--votes-only", action="store_true")
    ap.add_argument("--channels", type=int, nargs="*", default=list(CHANNELS))
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

    def backward():
        return torch.autograd.grad(color, cols, dense, retain_graph=True)[0]

    results = {}
    for D in args.channels:
        F = torch.randn(D, H, W, generator=torch.Generator().manual_seed(100 + D)).to(dev)
        launches = (D + 1 + C - 1) // C
        # the upstream planes of leg (b): F, the valid plane (all ones: no mask), zero padding to a whole launch
        planes = None if args.votes_only else torch.cat([F, torch.ones(1, H, W, device=dev),
                                                         torch.zeros(launches * C - D - 1, H, W, device=dev)])
        for rows_name, rows, Rn in (("none", None, P), ("leaf", leaf.to(torch.int32), K)):
            table = torch.zeros(Rn, D + 1, dtype=torch.int64, device=dev)
            dense_table = None if args.votes_only else torch.zeros(P, D + 1, device=dev)

            def votes():
                return R.feature_votes(entry, F, rows=rows, num_rows=Rn, out=table)

            def route():
                for i in range(launches):
                    grad = torch.autograd.grad(color, cols, planes[i * C:(i + 1) * C], retain_graph=True)[0]
                    n = min(C, D + 1 - i * C)
                    dense_table[:, i * C:i * C + n] = grad[:, :n]
                if rows is None:
                    return dense_table
                return torch.zeros(Rn, D + 1, device=dev).index_add_(0, leaf, dense_table)

            legs = {"feature_votes": votes} if args.votes_only else {"feature_votes": votes, "backward_route": route, "backward": backward}
            res = alternate(legs)
            rec = {"wall_ms": res, "kernels_ms": kernel_ms(votes)}
            if not args.votes_only:
                table.zero_()
                a = votes().to(torch.float64) * 2.0 ** -32
                b = route().to(torch.float64)
                va, vb = res["feature_votes"], res["backward_route"]
                spread = max(va["max"] - va["min"], vb["max"] - vb["min"])
                rec.update(route_launches=launches,
                           route_over_feature_votes=round(vb["median"] / va["median"], 2),
                           feature_votes_over_backward=round(va["median"] / res["backward"]["median"], 2),
                           spread_ms=round(spread, 3),
                           faster_by_more_than_the_spread=bool(vb["median"] - va["median"] > spread and vb["min"] > va["max"]),
                           max_difference_over_table_max=float((a - b).abs().max() / b.abs().max()),
                           sum_of_weight_column=float(a[:, D].sum()), sum_of_alpha=float(alpha.to(torch.float64).sum()),
                           extra_memory_bytes={"feature_votes": 8 * Rn * (D + 1),
                                               "backward_route": 4 * P * (D + 1) + (4 * Rn * (D + 1) if rows is not None else 0)
                                               + 4 * (launches * C - D) * W * H + 2 * 4 * P * C})
                del a, b
            results[f"D{D}_rows_{rows_name}"] = rec
            print(f"D{D}_rows_{rows_name}", json.dumps(rec), flush=True)
            del table, dense_table
        del F, planes
    out = {"device": torch.cuda.get_device_properties(0).name, "ogs_version": int(_lib.lib().ogs_version()), "repeats": REPEATS,
           "library": os.path.basename(os.environ.get("OGS_LIB_PATH", "default")),
           "block_columns": int(_lib.lib().ogs_feature_votes_block_columns()),
           "scene": dict(P=P, W=W, H=H, leaves=K, kept_records=int(entry.D), kept_channels=C), "cases": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
