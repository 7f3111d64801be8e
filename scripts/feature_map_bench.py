"""Feature maps, measured (run on the MI355X; writes profiles/feature_map_bench.json).

The query bench scene of scripts/feature_votes_bench.py (500 k Gaussians, 988 x 731, 320 random leaves), one kept 12-channel pass
with a zero background, legs in one process, alternating, 3 repeats after a warm-up of each, wall ms with a sync:
  (a) feature_map     rasterizer.feature_map on the kept pass: ONE call of ogs_raster_feature_map, planar [D, H, W] and
                      channels-last [H, W, D]; the output is allocated inside the window, as a user's call does
  (b) reblend_route   what a user had before: ceil(D / 12) re-blends (_ReblendKept) of the kept pass over [P, 12] slices of the
                      per-Gaussian features, the planes copied into one [D, H, W] tensor.  The slices are cut (and, with rows,
                      X[rows] is gathered) ONCE outside the timed window -- the route at its best; their bytes are reported
  (c) reblend         one re-blend of the pass: the unit, "one walk"
for D = 6, 16, 64 and 512 (seeded normal features), rows = None ([P, D] table) and rows = leaf ([320, D] table).  The kernel time
of (a) is read once more from the library's own event timer, outside the timed window.

--map-only: leg (a) alone, for the -DOGS_EXPERIMENTS variant builds named by OGS_LIB_PATH: another block width
(-DOGS_FEATURE_MAP_DB=32 / 64 / 128) or the ablations whose maps are wrong by construction (OGS_FMAP_WALK_ONLY,
OGS_FMAP_NO_STORE).
--merge FILE...: no measurement; folds the --map-only results of such runs into --out under "variant_builds".
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_map_bench.json"))
    ap.add_argument("--map-only", action="store_true")
    ap.add_argument("--channels", type=int, nargs="*", default=list(CHANNELS))
    ap.add_argument("--merge", nargs="*", default=[])
    args = ap.parse_args()
    if args.merge:
        with open(args.out) as fh:
            out = json.load(fh)
        builds = out.setdefault("variant_builds", {})
        for path in args.merge:
            with open(path) as fh:
                v = json.load(fh)
            builds[v["library"]] = dict(block_columns=v["block_columns"], cases={
                k: dict(wall_ms_median=c["wall_ms"]["feature_map"]["median"],
                        wall_ms_median_channels_last=c["wall_ms"]["feature_map_channels_last"]["median"],
                        kernel_ms=c["kernels_ms"]["feature_map_kernel"],
                        kernel_ms_channels_last=c["kernels_ms_channels_last"]["feature_map_kernel"]) for k, c in v["cases"].items()})
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("merged", len(args.merge), "variant builds into", args.out)
        return
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    P, W, H, f, K, C = 500_000, 988, 731, 800.0, 320, 12
    sc = make_scene(P, W, H, f, f, seed=0).to(dev)
    cam = make_camera(W, H, f, f).to(dev)
    g = torch.Generator().manual_seed(0)
    leaf = torch.randint(0, K, (P,), generator=g).to(dev)
    rs = R.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        bg=torch.zeros(C, device=dev), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=0, campos=cam.camera_center, prefiltered=False, debug=False)
    sink: list = []
    with torch.no_grad():
        R._RasterizeGaussians.apply(sc.means3D, torch.zeros_like(sc.means3D), None, torch.zeros(P, C, device=dev), sc.opacities,
                                    sc.scales, sc.rotations, None, rs, 0, None, None, 1, sink)
    kp = R.KeptPasses(budget_bytes=8 << 30)
    assert sink and kp.admit("view", "key", None, sink[0])
    entry = kp.slots["view"]
    del sink
    unit_cols = torch.rand(P, C, generator=torch.Generator().manual_seed(1)).to(dev)

    def reblend():
        with torch.no_grad():
            return R._ReblendKept.apply(unit_cols, entry, rs)[0]

    results = {}
    for D in args.channels:
        launches = (D + C - 1) // C
        for rows_name, rows, Rn in (("none", None, P), ("leaf", leaf.to(torch.int32), K)):
            X = torch.randn(Rn, D, generator=torch.Generator().manual_seed(100 + D)).to(dev)

            def fmap(channels_last=False):
                return R.feature_map(entry, X, rows=rows, channels_last=channels_last)

            legs = {"feature_map": fmap, "feature_map_channels_last": lambda: fmap(True)}
            slices = None
            if not args.map_only:
                # leg (b): the per-Gaussian features, cut into contiguous [P, 12] slices (zero padded) outside the window
                Xp = X if rows is None else X[leaf]
                slices = []
                for c0 in range(0, D, C):
                    s = torch.zeros(P, C, device=dev)
                    s[:, :min(C, D - c0)] = Xp[:, c0:c0 + C]
                    slices.append(s)
                gathered_bytes = 0 if rows is None else Xp.numel() * 4
                del Xp

                def route():
                    out = torch.empty(D, H, W, device=dev)
                    with torch.no_grad():
                        for i, s in enumerate(slices):
                            n = min(C, D - i * C)
                            out[i * C:i * C + n] = R._ReblendKept.apply(s, entry, rs)[0][:n]
                    return out

                legs.update(reblend_route=route, reblend=reblend)
            res = alternate(legs)
            rec = {"wall_ms": res, "kernels_ms": kernel_ms(fmap), "kernels_ms_channels_last": kernel_ms(lambda: fmap(True))}
            if not args.map_only:
                a, b = fmap(), route()
                va, vl, vb = res["feature_map"], res["feature_map_channels_last"], res["reblend_route"]
                rec.update(route_launches=launches,
                           route_over_feature_map=round(vb["median"] / va["median"], 2),
                           feature_map_over_reblend=round(va["median"] / res["reblend"]["median"], 2),
                           every_repeat_faster=bool(max(va["max"], vl["max"]) < vb["min"]),
                           max_difference_of_the_two_maps=float((a - b).abs().max()),
                           maps_equal=bool(torch.equal(a, b)),
                           channels_last_equal=bool(torch.equal(fmap(True).permute(2, 0, 1), a)),
                           map_bytes=4 * D * H * W,
                           extra_memory_bytes={"feature_map": 4 * Rn * D,
                                               "reblend_route": 4 * P * C * launches + gathered_bytes + 4 * (C + 2) * W * H,
                                               "reblend_route_gathered_X_rows": gathered_bytes})
                del a, b
            results[f"D{D}_rows_{rows_name}"] = rec
            print(f"D{D}_rows_{rows_name}", json.dumps(rec), flush=True)
            del X, slices, legs
            torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_properties(0).name, "ogs_version": int(_lib.lib().ogs_version()), "repeats": REPEATS,
           "library": os.path.basename(os.environ.get("OGS_LIB_PATH", "default")),
           "block_columns": int(_lib.lib().ogs_feature_map_block_columns()),
           "scene": dict(P=P, W=W, H=H, leaves=K, kept_records=int(entry.D), kept_channels=C), "cases": results}
    if not args.map_only:
        big = [k for k in results if k.startswith(("D64_", "D512_"))]
        out["acceptance_every_repeat_faster_at_D64_and_D512"] = bool(big) and all(results[k]["every_repeat_faster"] for k in big)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
