"""The kNN outlier filter of render(post_process=True): knn.outlier_mask (one HIP launch, no n x n buffer) against
renderer._knn_mean_filter (the torch stand-in render() used before: cdist + topk, one call per leaf), and knn.distCUDA2
against the scipy KDTree form the reference runs on the host.

    python scripts/knn_filter_bench.py [--out profiles/knn_filter_bench.json] [--only-new]

Both paths alternate in ONE process, three runs each, medians reported; every leg is warmed up and timed by a host clock
around work that ends in a device synchronise, long enough (>= 0.3 s or 200 calls) to be above the scheduler's noise.
--only-new times the kernel path alone (A-B of kernel builds through OGS_LIB_PATH).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opengaussian_amd import _lib, knn                     # noqa: E402
from opengaussian_amd import renderer as R                  # noqa: E402

RUNS = 3
ONE_GROUP = (5000, 20000, 50000)
GROUPS, GROUP_SIZE = 640, 300


def leg_ms(fn, min_s=0.3, max_calls=200):
    """milliseconds per call of fn over one timed leg (after a warm-up call that also sizes the leg)"""
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    once = time.perf_counter() - t0
    calls = int(min(max_calls, max(1, np.ceil(min_s / max(once, 1e-6)))))
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3, calls


def alternate(new, parent):
    res = {"new_ms": [], "parent_ms": []}
    for _ in range(RUNS):
        ms, calls = leg_ms(new)
        res["new_ms"].append(round(ms, 4)); res["new_calls_per_leg"] = calls
        if parent is not None:
            ms, calls = leg_ms(parent)
            res["parent_ms"].append(round(ms, 4)); res["parent_calls_per_leg"] = calls
    res["new_ms_median"] = statistics.median(res["new_ms"])
    if parent is not None:
        res["parent_ms_median"] = statistics.median(res["parent_ms"])
        res["spread_ms"] = round(max(max(v) - min(v) for v in (res["new_ms"], res["parent_ms"])), 4)
        res["new_below_parent"] = res["new_ms_median"] < res["parent_ms_median"]
    else:
        del res["parent_ms"]
    return res


def leafwise_parent(points, group):
    """the loop render() ran before: a read-back for the leaf list, a nonzero and an n x n matrix per leaf"""
    keep = torch.zeros_like(group, dtype=torch.bool)
    for g in torch.unique(group[group >= 0]).tolist():
        rows = torch.nonzero(group == g).flatten()
        keep[rows] = R._knn_mean_filter(points[rows])
    return keep


def parent_distance_error(points, chunk=1024):
    """largest |cdist(...)**2 - d2| of the stand-in's distance matrix against fp32 direct differences, row chunk by row chunk"""
    worst = 0.0
    for c0 in range(0, points.shape[0], chunk):
        d2 = torch.cdist(points, points, compute_mode="donot_use_mm_for_euclid_dist")[c0:c0 + chunk] ** 2
        diff = points[c0:c0 + chunk, None, :] - points[None, :, :]
        worst = max(worst, float((d2 - (diff * diff).sum(-1)).abs().max()))
    return worst


def scipy_dist(points_np):
    from scipy.spatial import KDTree
    d, _ = KDTree(points_np).query(points_np, k=4)
    return (d[:, 1:] ** 2).mean(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_filter_bench.json"))
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(ONE_GROUP))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(0)
    out = {"device": prop.name, "ogs_version": int(_lib.lib().ogs_version()), "lib": os.path.basename(_lib.LIB_PATH), "runs": RUNS,
           "one_group": [], "passes_per_call": 32}
    g = torch.Generator().manual_seed(0)
    for n in args.sizes:
        pts = torch.rand(n, 3, generator=g).to(dev)
        parent = None if args.only_new else (lambda: R._knn_mean_filter(pts))
        res = alternate(lambda: knn.outlier_mask(pts), parent)
        res["n"], res["K"] = n, int(n ** 0.5)
        res["new_pair_passes_per_s"] = round(32.0 * n * n / (res["new_ms_median"] * 1e-3), 0)
        if parent is not None:
            a, b = knn.outlier_mask(pts), R._knn_mean_filter(pts)
            res["masks_differ_rows"] = int((a != b).sum())
            res["parent_matrix_bytes"] = 4 * n * n
            res["parent_distance_max_abs_error"] = parent_distance_error(pts)
            if n <= 5000:                                # which of the two is right: the NumPy restatement decides
                from tests import knn_restatement
                want = torch.from_numpy(knn_restatement.outlier_mask(pts.cpu().numpy())).to(dev)
                res["new_differs_from_restatement_rows"] = int((a != want).sum())
                res["parent_differs_from_restatement_rows"] = int((b != want).sum())
            del a, b
        out["one_group"].append(res)
        print(json.dumps(res), flush=True)
        del pts
        torch.cuda.empty_cache()
    if not args.only_new:
        n = GROUPS * GROUP_SIZE
        sizes = torch.randint(GROUP_SIZE - 100, GROUP_SIZE + 101, (GROUPS,), generator=g)
        group = torch.repeat_interleave(torch.arange(GROUPS), sizes)
        group = group[torch.randperm(group.numel(), generator=g)].to(dev)
        pts = (torch.rand(group.numel(), 3, generator=g) + torch.rand(GROUPS, 3, generator=g)[group.cpu()] * 10).to(dev)
        res = alternate(lambda: knn.outlier_mask(pts, group, GROUPS), lambda: leafwise_parent(pts, group))
        res["groups"], res["rows"] = GROUPS, int(group.numel())
        res["masks_differ_rows"] = int((knn.outlier_mask(pts, group, GROUPS) != leafwise_parent(pts, group)).sum())
        out["many_groups"] = res
        print(json.dumps(res), flush=True)
        # the stand-in's n x n fp32 matrix against the device memory: arithmetic, nothing is allocated
        n = 5000
        while 4 * n * n <= prop.total_memory // 4:
            n *= 2
        out["parent_matrix_exceeds_quarter_of_memory_at_n"] = {"n": n, "matrix_bytes": 4 * n * n,
                                                               "device_bytes": int(prop.total_memory)}
        # distCUDA2
        n = 100000
        pts = torch.rand(n, 3, generator=g)
        p_dev = pts.to(dev)
        ms = [leg_ms(lambda: knn.distCUDA2(p_dev))[0] for _ in range(RUNS)]
        d = {"n": n, "new_ms": [round(v, 4) for v in ms], "new_ms_median": round(statistics.median(ms), 4)}
        try:
            host = []
            for _ in range(RUNS):
                t0 = time.perf_counter(); want = scipy_dist(pts.numpy()); host.append(round((time.perf_counter() - t0) * 1e3, 2))
            got = knn.distCUDA2(p_dev).cpu().numpy().astype(np.float64)
            d.update(scipy_host_ms=host, scipy_host_ms_median=statistics.median(host),
                     max_rel_diff=float(np.max(np.abs(got - want) / want)))
        except ImportError:
            d["scipy_host_ms"] = "not measured (scipy missing)"
        out["distCUDA2"] = d
        print(json.dumps(d), flush=True)
    ref = [r for r in out["one_group"] if r["n"] == 20000 and "parent_ms_median" in r]
    if ref:
        out["new_below_parent_at_20000"] = ref[0]["new_below_parent"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
