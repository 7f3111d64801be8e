"""knn.radius_count / knn.dbscan / query.segment_instances_dbscan against the walks they are built from and against scikit-learn.

    python scripts/knn_radius_bench.py [--out profiles/knn_radius_bench.json] [--sizes 500000 2000000]

Points: the means of a synthetic.make_scene scene, 500 k and 2 M rows, SNAPPED to a grid of a power of two near eps / 64, with eps
put half a grid step off a grid multiple.  Every d2 that could decide a pair is then an exact integer multiple of step^2 in fp32
and in fp64 alike and none lies closer to eps^2 than a quarter of step^2 (a relative margin of about 6e-5), so scikit-learn,
which compares in fp64, sees the pairs the fp32 kernels see.  eps starts from the median distance to the 8th neighbour
(knn.neighbors), min_pts = 8.  Three workloads per size: labels = 20 classes / 320 leaves (every row takes the nearest of that
many seeded centres) and none.

Timed per workload, in ONE process, the legs alternating, RUNS repeats each, every repeat kept:
  radius_count_ms              Index.radius_count of the set against its own index (index built before)
  dbscan_ms                    knn.dbscan whole
  dbscan_kernels               the launches of one knn.dbscan call from the library's event brackets (ms per kernel name)
  segment_instances_dbscan_ms  query.segment_instances_dbscan whole, its one read-back included (no labels: one class)
  neighbors16_ms               knn.neighbors(K = 16) on the same rows: the yardstick for one walk
  components_ms                knn.neighbors(K = 16) + knn.components under the same distance and labels: what the kNN-graph route
                               costs.  Its partition is NOT DBSCAN's (no core rule, 16 columns), so only its time is taken
  sklearn_ms                   sklearn.cluster.DBSCAN on the host (no labels only: it has no label rule), the copy of the points
                               down and of the result up included, one call per repeat; left out where it cannot be imported
Before scikit-learn's time is taken its core set, its partition of the cores and its noise set must equal the kernel's.  A leg
is warmed up and timed by a host clock around calls that end in a device synchronise, long enough (>= 0.3 s or 200 calls) to be
above the scheduler's noise."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opengaussian_amd import _lib, knn, query, synthetic           # noqa: E402

RUNS = 3
MIN_PTS = 8

try:
    from sklearn.cluster import DBSCAN
except ImportError:                                                 # the host comparator is optional
    DBSCAN = None


def leg_ms(fn, min_s=0.3, max_calls=200):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    once = time.perf_counter() - t0
    calls = int(min(max_calls, max(1, np.ceil(min_s / max(once, 1e-6)))))
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / calls * 1e3, 4)


def once_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 4)


def alternate(legs, single=()):
    res = {name: [] for name in legs}
    for _ in range(RUNS):
        for name, fn in legs.items():
            res[name].append(once_ms(fn) if name in single else leg_ms(fn))
            print("  ", name, res[name][-1], flush=True)
    return res


def nearest_centre_labels(pts, L, seed):
    g = torch.Generator().manual_seed(seed)
    centres = pts[torch.randperm(pts.shape[0], generator=g)[:L].to(pts.device)]
    out = torch.empty(pts.shape[0], dtype=torch.int32, device=pts.device)
    for r0 in range(0, pts.shape[0], 1 << 18):
        out[r0:r0 + (1 << 18)] = torch.cdist(pts[r0:r0 + (1 << 18)], centres).argmin(1).to(torch.int32)
    return out


def snap(pts, eps):
    """(points on the grid, eps half a step off the grid, step): step = the power of two nearest to eps / 64"""
    step = 2.0 ** round(np.log2(eps / 64.0))
    return torch.round(pts / step) * step, (np.floor(eps / step) + 0.5) * step, step


def canonical(labels):
    """a partition's labels renumbered by first occurrence: equal arrays mean equal partitions"""
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse]


def sklearn_dbscan(pts, eps):
    """(labels, core mask) on the host, the copies included"""
    x = pts.cpu().numpy().astype(np.float64)
    sk = DBSCAN(eps=eps, min_samples=MIN_PTS).fit(x)
    core = np.zeros(len(x), bool)
    core[sk.core_sample_indices_] = True
    return torch.from_numpy(sk.labels_).to(pts.device), torch.from_numpy(core).to(pts.device)


def kernel_times(fn):
    fn(); torch.cuda.synchronize()
    _lib.prof_enable(1)
    fn(); torch.cuda.synchronize()
    prof = _lib.prof_collect(); _lib.prof_enable(0)
    return {k: round(v["total_ms"] / max(v["calls"], 1), 4) for k, v in prof.items()}


def workload(pts, index, eps, labels, L):
    n = pts.shape[0]
    res = knn.dbscan(pts, eps, MIN_PTS, labels)
    again = knn.dbscan(pts, eps, MIN_PTS, labels)
    C = int(res.count)
    r = dict(n=n, labels=L, eps=eps, min_pts=MIN_PTS, clusters=C, cores=int(res.core.sum()), noise=int((res.cluster < 0).sum()),
             largest=int(res.sizes.max()), mean_degree=round(float(res.degree.float().mean()), 3), max_degree=int(res.degree.max()))
    r["kernel_same_bytes_twice"] = bool(all(torch.equal(a, b) for a, b in zip(again, res)))
    own = index.radius_count(pts, eps, labels, labels)
    r["radius_count_is_degree"] = bool(torch.equal(own, res.degree))
    assert r["kernel_same_bytes_twice"] and r["radius_count_is_degree"], r
    seg_labels = labels if labels is not None else torch.zeros(n, dtype=torch.int32, device=pts.device)
    legs = {"radius_count_ms": lambda: index.radius_count(pts, eps, labels, labels),
            "dbscan_ms": lambda: knn.dbscan(pts, eps, MIN_PTS, labels),
            "segment_instances_dbscan_ms": lambda: query.segment_instances_dbscan(pts, seg_labels, eps, MIN_PTS),
            "neighbors16_ms": lambda: knn.neighbors(pts, 16),
            "components_ms": lambda: knn.components(*knn.neighbors(pts, 16), max_d2=eps * eps, labels=labels)}
    single = ()
    if DBSCAN is not None and labels is None:
        print("   scikit-learn, checking", flush=True)
        sk_labels, sk_core = sklearn_dbscan(pts, eps)
        core = res.core.cpu().numpy()
        r["sklearn_same_cores"] = bool(torch.equal(sk_core, res.core))
        r["sklearn_same_noise"] = bool(torch.equal(sk_labels < 0, res.cluster < 0))
        r["sklearn_same_core_partition"] = bool(np.array_equal(canonical(sk_labels.cpu().numpy()[core]),
                                                               canonical(res.cluster.cpu().numpy()[core])))
        assert r["sklearn_same_cores"] and r["sklearn_same_noise"] and r["sklearn_same_core_partition"], r
        legs["sklearn_ms"] = lambda: sklearn_dbscan(pts, eps)
        single = ("sklearn_ms",)
    r["dbscan_kernels"] = kernel_times(lambda: knn.dbscan(pts, eps, MIN_PTS, labels))
    r.update(alternate(legs, single))
    if "sklearn_ms" in r:
        r["every_dbscan_repeat_below_every_sklearn_repeat"] = max(r["dbscan_ms"]) < min(r["sklearn_ms"])
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_radius_bench.json"))
    ap.add_argument("--sizes", nargs="*", type=int, default=[500000, 2000000])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_properties(0).name, "ogs_version": int(_lib.lib().ogs_version()),
           "lib": os.path.basename(_lib.LIB_PATH), "runs": RUNS, "sklearn": DBSCAN is not None, "rows": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for n in args.sizes:
        raw = synthetic.make_scene(n, 800, 800, 700.0, 700.0, seed=1).means3D.to(torch.float32).to(dev)
        _, d2 = knn.neighbors(raw, 8)
        pts, eps, step = snap(raw, float(d2[:, 7].median().sqrt()))
        del raw, d2
        index = knn.Index(pts)
        print(f"n={n} eps={eps} step={step}", flush=True)
        for L in (20, 320, None):
            labels = None if L is None else nearest_centre_labels(pts, L, L)
            out["rows"].append(dict(workload(pts, index, eps, labels, L), grid_step=step))
            with open(args.out, "w") as f:                          # after every workload: a cut-off run keeps what it measured
                json.dump(out, f, indent=1)
            torch.cuda.empty_cache()
        del pts, index
        torch.cuda.empty_cache()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
