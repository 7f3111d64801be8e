"""knn.query / knn.Index against what they replace.

    python scripts/knn_query_bench.py [--out profiles/knn_query_bench.json] [--shape NAME ...]

Shapes (reference rows n, query rows m, K):
    uniform_k1, uniform_k16   n = m = 500 k, two differently seeded uniform clouds
    scannet_k1                n = 2 M, m = 200 k: GT vertices asking a densified model for their nearest Gaussian
    clustered_k16             n = m = 500 k, the reference in two tight clusters plus a few outliers, the queries uniform over their span
    outside_k16               n = m = 500 k, the queries in a cube wholly outside the reference's bounding box

Legs of a shape, alternating in ONE process, RUNS repeats each:
    query_ms        knn.query(ref, q, K): index build + search
    search_ms       index.query(q, K) on an index built once
    torch_ms        torch.cdist + topk over chunks of query rows sized to a 1 GiB distance buffer (the only route before); its
                    lists are compared with the kernel's on a sample, so a wrong baseline is reported as wrong
    neighbors_ms    knn.neighbors(ref, K, exclude_self=False) at the same n and K: the one-set search the query is built from
                    (where m != n it is the search of n rows among themselves, for scale only)

A leg is warmed up and timed by a host clock around calls that end in a device synchronise, long enough (>= 0.3 s or 200 calls)
to be above the scheduler's noise.  Without --shape every shape runs in a child process of its own under a time limit, and the
first one that fails ends the run.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = 3
TORCH_BUFFER_BYTES = 1 << 30
SAMPLE = 2048
SHAPE_LIMIT_S = 420
SHAPES = ("uniform_k1", "uniform_k16", "scannet_k1", "clustered_k16", "outside_k16")


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
    return round((time.perf_counter() - t0) / calls * 1e3, 4)


def alternate(legs):
    """{name: [ms per repeat]} with the legs interleaved repeat by repeat"""
    res = {name: [] for name in legs}
    for _ in range(RUNS):
        for name, fn in legs.items():
            res[name].append(leg_ms(fn))
            print(f"  {name} {res[name][-1]}", flush=True)
    return res


def uniform(n, seed, dev):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)).to(dev)


def sets_of(shape, dev):
    if shape.startswith("uniform"):
        return uniform(500000, 1, dev), uniform(500000, 2, dev)
    if shape.startswith("scannet"):
        return uniform(2000000, 3, dev), uniform(200000, 4, dev)
    if shape.startswith("outside"):
        return uniform(500000, 5, dev), uniform(500000, 6, dev) * 0.1 + torch.tensor([5.0, -3.0, 2.0], device=dev)
    g = torch.Generator().manual_seed(7)
    n, outliers = 500000, 40
    a = torch.randn((n - outliers) // 2, 3, generator=g) * 0.05
    b = torch.randn(n - outliers - len(a), 3, generator=g) * 0.05 + torch.tensor([40.0, -25.0, 10.0])
    o = torch.rand(outliers, 3, generator=g) * 400.0 - 200.0
    ref = torch.cat([a, b, o])[torch.randperm(n, generator=g)]
    lo, hi = torch.tensor([-5.0, -30.0, -5.0]), torch.tensor([45.0, 5.0, 15.0])
    return ref.to(dev), (lo + torch.rand(n, 3, generator=g) * (hi - lo)).to(dev)


def torch_route(ref, q, K, chunk):
    """(idx int64 [m, K], distance fp32 [m, K]) by cdist + topk over chunks of `chunk` query rows"""
    idx = torch.empty((q.shape[0], K), dtype=torch.int64, device=q.device)
    dist = torch.empty((q.shape[0], K), dtype=torch.float32, device=q.device)
    for r0 in range(0, q.shape[0], chunk):
        d, i = torch.cdist(q[r0:r0 + chunk], ref).topk(K, dim=1, largest=False)
        idx[r0:r0 + chunk], dist[r0:r0 + chunk] = i, d
    return idx, dist


def run_shape(shape, dev):
    from opengaussian_amd import knn
    K = int(shape.rsplit("_k", 1)[1])
    ref, q = sets_of(shape, dev)
    n, m = ref.shape[0], q.shape[0]
    chunk = max(1, TORCH_BUFFER_BYTES // (4 * n))
    index = knn.Index(ref)
    r = dict(shape=shape, n=n, m=m, K=K, torch_chunk_rows=chunk, torch_buffer_bytes=chunk * n * 4,
             **alternate({"query_ms": lambda: knn.query(ref, q, K), "search_ms": lambda: index.query(q, K),
                          "torch_ms": lambda: torch_route(ref, q, K, chunk),
                          "neighbors_ms": lambda: knn.neighbors(ref, K, exclude_self=False)}))
    r["every_query_repeat_below_every_torch_repeat"] = max(r["query_ms"]) < min(r["torch_ms"])
    r["query_over_neighbors"] = round(float(np.median(r["query_ms"]) / np.median(r["neighbors_ms"])), 3)
    r["search_over_neighbors"] = round(float(np.median(r["search_ms"]) / np.median(r["neighbors_ms"])), 3)
    r["torch_over_query"] = round(float(np.median(r["torch_ms"]) / np.median(r["query_ms"])), 2)
    # the baseline's lists on a sample of query rows against the kernel's (exact by contract, tests/test_37d_knn_query_gpu.py)
    rows = torch.randperm(m, generator=torch.Generator().manual_seed(9))[:SAMPLE].to(dev)
    ki, kd2 = index.query(q[rows], K)
    ti, td = torch_route(ref, q[rows], K, chunk)
    r["torch_sample_rows"] = int(rows.numel())
    r["torch_rows_with_the_kernels_list"] = int((ti == ki.long()).all(1).sum())
    r["torch_max_abs_distance_error"] = float((td.double() - kd2.double().sqrt()).abs().max())
    r["torch_max_distance"] = float(kd2.double().sqrt().max())
    torch.cuda.synchronize()
    peak0 = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    knn.query(ref, q, K)
    torch.cuda.synchronize()
    r["query_peak_bytes"] = int(torch.cuda.max_memory_allocated() - peak0)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_query_bench.json"))
    ap.add_argument("--shape", nargs="*", default=None)
    args = ap.parse_args()
    if args.shape is None:                                          # the driver: one child per shape, each under a time limit
        parts = []
        with tempfile.TemporaryDirectory() as td:
            for shape in SHAPES:
                part = os.path.join(td, shape + ".json")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", shape, "--out", part], check=True,
                               timeout=SHAPE_LIMIT_S)
                parts.append(json.load(open(part)))
        out = dict(parts[0], shapes=[r for p in parts for r in p["shapes"]])
        s500 = [r for r in out["shapes"] if r["n"] == 500000 and r["m"] == 500000]
        out["acceptance_query_below_torch_at_every_500k_shape"] = all(r["every_query_repeat_below_every_torch_repeat"] for r in s500)
    else:
        from opengaussian_amd import _lib
        assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to measure without one"
        dev = torch.device("cuda:0")
        out = {"device": torch.cuda.get_device_properties(0).name, "ogs_version": int(_lib.lib().ogs_version()),
               "lib": os.path.basename(_lib.LIB_PATH), "runs": RUNS, "box_points": int(_lib.lib().ogs_knn_box_points()), "shapes": []}
        for shape in args.shape:
            out["shapes"].append(run_shape(shape, dev))
            print(json.dumps(out["shapes"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
