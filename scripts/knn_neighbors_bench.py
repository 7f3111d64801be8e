"""knn.neighbors / knn.aggregate against what they replace.

    python scripts/knn_neighbors_bench.py [--out profiles/knn_neighbors_bench.json] [--part a b c]

(a) distCUDA2(route="boxes") against route="brute" (the 32-pass threshold kernel, the only route before), n doubling from
    1 000 to 128 000, plus 100 000 and 200 000, on a uniform cloud and on the means of a synthetic.make_scene scene; boxes alone at 500 k, 1 M, 2 M.
    The switch of route=None is the smallest n of the sweep from which EVERY repeat of boxes beats EVERY repeat of brute at that
    and every larger n, on both clouds.
(b) knn.neighbors at K = 16, n = 500 k and 2 M.
(c) knn.aggregate against the torch composition (w[..., None] * X[idx]).sum(1), P = 500 k, K = 16, D = 6, 64, 512; the torch
    route is chunked over rows where its [rows, K, D] buffer would pass 2 GiB, and the buffer's bytes are recorded.

The legs alternate in ONE process, RUNS repeats each; a leg is warmed up and timed by a host clock around calls that end in a
device synchronise, long enough (>= 0.3 s or 200 calls) to be above the scheduler's noise.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opengaussian_amd import _lib, knn, synthetic           # noqa: E402

RUNS = 3
SWEEP = (1000, 2000, 4000, 8000, 16000, 32000, 64000, 100000, 128000, 200000)
BOXES_ONLY = (500000, 1000000, 2000000)
TORCH_BUFFER_LIMIT = 2 << 30


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
    return res


def cloud(kind, n, dev):
    if kind == "uniform":
        return torch.rand(n, 3, generator=torch.Generator().manual_seed(n)).to(dev)
    return synthetic.make_scene(n, 800, 800, 700.0, 700.0, seed=1).means3D.to(torch.float32).to(dev)


def part_a(dev, out):
    rows = []
    for kind in ("uniform", "scene"):
        for n in SWEEP + BOXES_ONLY:
            pts = cloud(kind, n, dev)
            legs = {"boxes_ms": lambda: knn.distCUDA2(pts, route="boxes")}
            if n in SWEEP:
                legs["brute_ms"] = lambda: knn.distCUDA2(pts, route="brute")
            r = dict(cloud=kind, n=n, **alternate(legs))
            if n in SWEEP:
                r["every_boxes_repeat_below_every_brute_repeat"] = max(r["boxes_ms"]) < min(r["brute_ms"])
                a, b = knn.distCUDA2(pts, route="boxes").double(), knn.distCUDA2(pts, route="brute").double()
                r["max_rel_diff"] = float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())
            rows.append(r)
            print(json.dumps(r), flush=True)
            del pts
            torch.cuda.empty_cache()
    out["distCUDA2"] = rows
    wins = lambda n: all(r["every_boxes_repeat_below_every_brute_repeat"] for r in rows if r["n"] == n and n in SWEEP)
    switch = None
    for n in reversed(SWEEP):
        if not wins(n):
            break
        switch = n
    out["boxes_win_from_n"] = switch
    out["acceptance_every_boxes_repeat_below_every_brute_repeat_at_100000"] = wins(100000)
    out["route_none_switch_in_knn_py"] = knn.DIST_BOXES_FROM
    out["route_none_switch_note"] = ("knn.DIST_BOXES_FROM: the smallest n of the sweep above 4097 rows, the largest cloud on which "
                                     "tests/test_knn_host.py pins distCUDA2() without a route to the brute entry point; "
                                     "boxes_win_from_n is what the timings alone give")


def part_b(dev, out):
    rows = []
    for n in (500000, 2000000):
        for kind in ("uniform", "scene"):
            pts = cloud(kind, n, dev)
            r = dict(cloud=kind, n=n, K=16, **alternate({"neighbors_ms": lambda: knn.neighbors(pts, 16)}))
            rows.append(r)
            print(json.dumps(r), flush=True)
            del pts
            torch.cuda.empty_cache()
    out["neighbors_k16"] = rows


def torch_aggregate(X, idx, w, chunk):
    out = torch.empty(idx.shape[0], X.shape[1], dtype=torch.float32, device=X.device)
    for r0 in range(0, idx.shape[0], chunk):
        out[r0:r0 + chunk] = (w[r0:r0 + chunk, :, None] * X[idx[r0:r0 + chunk]]).sum(1)
    return out


def part_c(dev, out):
    P, K = 500000, 16
    pts = cloud("scene", P, dev)
    idx, d2 = knn.neighbors(pts, K)
    from opengaussian_amd import query
    w = query.neighbor_weights(d2, idx)
    idx64 = idx.long()
    rows = []
    for D in (6, 64, 512):
        X = torch.randn(P, D, generator=torch.Generator().manual_seed(D)).to(dev)
        chunk = min(P, max(1, TORCH_BUFFER_LIMIT // (K * D * 4)))
        r = dict(P=P, K=K, D=D, torch_chunk_rows=chunk, torch_buffer_bytes=chunk * K * D * 4, torch_whole_buffer_bytes=P * K * D * 4,
                 **alternate({"aggregate_ms": lambda: knn.aggregate(X, idx, w),
                              "torch_ms": lambda: torch_aggregate(X, idx64, w, chunk)}))
        r["every_aggregate_repeat_below_every_torch_repeat"] = max(r["aggregate_ms"]) < min(r["torch_ms"])
        r["max_abs_diff"] = float((knn.aggregate(X, idx, w) - torch_aggregate(X, idx64, w, chunk)).abs().max())
        rows.append(r)
        print(json.dumps(r), flush=True)
        del X
        torch.cuda.empty_cache()
    out["aggregate"] = rows
    out["acceptance_aggregate_below_torch_at_D64"] = [r for r in rows if r["D"] == 64][0]["every_aggregate_repeat_below_every_torch_repeat"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_neighbors_bench.json"))
    ap.add_argument("--part", nargs="*", default=["a", "b", "c"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_properties(0).name, "ogs_version": int(_lib.lib().ogs_version()),
           "lib": os.path.basename(_lib.LIB_PATH), "runs": RUNS, "box_points": int(_lib.lib().ogs_knn_box_points())}
    parts = {"a": part_a, "b": part_b, "c": part_c}
    for p in args.part:
        parts[p](dev, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
