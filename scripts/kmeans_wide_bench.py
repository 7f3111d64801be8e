"""kmeans.wide_lloyd / wide_assign against the torch composition a user had before them.

    python scripts/kmeans_wide_bench.py [--out profiles/kmeans_wide_bench.json] [--shape N D k ...]

Per shape (N, D, k) and metric, in ONE process on one card, the legs alternating repeat by repeat:
  wide_assign_ms      one scoring pass (ogs_kmeans_wide_assign, ids and dist)
  wide_iteration_ms   one Lloyd iteration: (wide_lloyd(iters = 2) - wide_lloyd(iters = 0)) / 2, i.e. assign + inertia + update
  torch_assign_ms     the fp32 composition's scoring pass: row-chunked  X @ C.T (+ bias), argmax
  torch_iteration_ms  that pass, then index_add_ of the rows and of ones into [k, D] / [k] and the division
The torch route is chunked over rows so that its [chunk, k] score buffer stays at or below 1 GiB.  Every call is timed with
device events after WARMUP untimed calls; every repeat is kept and min / max are reported.  Peak extra memory is
torch.cuda.max_memory_allocated over one call minus what was allocated before it.  The two routes' ids are compared, and the
torch route's centres are compared with themselves across two runs (its index_add_ uses float atomics)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opengaussian_amd import _lib, kmeans           # noqa: E402

SHAPES = [(500_000, 64, 320), (500_000, 512, 320), (500_000, 512, 1024), (2_000_000, 64, 1024)]
RUNS, WARMUP = 5, 2
SCORE_BUFFER_LIMIT = 1 << 30


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(legs):
    for fn in legs.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name in legs}
    for _ in range(RUNS):
        for name, fn in legs.items():
            res[name].append(round(event_ms(fn), 4))
    return res


def peak_extra_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def torch_assign(X, C, metric, chunk):
    bias = -0.5 * (C * C).sum(1) if metric == "l2" else None
    ids = torch.empty(X.shape[0], dtype=torch.int64, device=X.device)
    for r0 in range(0, X.shape[0], chunk):
        s = X[r0:r0 + chunk] @ C.T
        if bias is not None:
            s += bias
        ids[r0:r0 + chunk] = s.argmax(1)
    return ids


def torch_iteration(X, C, metric, chunk):
    ids = torch_assign(X, C, metric, chunk)
    sums = torch.zeros_like(C).index_add_(0, ids, X)
    counts = torch.zeros(C.shape[0], device=X.device).index_add_(0, ids, torch.ones(X.shape[0], device=X.device))
    new = torch.where(counts[:, None] > 0, sums / counts.clamp_min(1)[:, None], C)
    return torch.nn.functional.normalize(new, dim=1) if metric == "cosine" else new


def row(N, D, k, metric, dev):
    g = torch.Generator(device=dev).manual_seed(N + D + k)
    # k blobs around random directions, so that the assignment is not all near-ties
    X = torch.randn(k, D, generator=g, device=dev)[torch.randint(0, k, (N,), generator=g, device=dev)]
    X += 0.5 * torch.randn(N, D, generator=g, device=dev)
    C0 = X[torch.randperm(N, generator=g, device=dev)[:k]].clone()
    if metric == "cosine":
        C0 = torch.nn.functional.normalize(C0, dim=1)
    chunk = min(N, max(1, SCORE_BUFFER_LIMIT // (4 * k)))
    legs = {"wide_assign_ms": lambda: kmeans.wide_assign(X, C0, metric),
            "wide_lloyd0_ms": lambda: kmeans.wide_lloyd(X, C0.clone(), 0, metric),
            "wide_lloyd2_ms": lambda: kmeans.wide_lloyd(X, C0.clone(), 2, metric),
            "torch_assign_ms": lambda: torch_assign(X, C0, metric, chunk),
            "torch_iteration_ms": lambda: torch_iteration(X, C0, metric, chunk)}
    t = alternate(legs)
    t["wide_iteration_ms"] = [round((b - a) / 2, 4) for a, b in zip(t["wide_lloyd0_ms"], t["wide_lloyd2_ms"])]
    r = dict(N=N, D=D, k=k, metric=metric, torch_chunk_rows=chunk, **t)
    for name in ("wide_assign_ms", "wide_iteration_ms", "torch_assign_ms", "torch_iteration_ms"):
        r[name.replace("_ms", "_min_max_ms")] = [min(t[name]), max(t[name])]
    r["wide_tmp_bytes"] = int(_lib.lib().ogs_kmeans_wide_tmp_bytes(N, D, k))
    r["wide_lloyd_peak_extra_bytes"] = peak_extra_bytes(legs["wide_lloyd2_ms"])
    r["torch_iteration_peak_extra_bytes"] = peak_extra_bytes(legs["torch_iteration_ms"])
    wi, ti = kmeans.wide_assign(X, C0, metric)[0], torch_assign(X, C0, metric, chunk)
    r["rows_where_the_routes_differ"] = int((wi != ti).sum())
    a, b = kmeans.wide_lloyd(X, C0.clone(), 2, metric), kmeans.wide_lloyd(X, C0.clone(), 2, metric)
    r["wide_same_bytes_twice"] = bool(all(torch.equal(x, y) for x, y in zip(a, b)))
    r["torch_centres_same_bytes_twice"] = bool(torch.equal(torch_iteration(X, C0, metric, chunk), torch_iteration(X, C0, metric, chunk)))
    r["every_wide_iteration_below_every_torch"] = max(t["wide_iteration_ms"]) < min(t["torch_iteration_ms"])
    r["every_torch_iteration_below_every_wide"] = max(t["torch_iteration_ms"]) < min(t["wide_iteration_ms"])
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_wide_bench.json"))
    ap.add_argument("--shape", nargs="*", type=int, default=None, help="N D k triples instead of the standard four")
    ap.add_argument("--metric", nargs="*", default=["l2", "cosine"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    shapes = SHAPES if not args.shape else [tuple(args.shape[i:i + 3]) for i in range(0, len(args.shape), 3)]
    lib = _lib.lib()
    out = {"device": torch.cuda.get_device_properties(0).name, "ogs_version": int(lib.ogs_version()), "runs": RUNS, "warmup": WARMUP,
           "row_tile": int(lib.ogs_kmeans_wide_row_tile()), "centre_tile": int(lib.ogs_kmeans_wide_centre_tile()),
           "dim_step": int(lib.ogs_kmeans_wide_dim_step()), "rows": []}
    for N, D, k in shapes:
        for metric in args.metric:
            out["rows"].append(row(N, D, k, metric, dev))
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
