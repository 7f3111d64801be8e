"""kmeans.wide_seed (exact k-means++ seeding, HIP) with and without pruning, against the torch composition a user would write.

    python scripts/kmeans_seed_bench.py [--out profiles/kmeans_seed_bench.json] [--shape N D k ...]

Data: a clustered synthetic set of unbalanced cluster sizes (k clusters, sizes proportional to 1 / rank, sigma = 0.3 about centres
4 * N(0, 1)).  Per shape (N, D, k), in ONE process on one card, the legs alternating repeat by repeat, every call timed with device
events after WARMUP untimed calls, every repeat kept:
  seed_prune_ms     wide_seed(prune=True): the whole call, k rounds
  seed_noprune_ms   wide_seed(prune=False)
  torch_seed_ms     per round ((X - c) ** 2).sum(1), minimum, cumsum, searchsorted; its draws come from torch's generator, so its
                    rows are not wide_seed's -- the same work, not the same bytes
Also: the bytes an unpruned round moves, N (4 D + 16), and the rate of the whole unpruned call over (k - 1) such rounds (launches,
picks and centre distances included: a whole-call rate, not a kernel's); the share of (row, round) pairs the bound skipped
(stats[2] / (stats[1] + stats[2])); whether prune on and off gave the same bytes; and the inertia after 10 Lloyd iterations of
query.build_codebook (L2) from init="k-means++" and from init=None."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opengaussian_amd import _lib, kmeans, query           # noqa: E402

SHAPES = [(500_000, 64, 320), (500_000, 512, 320), (500_000, 512, 1024), (2_000_000, 64, 1024)]
RUNS, WARMUP = 3, 1
LLOYD_ITERS = 10


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
            res[name].append(round(event_ms(fn), 3))
    return res


def clustered(N, D, k, dev):
    g = torch.Generator(device=dev).manual_seed(N + D + k)
    p = 1.0 / torch.arange(1, k + 1, dtype=torch.float64, device=dev)
    labels = torch.multinomial(p / p.sum(), N, replacement=True, generator=g)
    X = 4.0 * torch.randn(k, D, generator=g, device=dev)[labels]
    X += 0.3 * torch.randn(N, D, generator=g, device=dev)
    return X, labels


def torch_seed(X, k, seed):
    N, dev = X.shape[0], X.device
    g = torch.Generator(device=dev).manual_seed(seed)
    C = torch.empty(k, X.shape[1], device=dev)
    C[0] = X[torch.randint(N, (1,), generator=g, device=dev)[0]]
    d2 = ((X - C[0]) ** 2).sum(1)
    for r in range(1, k):
        cs = torch.cumsum(d2, 0)
        i = torch.searchsorted(cs, torch.rand(1, generator=g, device=dev) * cs[-1]).clamp_max(N - 1)[0]
        C[r] = X[i]
        d2 = torch.minimum(d2, ((X - C[r]) ** 2).sum(1))
    return C, d2


def row(N, D, k, dev):
    X, _ = clustered(N, D, k, dev)
    legs = {"seed_prune_ms": lambda: kmeans.wide_seed(X, k, "l2", None, 0, True),
            "seed_noprune_ms": lambda: kmeans.wide_seed(X, k, "l2", None, 0, False),
            "torch_seed_ms": lambda: torch_seed(X, k, 0)}
    t = alternate(legs)
    r = dict(N=N, D=D, k=k, **t)
    for name in legs:
        r[name.replace("_ms", "_min_max_ms")] = [min(t[name]), max(t[name])]
    on, off = legs["seed_prune_ms"](), legs["seed_noprune_ms"]()
    r["prune_on_off_same_bytes"] = bool(all(torch.equal(a, b) for a, b in zip(on[:4], off[:4])))
    stats = on[4].cpu().tolist()
    r["stats_prune"], r["stats_noprune"] = stats, off[4].cpu().tolist()
    r["pruned_share"] = round(stats[2] / max(stats[1] + stats[2], 1), 4)
    r["bytes_per_unpruned_round"] = N * (4 * D + 16)
    r["unpruned_whole_call_gb_per_s"] = round(r["bytes_per_unpruned_round"] * (k - 1) / (min(t["seed_noprune_ms"]) * 1e-3) / 1e9, 1)
    r["seed_tmp_bytes"] = int(_lib.lib().ogs_kmeans_wide_seed_tmp_bytes(N, D, k))
    inertia = lambda cb: float(cb.dist.double().sum())
    r["inertia_after_lloyd_kmeanspp"] = inertia(query.build_codebook(X, k, metric="l2", iters=LLOYD_ITERS, init="k-means++", seed=0))
    r["inertia_after_lloyd_random_rows"] = inertia(query.build_codebook(X, k, metric="l2", iters=LLOYD_ITERS, init=None, seed=0))
    r["torch_seed_inertia_before_lloyd"] = float(torch_seed(X, k, 0)[1].double().sum())
    r["wide_seed_inertia_before_lloyd"] = float(on[3].double().sum())
    r["every_prune_below_every_noprune"] = max(t["seed_prune_ms"]) < min(t["seed_noprune_ms"])
    r["every_noprune_below_every_prune"] = max(t["seed_noprune_ms"]) < min(t["seed_prune_ms"])
    r["every_prune_below_every_torch"] = max(t["seed_prune_ms"]) < min(t["torch_seed_ms"])
    r["every_torch_below_every_prune"] = max(t["torch_seed_ms"]) < min(t["seed_prune_ms"])
    r["every_torch_below_every_noprune"] = max(t["torch_seed_ms"]) < min(t["seed_noprune_ms"])
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_seed_bench.json"))
    ap.add_argument("--shape", nargs="*", type=int, default=None, help="N D k triples instead of the standard four")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    shapes = SHAPES if not args.shape else [tuple(args.shape[i:i + 3]) for i in range(0, len(args.shape), 3)]
    lib = _lib.lib()
    out = {"device": torch.cuda.get_device_properties(0).name, "ogs_version": int(lib.ogs_version()), "runs": RUNS, "warmup": WARMUP,
           "lloyd_iters": LLOYD_ITERS, "seed_rows": int(lib.ogs_kmeans_wide_seed_rows()), "rows": []}
    for N, D, k in shapes:
        out["rows"].append(row(N, D, k, dev))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
