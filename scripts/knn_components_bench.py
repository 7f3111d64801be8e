"""knn.components / query.segment_instances against what they replace.

    python scripts/knn_components_bench.py [--out profiles/knn_components_bench.json] [--sizes 500000 2000000]

Tables: knn.neighbors(K = 16) over the means of a synthetic.make_scene scene, 500 k and 2 M rows.  Per table four workloads:
labels = 20 classes / 320 leaves (every row takes the nearest of that many seeded centres, so labels are spatially coherent the way
classes and leaves are), each with a THRESHOLD (the median distance to the second neighbour: below the percolation point, many
small components) and WITHOUT one (a few giant components per label: every hook lands on the same few roots).

Timed per workload, in ONE process, the legs alternating, RUNS repeats each, every repeat kept:
  components_ms         the knn.components call alone (table given)
  segment_instances_ms  query.segment_instances with its knn.neighbors call and its one read-back
  torch_ms              (a) a torch composition on the GPU: edge list by boolean masks, then min-label propagation both ways with
                        scatter_reduce(amin) plus two pointer jumps per round, looped until a round changes nothing; its
                        read-backs (the mask sizes, the `unchanged` test of every round) are part of it
  scipy_ms              (b) scipy.sparse.csgraph.connected_components on the host, the copy of the table down and of the labels
                        up included; one call per repeat; left out where scipy cannot be imported
Before any time is printed both comparators must give the kernel's partition (compared through the smallest member of every
row's component).  A leg is warmed up and timed by a host clock around calls that end in a device synchronise, long enough
(>= 0.3 s or 200 calls) to be above the scheduler's noise."""
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
K = 16

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
except ImportError:                                                 # comparator (b) is optional
    connected_components = None


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
    return res


def nearest_centre_labels(pts, L, seed):
    g = torch.Generator().manual_seed(seed)
    centres = pts[torch.randperm(pts.shape[0], generator=g)[:L].to(pts.device)]
    out = torch.empty(pts.shape[0], dtype=torch.int32, device=pts.device)
    for r0 in range(0, pts.shape[0], 1 << 18):
        out[r0:r0 + (1 << 18)] = torch.cdist(pts[r0:r0 + (1 << 18)], centres).argmin(1).to(torch.int32)
    return out


def edge_mask(idx, d2, max_d2, labels):
    n = idx.shape[0]
    j = idx.long()
    ok = (j >= 0) & (j < n)
    if max_d2 is not None:
        ok &= d2 <= max_d2
    lj = labels[j.clamp(0, n - 1)]
    return ok & (labels[:, None] >= 0) & (lj == labels[:, None])


def torch_components(idx, d2, max_d2, labels):
    """min member row of every row's component, int64 [n] (an inactive row keeps itself)"""
    n, k = idx.shape
    ok = edge_mask(idx, d2, max_d2, labels)
    src = torch.arange(n, device=idx.device).repeat_interleave(k)[ok.reshape(-1)]
    dst = idx.reshape(-1)[ok.reshape(-1)].long()
    lab = torch.arange(n, device=idx.device)
    rounds = 0
    while True:
        new = lab.scatter_reduce(0, dst, lab[src], "amin").scatter_reduce(0, src, lab[dst], "amin")
        new = new[new]
        new = new[new]
        rounds += 1
        if torch.equal(new, lab):
            return lab, rounds
        lab = new


def scipy_components(idx, d2, max_d2, labels):
    """the same on the host, copies included: min member row per row, as a device tensor"""
    n, k = idx.shape
    i, d, l = idx.cpu().numpy().astype(np.int64), d2.cpu().numpy(), labels.cpu().numpy()
    ok = (i >= 0) & (i < n)
    if max_d2 is not None:
        ok &= d <= np.float32(max_d2)
    ok &= (l[:, None] >= 0) & (l[np.clip(i, 0, n - 1)] == l[:, None])
    rows = np.repeat(np.arange(n), k)[ok.reshape(-1)]
    cols = i.reshape(-1)[ok.reshape(-1)]
    C, lab = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n)).tocsr(), directed=False)
    smallest = np.full(C, n, np.int64)
    np.minimum.at(smallest, lab, np.arange(n))
    return torch.from_numpy(smallest[lab]).to(idx.device)


def workload(name, pts, idx, d2, labels, max_d2, L):
    n = idx.shape[0]
    comp, count, sizes, first = knn.components(idx, d2, max_d2, labels)
    active = comp >= 0
    smallest = first[comp.clamp_min(0).long()].long()
    C = int(count)
    r = dict(workload=name, n=n, K=K, labels=L, max_d2=max_d2, components=C, largest=int(sizes.max()),
             singletons=int((sizes[:C] == 1).sum()) if C else 0)
    again = knn.components(idx, d2, max_d2, labels)
    r["kernel_same_bytes_twice"] = bool(all(torch.equal(a, b) for a, b in zip(again, (comp, count, sizes, first))))
    tlab, rounds = torch_components(idx, d2, max_d2, labels)
    r["torch_rounds"] = rounds
    r["torch_same_partition"] = bool(torch.equal(tlab[active], smallest[active]))
    assert r["torch_same_partition"] and r["kernel_same_bytes_twice"], r
    legs = {"components_ms": lambda: knn.components(idx, d2, max_d2, labels),
            "torch_ms": lambda: torch_components(idx, d2, max_d2, labels)}
    single = ()
    if connected_components is not None:
        r["scipy_same_partition"] = bool(torch.equal(scipy_components(idx, d2, max_d2, labels)[active], smallest[active]))
        assert r["scipy_same_partition"], r
        legs["scipy_ms"] = lambda: scipy_components(idx, d2, max_d2, labels)
        single = ("scipy_ms",)
    max_dist = None if max_d2 is None else float(np.sqrt(np.float64(max_d2)))
    legs["segment_instances_ms"] = lambda: query.segment_instances(pts, labels, k=K, max_dist=max_dist)
    legs["neighbors_ms"] = lambda: knn.neighbors(pts, K)
    r.update(alternate(legs, single))
    r["every_components_repeat_below_every_torch_repeat"] = max(r["components_ms"]) < min(r["torch_ms"])
    r["every_torch_repeat_below_every_components_repeat"] = max(r["torch_ms"]) < min(r["components_ms"])
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_components_bench.json"))
    ap.add_argument("--sizes", nargs="*", type=int, default=[500000, 2000000])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_properties(0).name, "ogs_version": int(_lib.lib().ogs_version()),
           "lib": os.path.basename(_lib.LIB_PATH), "runs": RUNS, "scipy": connected_components is not None, "rows": []}
    for n in args.sizes:
        pts = synthetic.make_scene(n, 800, 800, 700.0, 700.0, seed=1).means3D.to(torch.float32).to(dev)
        idx, d2 = knn.neighbors(pts, K)
        thr = float(d2[:, 1].median())
        for L in (20, 320):
            labels = nearest_centre_labels(pts, L, L)
            for name, max_d2 in (("threshold", thr), ("no threshold", None)):
                out["rows"].append(workload(name, pts, idx, d2, labels, max_d2, L))
                torch.cuda.empty_cache()
        del pts, idx, d2
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
