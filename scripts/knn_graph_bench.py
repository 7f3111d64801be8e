"""knn.reverse_edges / knn.gather_sum / query.neighbor_smoothness against the torch compositions they replace.

    python scripts/knn_graph_bench.py [--out profiles/knn_graph_bench.json] [--part a b c]

(a) knn.reverse_edges at K = 16, n = 500 k and 2 M: built once per graph, nothing to compare it with.
(b) knn.gather_sum forward + backward (gradients of X and w, the reverse lists given) against torch autograd of
    (w[..., None] * X[idx]).sum(1), P = 500 k, K = 16, D = 6, 64, 512; the torch route is chunked over rows where its
    [rows, K, D] buffer would pass 2 GiB.  The largest difference between the two routes' gradients is recorded.  Beside the
    even graph a SKEWED one: the same 500 k x 16 slots pointing into a table of 320 rows (rows -> leaves), so every reverse list
    has about 25 000 slots and is summed in chunks.
(c) query.neighbor_smoothness forward + backward (gradients of F and w) against the torch composition
    (w * ((F[:, None] - F[idx]) ** 2).sum(-1)).mean(), 2 M x 16 at D = 6 and 500 k x 16 at D = 64, chunked the same way.

Clouds: the means of a synthetic.make_scene scene and a uniform one.  The legs alternate in ONE process, RUNS repeats each; a
leg is warmed up and timed by a host clock around calls that end in a device synchronise, long enough (>= 0.3 s or 200 calls)
to be above the scheduler's noise.  Every repeat is kept."""
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


def graph(kind, n, K, dev):
    pts = cloud(kind, n, dev)
    idx, d2 = knn.neighbors(pts, K)
    return idx, query.neighbor_weights(d2, idx)


def rand(shape, seed, dev):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def chunk_rows(n, K, D):
    return min(n, max(1, TORCH_BUFFER_LIMIT // (K * D * 4)))


def degree_stats(begin):
    deg = (begin[1:] - begin[:-1]).to(torch.float64)
    return dict(in_degree_max=int(deg.max()), in_degree_median=float(deg.median()), rows_without_in_edge=int((deg == 0).sum()))


def part_a(dev, out):
    rows = []
    for n in (500000, 2000000):
        for kind in ("scene", "uniform"):
            idx, _ = graph(kind, n, 16, dev)
            r = dict(cloud=kind, n=n, K=16, **alternate({"reverse_edges_ms": lambda: knn.reverse_edges(idx)}))
            r.update(degree_stats(knn.reverse_edges(idx)[0]))
            rows.append(r)
            print(json.dumps(r), flush=True)
            del idx
            torch.cuda.empty_cache()
    out["reverse_edges"] = rows


def kernel_gather(X, idx, w, G, reverse):
    X.grad = w.grad = None
    knn.gather_sum(X, idx, w, reverse).backward(G)
    return X.grad, w.grad


def torch_gather(X, idx64, w, G, chunk):
    X.grad = w.grad = None
    for r0 in range(0, idx64.shape[0], chunk):
        (w[r0:r0 + chunk, :, None] * X[idx64[r0:r0 + chunk]]).sum(1).backward(G[r0:r0 + chunk])
    return X.grad, w.grad


def gather_row(name, idx, w, R, D, dev):
    n, K = idx.shape
    idx64 = idx.long()
    reverse = knn.reverse_edges(idx, R)
    X, G = rand((R, D), D, dev).requires_grad_(True), rand((n, D), D + 1, dev)
    wg = w.clone().requires_grad_(True)
    chunk = chunk_rows(n, K, D)
    r = dict(graph=name, n=n, K=K, R=R, D=D, torch_chunk_rows=chunk, torch_buffer_bytes=chunk * K * D * 4,
             torch_whole_buffer_bytes=n * K * D * 4, **degree_stats(reverse[0]),
             **alternate({"gather_sum_ms": lambda: kernel_gather(X, idx, wg, G, reverse),
                          "torch_ms": lambda: torch_gather(X, idx64, wg, G, chunk)}))
    r["every_gather_sum_repeat_below_every_torch_repeat"] = max(r["gather_sum_ms"]) < min(r["torch_ms"])
    r["every_torch_repeat_below_every_gather_sum_repeat"] = max(r["torch_ms"]) < min(r["gather_sum_ms"])
    kx, kw = (g.clone() for g in kernel_gather(X, idx, wg, G, reverse))
    tx, tw = torch_gather(X, idx64, wg, G, chunk)
    r["grad_X_max_abs_diff"], r["grad_X_max_abs"] = float((kx - tx).abs().max()), float(tx.abs().max())
    r["grad_w_max_abs_diff"], r["grad_w_max_abs"] = float((kw - tw).abs().max()), float(tw.abs().max())
    kx2, kw2 = kernel_gather(X, idx, wg, G, reverse)
    r["kernel_gradients_same_bytes_twice"] = bool(torch.equal(kx, kx2) and torch.equal(kw, kw2))
    tx2 = torch_gather(X, idx64, wg, G, chunk)[0].clone()
    r["torch_grad_X_same_bytes_twice"] = bool(torch.equal(tx2, torch_gather(X, idx64, wg, G, chunk)[0]))
    print(json.dumps(r), flush=True)
    return r


def part_b(dev, out):
    P, K = 500000, 16
    rows = []
    for kind in ("scene", "uniform"):
        idx, w = graph(kind, P, K, dev)
        for D in (6, 64, 512):
            rows.append(gather_row(kind, idx, w, P, D, dev))
            torch.cuda.empty_cache()
    leaves = torch.randint(0, 320, (P, K), generator=torch.Generator().manual_seed(5)).to(torch.int32).to(dev)
    for D in (6, 64):
        rows.append(gather_row("skewed: 320 leaves", leaves, w, 320, D, dev))
        torch.cuda.empty_cache()
    out["gather_sum_forward_backward"] = rows


def kernel_smooth(F, idx, w, reverse):
    F.grad = w.grad = None
    query.neighbor_smoothness(F, idx, w, reverse).backward()
    return F.grad, w.grad


def torch_smooth(F, idx64, w, chunk):
    F.grad = w.grad = None
    n, K = idx64.shape
    for r0 in range(0, n, chunk):
        d2 = ((F[r0:r0 + chunk, None, :] - F[idx64[r0:r0 + chunk]]) ** 2).sum(-1)
        ((w[r0:r0 + chunk] * d2).sum() / (n * K)).backward()
    return F.grad, w.grad


def part_c(dev, out):
    rows = []
    for n, D in ((2000000, 6), (500000, 64)):
        for kind in ("scene", "uniform"):
            K = 16
            idx, w = graph(kind, n, K, dev)
            idx64 = idx.long()
            reverse = knn.reverse_edges(idx)
            F = rand((n, D), D, dev).requires_grad_(True)
            wg = w.clone().requires_grad_(True)
            chunk = chunk_rows(n, K, D)
            r = dict(cloud=kind, n=n, K=K, D=D, torch_chunk_rows=chunk, torch_buffer_bytes=chunk * K * D * 4,
                     **alternate({"neighbor_smoothness_ms": lambda: kernel_smooth(F, idx, wg, reverse),
                                  "torch_ms": lambda: torch_smooth(F, idx64, wg, chunk)}))
            r["every_kernel_repeat_below_every_torch_repeat"] = max(r["neighbor_smoothness_ms"]) < min(r["torch_ms"])
            r["every_torch_repeat_below_every_kernel_repeat"] = max(r["torch_ms"]) < min(r["neighbor_smoothness_ms"])
            kf, kw = (g.clone() for g in kernel_smooth(F, idx, wg, reverse))
            tf, tw = torch_smooth(F, idx64, wg, chunk)
            r["grad_F_max_abs_diff"], r["grad_F_max_abs"] = float((kf - tf).abs().max()), float(tf.abs().max())
            r["grad_w_max_abs_diff"], r["grad_w_max_abs"] = float((kw - tw).abs().max()), float(tw.abs().max())
            rows.append(r)
            print(json.dumps(r), flush=True)
            del idx, idx64, w, wg, F, reverse
            torch.cuda.empty_cache()
    out["neighbor_smoothness_forward_backward"] = rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_graph_bench.json"))
    ap.add_argument("--part", nargs="*", default=["a", "b", "c"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_properties(0).name, "ogs_version": int(_lib.lib().ogs_version()),
           "lib": os.path.basename(_lib.LIB_PATH), "runs": RUNS, "chunk": int(_lib.lib().ogs_knn_transpose_chunk())}
    parts = {"a": part_a, "b": part_b, "c": part_c}
    for p in args.part:
        parts[p](dev, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
