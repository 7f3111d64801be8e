"""The neighbour lists of ``ogs_knn_neighbors`` and what is built on them, restated in NumPy.

``neighbors`` takes the fp32 distances of tests/knn_restatement.py (``sqdist_rows``: the kernel's operation order) and orders
every row by the pair (d2, j) with ``np.lexsort``; the gather-sum, the weights and the diffusion are float64.
tests/test_knn_neighbors_host.py pins this file to a per-row Python loop, tests/test_37b_knn_neighbors_gpu.py holds the kernels to
it."""
import numpy as np

from tests import knn_restatement as kr


def neighbors(points, K, exclude_self=True, rows=None, chunk=512):
    """(idx int32 [len(rows), K], d2 fp32 [len(rows), K]) of the given rows (default: all): the first K of all j (without
    j = row when exclude_self) by ascending (d2, j); slots past the end of the list hold -1 and +inf."""
    points = np.ascontiguousarray(points, dtype=np.float32)
    n = len(points)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    idx = np.full((len(rows), K), -1, np.int32)
    d2 = np.full((len(rows), K), np.inf, np.float32)
    j = np.broadcast_to(np.arange(n), (min(chunk, max(len(rows), 1)), n))
    for c0 in range(0, len(rows), chunk):
        r = rows[c0:c0 + chunk]
        d = kr.sqdist_rows(points, r)
        jj = j[:len(r)]
        order = np.lexsort((jj, d), axis=1)                           # last key first: by d2, then by j
        if exclude_self:
            order = order[order != r[:, None]].reshape(len(r), n - 1)
        order = order[:, :K]
        m = order.shape[1]
        idx[c0:c0 + len(r), :m] = order
        d2[c0:c0 + len(r), :m] = np.take_along_axis(d, order, axis=1)
    return idx, d2


def aggregate(X, idx, w):
    """(out float64 [n, D], scale float64 [n, D]): out[i] = sum_k w[i, k] * X[idx[i, k]] over the slots with 0 <= idx < R,
    and scale = sum_k |w * x| over the same slots (what an error bar of the fp32 chain is stated in)."""
    X = np.asarray(X, np.float64)
    idx = np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < len(X))
    wz = np.where(ok, np.asarray(w, np.float64), 0.0)                 # a skipped slot's weight is never a value
    g = X[np.where(ok, idx, 0)]                                       # [n, K, D]: fine at test sizes
    return (wz[..., None] * g).sum(1), (np.abs(wz)[..., None] * np.abs(g)).sum(1)


def neighbor_weights(d2, idx, valid=None, bandwidth=None):
    d2, idx = np.asarray(d2), np.asarray(idx, np.int64)
    ok = (idx >= 0) & np.isfinite(d2)
    if valid is not None:
        ok &= np.asarray(valid, bool)[np.maximum(idx, 0)]
    d = np.where(ok, d2, 0).astype(np.float64)
    if bandwidth is None:
        h = d.sum(1) / np.maximum(ok.sum(1), 1)
    else:
        h = np.broadcast_to(np.asarray(bandwidth, np.float64), (len(d2),))
    arg = np.where(h[:, None] > 0, d / (2.0 * np.where(h > 0, h, 1.0))[:, None], 0.0)
    w = np.where(ok, np.exp(-arg), 0.0)
    s = w.sum(1, keepdims=True)
    return w / np.where(s > 0, s, 1.0)


def diffuse_step(X, idx, w, rate=1.0, fixed=None):
    """One step in float64: (new X, scale of its error bar (1 - rate) * |X| + rate * sum_k |w * x|)."""
    X = np.asarray(X, np.float64)
    keep = ~((np.asarray(idx) >= 0) & (np.asarray(w) != 0)).any(1)
    if fixed is not None:
        keep |= np.asarray(fixed, bool)
    agg, scale = aggregate(X, idx, w)
    new = np.where(keep[:, None], X, (1.0 - rate) * X + rate * agg)
    return new, np.where(keep[:, None], 0.0, (1.0 - rate) * np.abs(X) + rate * scale)


def diffuse(X, idx, w, steps=1, rate=1.0, fixed=None):
    X = np.asarray(X, np.float64)
    for _ in range(steps):
        X, _ = diffuse_step(X, idx, w, rate, fixed)
    return X
