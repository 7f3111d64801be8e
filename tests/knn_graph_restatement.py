"""The kNN graph backwards (include/ogs_knn.h: ogs_knn_transpose, ogs_knn_aggregate_t, ogs_knn_edge_dots,
ogs_knn_smoothness_fwd / _bwd) restated in NumPy.

The reverse lists come from ``np.argsort(kind="stable")`` over the valid slots; everything else is a float64 composition that
also returns the SCALE its error bar is stated in (the sum of the absolute values of the terms) and, where the bar depends on
it, the number of terms.  tests/test_knn_graph_host.py pins this file to per-row Python loops,
tests/test_37c_knn_graph_gpu.py holds the kernels to it."""
import numpy as np

U = 2.0 ** -24                  # unit roundoff of fp32


def valid_slots(idx, R):
    idx = np.asarray(idx, np.int64)
    return (idx >= 0) & (idx < R)


def reverse_lists(idx, R):
    """(begin int32 [R + 1], slots int32 [valid slots]): slots[begin[r]:begin[r + 1]] = the flat slots e with idx.flat[e] == r,
    ascending."""
    flat = np.asarray(idx, np.int64).reshape(-1)
    e = np.nonzero((flat >= 0) & (flat < R))[0]
    slots = e[np.argsort(flat[e], kind="stable")].astype(np.int32)
    counts = np.bincount(flat[e], minlength=R)[:R] if R > 0 else np.zeros(0, np.int64)
    begin = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    return begin, slots


def in_degree(idx, R):
    begin, _ = reverse_lists(idx, R)
    return np.diff(begin.astype(np.int64))


def aggregate_t(G, w, idx, R):
    """(out, scale float64 [R, D], m int64 [R]): out[r] = sum over the valid slots e with idx.flat[e] == r of w.flat[e] * G[e // K],
    scale the same sum of |w * g|, m the number of terms."""
    G = np.asarray(G, np.float64)
    idx = np.asarray(idx, np.int64)
    K = idx.shape[1]
    ok = valid_slots(idx, R).reshape(-1)
    e = np.nonzero(ok)[0]
    tgt = idx.reshape(-1)[e]
    terms = np.asarray(w, np.float64).reshape(-1)[e, None] * G[e // K]
    out = np.zeros((R, G.shape[1]))
    scale = np.zeros_like(out)
    np.add.at(out, tgt, terms)
    np.add.at(scale, tgt, np.abs(terms))
    return out, scale, np.bincount(tgt, minlength=R)[:R] if R > 0 else np.zeros(0, np.int64)


def edge_dots(G, X, idx):
    """(gw, scale float64 [n, K]): gw[i, k] = <G[i], X[idx[i, k]]> on the valid slots and 0 on the others; scale = sum_c |g * x|."""
    G, X = np.asarray(G, np.float64), np.asarray(X, np.float64)
    ok = valid_slots(idx, len(X))
    if len(X) == 0:
        return np.zeros(ok.shape), np.zeros(ok.shape)
    x = X[np.where(ok, np.asarray(idx, np.int64), 0)]                 # [n, K, D]: fine at test sizes
    gw = np.einsum("id,ikd->ik", G, x)
    scale = np.einsum("id,ikd->ik", np.abs(G), np.abs(x))
    return np.where(ok, gw, 0.0), np.where(ok, scale, 0.0)


def smoothness(F, idx, w):
    """Row energies of sum_k w[i, k] * |F[i] - F[idx[i, k]]|^2 over the valid slots (R = n): (e float64 [n], scale = the same sum
    of |w| * d2, d2 float64 [n, K] with 0 on the invalid slots, ok bool [n, K])."""
    F = np.asarray(F, np.float64)
    ok = valid_slots(idx, len(F))
    diff = F[:, None, :] - F[np.where(ok, np.asarray(idx, np.int64), 0)]
    d2 = np.where(ok, (diff * diff).sum(-1), 0.0)
    wz = np.where(ok, np.asarray(w, np.float64), 0.0)
    return (wz * d2).sum(1), (np.abs(wz) * d2).sum(1), d2, ok


def smoothness_grad(F, idx, w, scale=1.0):
    """Gradient of scale * sum(e): (gF, sF float64 [n, D], m int64 [n], gw float64 [n, K]).  gF[i] = 2 * scale * (sum_k w[i, k] *
    (F[i] - F[j]) + sum over the in-edges e of i of w[e] * (F[i] - F[e // K])); sF is the same sum of |2 * scale * w * dF| and m
    its number of terms; gw = scale * d2."""
    F = np.asarray(F, np.float64)
    idx = np.asarray(idx, np.int64)
    n, K = idx.shape
    ok = valid_slots(idx, n)
    j = np.where(ok, idx, 0)
    wz = np.where(ok, np.asarray(w, np.float64), 0.0)
    terms = 2.0 * scale * wz[..., None] * (F[:, None, :] - F[j])      # [n, K, D], 0 on the invalid slots
    gF = terms.sum(1)
    sF = np.abs(terms).sum(1)
    np.add.at(gF, j.reshape(-1), -terms.reshape(n * K, -1))           # the target's side of every edge: w * (F[j] - F[i])
    np.add.at(sF, j.reshape(-1), np.abs(terms).reshape(n * K, -1))
    m = ok.sum(1) + in_degree(idx, n)
    _, _, d2, _ = smoothness(F, idx, w)
    return gF, sF, m, scale * d2
