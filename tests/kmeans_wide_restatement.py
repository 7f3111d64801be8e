"""NumPy float64 restatement of the wide k-means (include/ogs_kmeans.h, the ogs_kmeans_wide_* block): the oracle of
tests/test_22_kmeans_wide_gpu.py.  The reference project has no wide k-means."""
import numpy as np

U = 2.0 ** -24


def _f64(a):
    return np.asarray(a, np.float64)


def cost_matrix(X, C, metric):
    """[N, k] float64: L2 -- squared distances, differences first; cosine -- minus the dot products (the row's norm does not
    change the arg-min)"""
    X, C = _f64(X), _f64(C)
    if metric == "cosine":
        return -(X @ C.T)
    out = np.empty((X.shape[0], C.shape[0]))
    step = max(1, (1 << 22) // max(1, C.size))
    for s in range(0, X.shape[0], step):
        d = X[s:s + step, None, :] - C[None, :, :]
        out[s:s + step] = (d * d).sum(axis=2)
    return out


def dist_of(X, C, ids, metric):
    """[N] float64 distance of every row to the centre `ids` names: L2 squared distance; cosine 1 - x.c / |x|, 1 for a zero row"""
    X, c = _f64(X), _f64(C)[ids]
    if metric == "l2":
        return ((X - c) ** 2).sum(axis=1)
    n = np.linalg.norm(X, axis=1)
    return np.where(n > 0, 1.0 - (X * c).sum(axis=1) / np.where(n > 0, n, 1.0), 1.0)


def assign(X, C, metric):
    """(ids int64 [N], dist float64 [N]): the first minimum wins (the lowest centre index on a tie)"""
    ids = np.argmin(cost_matrix(X, C, metric), axis=1).astype(np.int64) if len(X) else np.zeros(0, np.int64)
    return ids, dist_of(X, C, ids, metric)


def update(X, ids, C_prev, metric, w=None):
    """(centres [k, D], counts [k], scale [k, D], m [k]): the weighted mean of every centre's rows (cosine: normalised); a centre
    whose weights sum to 0 -- or, under cosine, whose mean has zero norm -- keeps its previous value.  scale = sum |w x| / sum w
    (what the rounding bounds are stated in, 0 for a kept centre), m = rows per centre."""
    X, C = _f64(X), _f64(C_prev).copy()
    k = C.shape[0]
    w = np.ones(len(X)) if w is None else _f64(w)
    sums, scale = np.zeros_like(C), np.zeros_like(C)
    np.add.at(sums, ids, w[:, None] * X)
    np.add.at(scale, ids, np.abs(w[:, None] * X))
    counts = np.bincount(ids, weights=w, minlength=k)
    m = np.bincount(ids, minlength=k)
    for c in range(k):
        if counts[c] > 0:
            v = sums[c] / counts[c]
            scale[c] /= counts[c]
            if metric == "cosine":
                n = np.linalg.norm(v)
                if n == 0:
                    scale[c] = 0
                    continue
                v = v / n
            C[c] = v
        else:
            scale[c] = 0
    return C, counts, scale, m


def inertia(dist, w=None):
    return float((_f64(dist) * (1.0 if w is None else _f64(w))).sum())


def lloyd(X, C, iters, metric, w=None):
    """(ids, dist, centres, counts, inertia [iters + 1]): iters x (assign, update), then the final assign; inertia[t] belongs to
    the assignment of iteration t"""
    C = _f64(C).copy()
    counts, total = np.zeros(C.shape[0]), []
    for t in range(iters + 1):
        ids, dist = assign(X, C, metric)
        total.append(inertia(dist, w))
        if t < iters:
            C, counts, _, _ = update(X, ids, C, metric, w)
    return ids, dist, C, counts, np.array(total)


def score_slack(X, C, metric):
    """[N] float64: (8 D + 64) U max_c S(x, c), the any-order rounding bound of one score -- at most six partial products per
    dimension, the dropped products, bias, shift and split roundings.  L2: S = sum_j |x'_j| |c'_j| + |c'|^2 / 2 on operands
    centred on the float64 mean of the centres; cosine: S = sum_j |x_j| |c_j|."""
    X, C = _f64(X), _f64(C)
    D = X.shape[1]
    if metric == "l2":
        mu = C.mean(axis=0)
        X, C = X - mu, C - mu
        S = np.abs(X) @ np.abs(C).T + 0.5 * (C * C).sum(axis=1)[None, :]
    else:
        S = np.abs(X) @ np.abs(C).T
    return (8 * D + 64) * U * S.max(axis=1)
