"""The lists of ``ogs_knn_query`` (include/ogs_knn.h) and the transfers ``opengaussian_amd.query`` builds on them, restated in NumPy.

``query`` takes fp32 distances in the kernel's operation order -- ``sqdist_cross``, the cross-set sibling of
``knn_restatement.sqdist_rows`` -- and orders every row by the pair (d2, j) with ``np.lexsort``; the transfers are float64 on those
lists.  tests/test_knn_query_host.py pins this file to per-row Python loops, tests/test_37d_knn_query_gpu.py holds the kernels to it."""
import numpy as np


def sqdist_cross(points, queries, rows):
    """fp32 squared distances [len(rows), n] from the given QUERY rows to every reference point, dx = x_q - x_j."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 3)[np.asarray(rows, dtype=np.int64)]
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return d


def query(points, queries, K, rows=None, chunk=64):
    """(idx int32 [len(rows), K], d2 fp32 [len(rows), K]) of the given query rows (default: all): the first K of all reference
    rows j by ascending (d2, j); slots past the end of the list hold -1 and +inf."""
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n, m = len(points), len(queries)
    rows = np.arange(m) if rows is None else np.asarray(rows)
    idx = np.full((len(rows), K), -1, np.int32)
    d2 = np.full((len(rows), K), np.inf, np.float32)
    if n == 0:
        return idx, d2
    j = np.broadcast_to(np.arange(n), (min(chunk, max(len(rows), 1)), n))
    for c0 in range(0, len(rows), chunk):
        r = rows[c0:c0 + chunk]
        d = sqdist_cross(points, queries, r)
        order = np.lexsort((j[:len(r)], d), axis=1)[:, :K]            # last key first: by d2, then by j
        idx[c0:c0 + len(r), :order.shape[1]] = order
        d2[c0:c0 + len(r), :order.shape[1]] = np.take_along_axis(d, order, axis=1)
    return idx, d2


def raw_weights(d2, counts, bandwidth=None):
    """float64 exp(-d2 / (2 h)) on the slots that count (h: their mean d2 per row, or `bandwidth`), 0 elsewhere; NOT normalised."""
    d = np.where(counts, d2, 0).astype(np.float64)
    if bandwidth is None:
        h = d.sum(1) / np.maximum(counts.sum(1), 1)
    else:
        h = np.broadcast_to(np.asarray(bandwidth, np.float64), (len(d2),))
    arg = np.where(h[:, None] > 0, d / (2.0 * np.where(h > 0, h, 1.0))[:, None], 0.0)
    return np.where(counts, np.exp(-arg), 0.0)


def _counting_slots(idx, d2, max_dist, row_ok):
    counts = (idx >= 0) & np.isfinite(d2)
    if max_dist is not None:
        counts &= d2 <= np.float32(float(max_dist) ** 2)
    if row_ok is not None:
        counts &= np.asarray(row_ok, bool)[np.maximum(idx, 0)]
    return counts


def transfer_labels(src_xyz, src_labels, dst_xyz, k=1, num_labels=None, max_dist=None, ignore=None):
    """(labels int64 [m], margin float64 [m]): the label with the largest weight sum (the lowest of equals), -1 without a counting
    neighbour; margin = (largest sum - second largest) / largest, inf where a single label has weight, 0 on an exact tie."""
    lab = np.asarray(src_labels, np.int64)
    L = int(lab.max()) + 1 if num_labels is None else int(num_labels)
    idx, d2 = query(src_xyz, dst_xyz, k)
    ok = (lab >= 0) & (lab < L)
    if ignore is not None:
        ok &= ~np.asarray(ignore, bool)
    counts = _counting_slots(idx, d2, max_dist, ok)
    w = raw_weights(d2, counts)
    w = w / np.where(w.sum(1, keepdims=True) > 0, w.sum(1, keepdims=True), 1.0)
    m = len(idx)
    table = np.zeros((m, L))
    for s in range(idx.shape[1]):
        c = counts[:, s]
        np.add.at(table, (np.nonzero(c)[0], lab[idx[c, s]]), w[c, s])
    out = np.where(counts.any(1), table.argmax(1), -1)                # np.argmax: the first, so the lowest, of equal maxima
    top = np.sort(table, axis=1)[:, ::-1]
    second = top[:, 1] if L > 1 else np.zeros(m)
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.where(second > 0, (top[:, 0] - second) / top[:, 0], np.inf)
    return out.astype(np.int64), margin


def transfer_features(src_xyz, src_feat, dst_xyz, k=8, max_dist=None, valid=None, bandwidth=None):
    """dict(feat float64 [m, D], weight float64 [m], scale float64 [m, D] = sum_k |w x|, idx, w): the float64 weighted mean."""
    X = np.asarray(src_feat, np.float64)
    idx, d2 = query(src_xyz, dst_xyz, k)
    counts = _counting_slots(idx, d2, max_dist, valid)
    raw = raw_weights(d2, counts, bandwidth)
    total = raw.sum(1)
    w = raw / np.where(total > 0, total, 1.0)[:, None]
    g = X[np.maximum(idx, 0)]                                         # [m, k, D]: fine at test sizes
    return dict(feat=(w[..., None] * g).sum(1), weight=total, scale=(np.abs(w)[..., None] * np.abs(g)).sum(1), idx=idx, w=w)
