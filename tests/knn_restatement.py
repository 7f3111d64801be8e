"""The k-nearest-distance sums of include/ogs_knn.h and the reference's outlier rule on top of them, restated in NumPy.

Distances are fp32 in the kernel's operation order, ``(dx*dx + dy*dy) + dz*dz`` (NumPy does not contract); the K smallest are
selected by SORTING (the kernel bisects on bit patterns instead); sums are fp64.  tests/test_knn_host.py pins this file to
goldens made by the reference's own code, tests/test_37_knn_gpu.py holds the kernel to it.
"""
import numpy as np


def k_rule(n, k_scale=1):
    """K of the reference: ``int(n ** 0.5)`` (gaussian_renderer/__init__.py:298), times 2 in scripts/render_by_click.py:177."""
    return int(n ** 0.5) * k_scale


def sqdist_rows(points, rows):
    """fp32 squared distances [len(rows), n] from the given rows to every point, the row itself included."""
    p = np.ascontiguousarray(points, dtype=np.float32)
    q = p[np.asarray(rows)]
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return d


def ksum(points, K, rows=None, chunk=512):
    """(kth fp32, sum1 fp64, sum2 fp64) of the given rows (default: all) inside ONE group; K is clamped to the group size;
    K = 0 gives zeros."""
    n = len(points)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    K = min(max(int(K), 0), n)
    kth, s1, s2 = np.zeros(len(rows), np.float32), np.zeros(len(rows)), np.zeros(len(rows))
    if K == 0:
        return kth, s1, s2
    for c0 in range(0, len(rows), chunk):
        d = np.sort(sqdist_rows(points, rows[c0:c0 + chunk]), axis=1)[:, :K]
        kth[c0:c0 + chunk] = d[:, K - 1]
        d64 = d.astype(np.float64)
        s1[c0:c0 + chunk] = d64.sum(axis=1)
        s2[c0:c0 + chunk] = (d64 * d64).sum(axis=1)
    return kth, s1, s2


def group_ksum(points, group, num_groups, k):
    """Per-row results in the caller's order for integer group ids (rows with an id outside [0, num_groups) get NaN so that a
    test cannot compare them by accident); k: one K or one per group."""
    points, group = np.asarray(points, np.float32), np.asarray(group)
    n = len(points)
    kth, s1, s2 = np.full(n, np.nan, np.float32), np.full(n, np.nan), np.full(n, np.nan)
    for g in range(num_groups):
        rows = np.nonzero(group == g)[0]
        if len(rows):
            kg = k[g] if np.ndim(k) else k
            kth[rows], s1[rows], s2[rows] = ksum(points[rows], kg)
    return kth, s1, s2


def outlier_stats(points, k_scale=1, std_weight=1.0):
    """The reference's rule on one group, in fp64 on the fp32 distances: dict(mask, row_mean, mean, std, limit, margin).
    margin[i] = |row_mean[i] - limit| / |limit|: how far row i is from changing sides (inf where the limit is nan or 0)."""
    n = len(points)
    K = min(k_rule(n, k_scale), n)
    _, s1, s2 = ksum(points, K)
    N = n * K
    row_mean = s1 / K
    mean = s1.sum() / N
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(max((s2.sum() - s1.sum() ** 2 / N), 0.0) / np.float64(N - 1)) if N > 1 else np.float64("nan")
        limit = mean + std_weight * std
        margin = np.where(np.isfinite(limit) & (limit != 0), np.abs(row_mean - limit) / np.abs(limit), np.inf)
        mask = row_mean < limit
    return dict(mask=mask, row_mean=row_mean, mean=mean, std=std, limit=limit, margin=margin, K=K)


def outlier_mask(points, group=None, num_groups=1, k_scale=1, std_weight=1.0):
    points = np.asarray(points, np.float32)
    if group is None:
        return outlier_stats(points, k_scale, std_weight)["mask"]
    group = np.asarray(group)
    keep = np.zeros(len(points), bool)
    for g in range(num_groups):
        rows = np.nonzero(group == g)[0]
        if len(rows):
            keep[rows] = outlier_stats(points[rows], k_scale, std_weight)["mask"]
    return keep


def dist_cuda2(points):
    """simple_knn's distCUDA2: mean squared distance to the 3 nearest other points = the 4 smallest with the self-distance, / 3."""
    _, s1, _ = ksum(points, 4)
    return (s1 / 3.0).astype(np.float32)
