"""Seeded clouds shared by tests/test_knn_neighbors_host.py (which asserts, on the CPU, the conditions the GPU cases rely on) and
tests/test_37b_knn_neighbors_gpu.py (which runs the kernels on them).  Built on tests/knn_cases.py."""
import numpy as np

from tests import knn_cases as kc

KS = (1, 3, 4, 5, 8, 9, 16, 17, 32)           # both sides of every list size the search is compiled for (4, 8, 16, 32)
MAX_K = 32
TIE_K = (4, 5, 8, 16)


def sizes(box):
    """Row counts around the search box of `box` points, and one past several workgroups of every helper kernel."""
    return (1, 2, 5, box - 1, box, box + 1, 2 * box + 1, 4097)


def coincident(n=300):
    return np.full((n, 3), 0.25, np.float32)


def collinear(n=700, seed=41):
    """All points on a line parallel to x: two axes of zero extent, and duplicates on the line."""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 3), np.float32)
    p[:, 0] = rng.integers(0, n // 2, n).astype(np.float32) * np.float32(0.125)
    p[:, 1], p[:, 2] = np.float32(-3.0), np.float32(7.5)
    return p


def two_clusters(n=1500, seed=43, outliers=12):
    """Two tight clusters far apart plus a few points far from both: the K-th distance of an outlier is orders of magnitude
    above that of a cluster point.  Returns (points, cluster id per row: 0, 1, or -1 for an outlier)."""
    rng = np.random.default_rng(seed)
    half = (n - outliers) // 2
    a = rng.standard_normal((half, 3)) * 0.05
    b = rng.standard_normal((n - outliers - half, 3)) * 0.05 + np.array([40.0, -25.0, 10.0])
    o = rng.random((outliers, 3)) * 400.0 - 200.0
    pts = np.concatenate([a, b, o]).astype(np.float32)
    lab = np.concatenate([np.zeros(len(a), int), np.ones(len(b), int), np.full(outliers, -1)])
    perm = rng.permutation(n)
    return pts[perm], lab[perm]


def clouds(K):
    """name -> points: every cloud of the exactness test at list size K."""
    out = {"offset": kc.cloud(1000, 8, shift=1000.0), "coincident": coincident(), "collinear": collinear(),
           "clusters": two_clusters()[0]}
    for name, p in kc.tie_clouds(K).items():
        out["tie_" + name] = p
    return out
