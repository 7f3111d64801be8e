"""Seeded reference / query sets shared by tests/test_knn_query_host.py (which asserts, on the CPU, the conditions the GPU cases rely
on) and tests/test_37d_knn_query_gpu.py (which runs the kernels on them).  Built on tests/knn_cases.py and
tests/knn_neighbors_cases.py."""
import numpy as np

from tests import knn_cases as kc
from tests import knn_neighbors_cases as nc

KS = nc.KS
MAX_K = nc.MAX_K
TIE_K = nc.TIE_K

# (n_ref, m): both sides of the 64-point box on either set, and past one round of 64 candidate boxes (4097 points = 65 boxes)
SIZE_PAIRS = ((1, 1), (1, 65), (2, 5), (5, 64), (63, 1), (64, 64), (65, 63), (129, 65), (4097, 129), (129, 4097), (4097, 4097))

CLUSTER_CENTRES = np.array([[0.0, 0.0, 0.0], [40.0, -25.0, 10.0]])   # of nc.two_clusters


def size_pair(n, m):
    return kc.cloud(n, 700 + n), kc.cloud(m, 900 + m)


def between():
    """nc.two_clusters() as reference; 200 queries around the midpoint of the two centres, far from both clusters, then the
    outliers' own positions (hits at d2 = 0).  Returns (reference, queries, cluster id per reference row)."""
    ref, lab = nc.two_clusters()
    rng = np.random.default_rng(71)
    mid = CLUSTER_CENTRES.mean(0) + rng.standard_normal((200, 3)) * 0.5
    return ref, np.concatenate([mid.astype(np.float32), ref[lab < 0]]).astype(np.float32), lab


def hard():
    """name -> (reference, queries)"""
    rng = np.random.default_rng(73)
    same = kc.cloud(1000, 8, shift=1000.0)
    unit = kc.cloud(1000, 11)
    outside = (np.array([5.0, -3.0, 2.0]) + rng.random((300, 3)) * 0.1).astype(np.float32)
    straddle = (rng.random((400, 3)) * 3.0 - 1.0).astype(np.float32)
    line = nc.collinear()
    off_line = line[rng.integers(0, len(line), 250)] + (rng.standard_normal((250, 3)) * 0.5).astype(np.float32)
    ref_b, q_b, _ = between()
    return {"same": (same, same), "outside": (unit, outside), "straddle": (unit, straddle), "between": (ref_b, q_b),
            "coincident_ref": (nc.coincident(), kc.cloud(150, 12)),
            "coincident_queries": (unit, np.full((200, 3), 0.4, np.float32)),
            "collinear": (line, off_line.astype(np.float32))}


def tie_sets(K):
    """name -> (reference, queries) with exact ties.  'lattice': the 6 x 6 x 6 integer lattice against its 125 cell centres -- d2
    is exactly 0.75 to the 8 corners of the cell and 2.75 to the 24 lattice points of the next shell (fewer at the boundary).
    'dup': kc.tie_clouds(K)['dup'] against its distinct points -- one of them is present K + 2 times, at d2 = 0."""
    clouds = kc.tie_clouds(K)
    g = np.arange(5, dtype=np.float32) + np.float32(0.5)
    centres = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    return {"lattice": (clouds["lattice"], centres), "dup": (clouds["dup"], np.unique(clouds["dup"], axis=0))}


def short():
    """fewer reference rows than K"""
    return {"three": (kc.cloud(3, 5), kc.cloud(70, 6), 8), "none": (np.zeros((0, 3), np.float32), kc.cloud(70, 6), 8)}


def medium(n=50000, m=20000):
    """a clustered reference (most boxes pruned, a few outliers far away) against uniform queries over the clusters' span"""
    ref, _ = nc.two_clusters(n, seed=47, outliers=40)
    rng = np.random.default_rng(75)
    lo, hi = CLUSTER_CENTRES.min(0) - 5.0, CLUSTER_CENTRES.max(0) + 5.0
    return ref, (lo + rng.random((m, 3)) * (hi - lo)).astype(np.float32)
