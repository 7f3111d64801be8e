"""Case builders of the radius-count and DBSCAN tests (tests/test_knn_radius_host.py asserts what the GPU tests rely on)."""
import numpy as np

from tests import knn_components_cases as cc
from tests import knn_radius_restatement as rr

I32 = np.iinfo(np.int32)
BELOW_ONE = np.nextafter(np.float32(1), np.float32(0))
DBSCAN_SIZES = (63, 64, 65, 127, 129, 4097)            # around one box, around two, and many workgroups
COUNT_M = (1, 63, 64, 65)
COUNT_N = (1, 64, 65, 5000)
KTH = 5                                                 # eps2_of: the median d2 to the KTH nearest row, the row itself counted
MIN_PTS = 5                                             # with eps2_of: about half of the rows are cores
COINCIDENT = 3000
SKLEARN_N, SKLEARN_SEED, SKLEARN_EPS, SKLEARN_MIN_PTS = 2000, 16, 0.03, 8    # the seed: the first whose points pass the margin check
GRAPH_N, GRAPH_SEED, GRAPH_EPS2 = 1000, 5, np.float32(0.0004)      # min_pts = 1 against knn.components on a K = 32 table


def eps2_of(points, kth=KTH):
    """a threshold that leaves cores, borders and noise: the median over the rows of the kth smallest d2 (self included)"""
    d2 = rr.d2_matrix(points, points)
    k = min(kth, len(points)) - 1
    return np.float32(np.median(np.partition(d2, k, axis=1)[:, k]))


def blobs(n):
    return cc.blobs(n, 300 + n)


def queries_inside(m, seed):
    """m points spread over the unit cube and a bit beyond it"""
    return (np.random.default_rng(seed).random((m, 3)) * 1.2 - 0.1).astype(np.float32)


def queries_outside(m, seed):
    """m points wholly outside the bounding box of any set in the unit cube: a small cloud around (3, 3, 3)"""
    return (3.0 + 0.05 * np.random.default_rng(seed).standard_normal((m, 3))).astype(np.float32)


def two_blocks(with_pair=True):
    """Integer points: 3 x 3 blocks at x in {0, 1, 2} (rows 0..8) and x in {4, 5, 6} (rows 9..17), y in {0, 1, 2}; row 18 = (3, 1)
    between them; rows 19, 20 = (10, 10), (10, 11), a pair away from everything.  With eps2 = 1 and min_pts = 4 the edge midpoints
    and the centres are cores, the corners borders, (3, 1) a border at d2 = 1 from the cores (2, 1) = row 7 and (4, 1) = row 10, and
    the pair is noise (each has only the other, a non-core, in reach)."""
    x, y = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    a = np.stack((x.reshape(-1), y.reshape(-1)), 1)
    pts = [a, a + np.array([4, 0]), np.array([[3, 1]])]
    if with_pair:
        pts.append(np.array([[10, 10], [10, 11]]))
    xy = np.concatenate(pts)
    return np.concatenate((xy, np.zeros((len(xy), 1), np.int64)), 1).astype(np.float32)


def path_points(cuts=()):
    """The chain of cc.path_graph as points on a line: row p[t] sits at x = t, plus one more unit for every cut at or before t --
    neighbours in the chain are at d2 = 1, across a cut at d2 = 4.  Returns (points, p)."""
    _, p = cc.path_graph(cuts=cuts)
    t = np.arange(cc.PATH_N)
    x = t + (np.asarray(cuts, np.int64)[None, :] <= t[:, None]).sum(1) if len(cuts) else t
    pts = np.zeros((cc.PATH_N, 3), np.float32)
    pts[p, 0] = x
    return pts, p


def coincident():
    """COINCIDENT copies of one point and one more row, last, at d2 = 1 from them"""
    pts = np.full((COINCIDENT + 1, 3), 0.5, np.float32)
    pts[-1, 0] = 1.5
    return pts


def graph_blobs():
    return cc.blobs(GRAPH_N, GRAPH_SEED)


def sklearn_points():
    return cc.blobs(SKLEARN_N, SKLEARN_SEED)


def permuted(points, labels, seed):
    """The same set with its rows renumbered: new row pos[i] is old row i.  Returns (points', labels', pos)."""
    n = len(points)
    perm = np.random.default_rng(seed).permutation(n)                      # new row r is old row perm[r]
    pos = np.empty(n, np.int64)
    pos[perm] = np.arange(n)
    return points[perm], None if labels is None else labels[perm], pos


def ambiguous_borders(points, eps2, min_pts, labels=None):
    """bool [n]: the border rows that have cores of two different clusters at their smallest d2 -- the only rows whose cluster
    may change when the rows are renumbered"""
    cluster, core, _, _, _, _ = rr.dbscan(points, eps2, min_pts, labels)
    lab = np.zeros(len(points), np.int64) if labels is None else np.asarray(labels, np.int64)
    near = rr.within(points, points, eps2, lab, lab) & (core != 0)[None, :]
    d2 = np.where(near, rr.d2_matrix(points, points), np.inf)
    out = np.zeros(len(points), bool)
    for i in np.nonzero((core == 0) & near.any(1))[0]:
        js = np.nonzero(d2[i] == d2[i].min())[0]
        out[i] = len(set(cluster[js].tolist())) > 1
    return out


# ---- scenes of tests/test_38c_dbscan_instances_gpu.py ------------------------------------------------------------------------------
INSTANCE_EPS = 0.08
INSTANCE_MIN_PTS = 6
BRIDGE_EPS = 0.25
BRIDGE_MIN_PTS = 8
BRIDGE_K = 16
FILTER_EPS = 0.3
FILTER_MIN_PTS = 8


def bridge_scene(seed=31):
    """Two blobs of class 0 (150 points each, sigma 0.08) centred at x = 0 and x = 2, and between them a thin bridge of the same
    class: one point every 0.2 from x = 0.3 to x = 1.7.  Every link of the chain is shorter than BRIDGE_EPS, so the kNN graph under
    that max_dist joins everything; a bridge point in the middle has itself and its two neighbours within BRIDGE_EPS, far below
    BRIDGE_MIN_PTS, so it is no core and DBSCAN keeps the blobs apart (the ends of the bridge may become borders, or cores, of the
    blob they touch).  Returns (points, labels, part: 0 / 1 for the blobs, -1 for the bridge)."""
    rng = np.random.default_rng(seed)
    a = 0.08 * rng.standard_normal((150, 3))
    b = np.array([2.0, 0, 0]) + 0.08 * rng.standard_normal((150, 3))
    xs = np.arange(0.3, 1.71, 0.2)
    bridge = np.stack((xs, np.zeros_like(xs), np.zeros_like(xs)), 1)
    pts = np.concatenate((a, b, bridge)).astype(np.float32)
    part = np.array([0] * 150 + [1] * 150 + [-1] * len(xs), np.int64)
    order = rng.permutation(len(pts))
    return pts[order], np.zeros(len(pts), np.int64), part[order]
