"""CPU: tests/knn_radius_restatement.py pinned to a brute-force flood fill and to scikit-learn's DBSCAN, and the planted
conditions that tests/test_37f_knn_radius_gpu.py and tests/test_38c_dbscan_instances_gpu.py rely on in
tests/knn_radius_cases.py and tests/knn_components_cases.py."""
import numpy as np
import pytest

from tests import knn_components_cases as cc
from tests import knn_components_restatement as cr
from tests import knn_neighbors_restatement as nr
from tests import knn_radius_cases as rc
from tests import knn_radius_restatement as rr

NAMES = ("cluster", "core", "degree", "sizes", "first", "count")


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def test_restatement_is_the_flood_fill_on_random_sets():
    rng = np.random.default_rng(0)
    kinds = set()
    for trial in range(40):
        n = int(rng.integers(1, 60))
        pts = rng.integers(0, 6, (n, 3)).astype(np.float32)                # a small lattice: ties in d2 and coincident rows
        labels = rng.integers(-1, 3, n).astype(np.int32)
        for eps2, min_pts in ((1.0, 1), (1.0, 3), (2.0, 4), (0.0, 2), (np.nan, 1), (np.inf, 5)):
            for lab in (None, labels):
                got, want = rr.dbscan(pts, eps2, min_pts, lab), rr.flood_fill(pts, eps2, min_pts, lab)
                assert _same(got, want), (trial, eps2, min_pts, lab is not None)
                cluster, core, degree, sizes, first, count = got
                C = int(count[0])
                assert sizes[:C].sum() == (cluster >= 0).sum() and not sizes[C:].any() and (first[C:] == -1).all()
                assert (np.diff(first[:C]) > 0).all() and all(cluster[first[c]] == c and core[first[c]] for c in range(C))
                assert (cluster[core != 0] >= 0).all() and ((degree >= min_pts) == (core != 0)).all()
                border = (core == 0) & (cluster >= 0)
                kinds |= {("border", bool(border.any())), ("noise", bool(((cluster < 0) & (degree > 0)).any())), ("C", min(C, 3))}
    assert len(kinds) >= 7                                                  # borders, noise and several cluster counts all occurred


def test_restatement_details():
    pts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [4, 0, 0], [np.nan, 0, 0]], np.float32)
    cluster, core, degree, sizes, first, count = rr.dbscan(pts, 1.0, 2)
    assert degree.tolist() == [2, 3, 2, 1, 0] and core.tolist() == [1, 1, 1, 0, 0]     # equality counts, a NaN row not even itself
    assert cluster.tolist() == [0, 0, 0, -1, -1] and count.tolist() == [1] and sizes.tolist() == [3, 0, 0, 0, 0]
    assert rr.dbscan(pts, rc.BELOW_ONE, 1)[5].tolist() == [4] and rr.dbscan(pts, np.nan, 1)[5].tolist() == [0]
    assert rr.dbscan(pts, -1.0, 1)[2].tolist() == [0] * 5 and rr.dbscan(pts, np.inf, 1)[2].tolist() == [4, 4, 4, 4, 0]
    assert rr.dbscan(np.zeros((0, 3), np.float32), 1.0, 1)[5].tolist() == [0]
    lab = np.array([3, 3, -1, 3, 3], np.int32)
    assert rr.dbscan(pts, 4.0, 1, lab)[0].tolist() == [0, 0, -1, 1, -1]     # the inactive row 2 bridges nothing
    assert rr.radius_count(pts, pts[:2], 1.0).tolist() == [2, 3]
    assert rr.radius_count(pts, pts[:4], 4.0, lab, np.array([3, -1, 3, 2])).tolist() == [2, 0, 3, 0]
    assert rr.radius_count(pts[:0], pts, 1.0).tolist() == [0] * 5


def test_restatement_against_scikit_learn_on_margin_checked_points():
    from sklearn.cluster import DBSCAN
    pts = rc.sklearn_points()
    eps2 = np.float32(rc.SKLEARN_EPS) * np.float32(rc.SKLEARN_EPS)
    d2 = rr.d2_matrix(pts, pts)
    assert not (np.abs(d2 - eps2) < 1e-4 * eps2).any()                      # scikit-learn compares in fp64: no pair near the edge
    cluster, core, degree, sizes, first, count = rr.dbscan(pts, eps2, rc.SKLEARN_MIN_PTS)
    sk = DBSCAN(eps=float(rc.SKLEARN_EPS), min_samples=rc.SKLEARN_MIN_PTS).fit(pts.astype(np.float64))
    sk_core = np.zeros(len(pts), bool)
    sk_core[sk.core_sample_indices_] = True
    assert np.array_equal(sk_core, core != 0) and 100 < sk_core.sum() < len(pts) - 100
    assert np.array_equal(cr.canonical(sk.labels_[sk_core]), cr.canonical(cluster[sk_core])) and count[0] > 1
    assert np.array_equal(sk.labels_ < 0, cluster < 0) and (cluster < 0).sum() > 50
    # borders may differ only where a border has cores of two clusters in reach
    to_sk = {int(cluster[i]): int(sk.labels_[i]) for i in np.nonzero(sk_core)[0]}
    differ = np.array([c >= 0 and to_sk[int(c)] != int(s) for c, s in zip(cluster, sk.labels_)])
    near_core = rr.within(pts, pts, eps2) & sk_core[None, :]
    two = np.array([len(set(cluster[np.nonzero(row)[0]].tolist())) > 1 for row in near_core])
    assert not (differ & ~two).any() and not (differ & sk_core).any()
    print("scikit-learn: cores", int(sk_core.sum()), "clusters", int(count[0]), "noise", int((cluster < 0).sum()), "borders that differ",
          int(differ.sum()), "max degree", int(degree.max()))


def test_two_blocks_are_what_the_border_tests_plant():
    pts = rc.two_blocks()
    cluster, core, degree, sizes, first, count = rr.dbscan(pts, 1.0, 4)
    assert count[0] == 2 and first[:2].tolist() == [1, 10]                  # (0, 1) and (4, 1): the smallest core rows
    corners = [0, 2, 6, 8, 9, 11, 15, 17]
    assert not core[corners].any() and (degree[corners] == 3).all() and cluster[corners].tolist() == [0] * 4 + [1] * 4
    assert core[[1, 3, 4, 5, 7]].all() and core[[10, 12, 13, 14, 16]].all()
    assert degree[18] == 3 and not core[18] and cluster[18] == 0            # (3, 1): d2 = 1 to rows 7 and 10, the smaller row wins
    assert rr.d2_matrix(pts[18:19], pts[[7, 10]]).tolist() == [[1.0, 1.0]]
    assert degree[19:].tolist() == [2, 2] and cluster[19:].tolist() == [-1, -1] and sizes[:2].tolist() == [10, 9]
    back = rr.dbscan(pts[::-1], 1.0, 4)                                     # reversed: (4, 1) now has the smaller row
    assert back[0][::-1][18] == back[0][::-1][10] != back[0][::-1][7] and back[5][0] == 2
    assert rc.ambiguous_borders(pts, 1.0, 4).nonzero()[0].tolist() == [18]
    from sklearn.cluster import DBSCAN
    sk = DBSCAN(eps=1.0, min_samples=4).fit(pts.astype(np.float64))
    assert np.array_equal(cr.canonical(sk.labels_), cr.canonical(cluster))  # scikit-learn gives (3, 1) to the first cluster too


@pytest.mark.parametrize("cuts", [(), cc.PATH_CUTS])
def test_path_points_are_one_chain_per_piece(cuts):
    pts, p = rc.path_points(cuts)
    x = pts[p, 0].astype(np.int64)
    gaps = np.diff(x)
    assert set(gaps.tolist()) <= {1, 2} and (gaps == 2).sum() == len(cuts) and (gaps[[t - 1 for t in cuts]] == 2).all()
    assert x.max() < 1 << 23 and not pts[:, 1:].any()                       # exact in fp32


def test_coincident_and_lattice_cases():
    pts = rc.coincident()
    d2 = rr.d2_matrix(pts[-1:], pts)
    assert (d2[0, :-1] == 1.0).all() and not rr.d2_matrix(pts[:1], pts[:-1]).any()
    full = cc.lattice(gap_after=())
    lab = cc.checkerboard_labels(full)
    assert rr.dbscan(full, 2.0, 1, lab)[5][0] == 2 and rr.dbscan(full, 1.0, 1, lab)[5][0] == len(full)
    wall = cc.wall_labels(full)
    assert rr.dbscan(full, 1.0, 1, wall)[5][0] == 2 and rr.dbscan(full, 1.0, 1)[5][0] == 1


def test_graph_blobs_fit_a_table_of_32():
    pts = rc.graph_blobs()
    degree = rr.radius_count(pts, pts, rc.GRAPH_EPS2)
    assert degree.max() - 1 <= 31 and degree.max() > 8                      # at most 31 OTHERS within eps: a K = 32 table holds them all
    d2 = rr.d2_matrix(pts, pts)
    assert not (d2 == rc.GRAPH_EPS2).any()
    count = rr.dbscan(pts, rc.GRAPH_EPS2, 1)[5][0]
    assert 10 < count < len(pts)
    idx, nd2 = nr.neighbors(pts, 32)
    assert np.array_equal(cr.components(idx, nd2, rc.GRAPH_EPS2)[0], rr.dbscan(pts, rc.GRAPH_EPS2, 1)[0])


@pytest.mark.parametrize("n", rc.DBSCAN_SIZES[:5])
def test_size_cases_have_cores_borders_and_noise(n):
    pts = rc.blobs(n)
    cluster, core, degree, _, _, count = rr.dbscan(pts, rc.eps2_of(pts), rc.MIN_PTS)
    assert core.any() and not core.all() and count[0] >= 1 and (cluster < 0).any() and ((core == 0) & (cluster >= 0)).any()


def test_bridge_scene_geometry():
    pts, lab, part = rc.bridge_scene()
    inst, num, ilab, isize = rr.segment_instances_dbscan(pts, lab, rc.BRIDGE_EPS, rc.BRIDGE_MIN_PTS)
    a, b = np.unique(inst[part == 0]), np.unique(inst[part == 1])
    assert num == 2 and len(a) == 1 and len(b) == 1 and a[0] >= 0 and b[0] >= 0 and a[0] != b[0]      # two instances
    idx, d2 = nr.neighbors(pts, rc.BRIDGE_K)
    merged = cr.segment_instances(idx, d2, lab, rc.BRIDGE_EPS)
    assert merged[1] == 1 and (merged[0] == 0).all()                        # the kNN graph under the same distance: one


def test_instance_and_filter_scenes():
    pts, lab, blob = cc.instance_scene()
    inst, num, ilab, isize = rr.segment_instances_dbscan(pts, lab, rc.INSTANCE_EPS, rc.INSTANCE_MIN_PTS, 1, (7,))
    assert num >= 6 and (inst[lab == 7] == -1).all() and (inst[lab == -1] == -1).all()
    for b in range(blob.max() + 1):
        if lab[blob == b][0] != 7:
            ids = np.unique(inst[(blob == b) & (inst >= 0)])
            assert len(ids) == 1                                            # every blob is one instance (its fringe may be noise)
    pts, grp, main = cc.filter_scene()
    for share in (None, 0.5, 0.2):
        assert np.array_equal(rr.density_filter(pts, grp, cc.FILTER_GROUPS, rc.FILTER_EPS, rc.FILTER_MIN_PTS, share), main), share
    both = rr.density_filter(pts, grp, cc.FILTER_GROUPS, rc.FILTER_EPS, rc.FILTER_MIN_PTS, 0.05)
    assert both.sum() == main.sum() + 40 * cc.FILTER_GROUPS                 # a small share keeps the dense floaters too
