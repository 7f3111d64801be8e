"""CPU: tests/knn_components_restatement.py pinned to a brute-force flood fill, what tests/test_37e_knn_components_gpu.py and
tests/test_38b_instances_gpu.py rely on in tests/knn_components_cases.py, the size query, the argument checks of the wrappers, and
the post-processing of query.segment_instances / component_filter around a stand-in for knn.components."""
import os

import numpy as np
import pytest
import torch

from tests import knn_components_cases as cc
from tests import knn_components_restatement as cr
from tests import knn_neighbors_restatement as nr
from tests import knn_restatement as kr


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def _random_graph(rng, n, K):
    idx = rng.integers(-2, n + 2, (n, K)).astype(np.int32)
    idx[rng.random((n, K)) < 0.55] = -1                                     # sparse enough to leave several components
    d2 = rng.integers(0, 5, (n, K)).astype(np.float32)
    d2[rng.random((n, K)) < 0.05] = np.nan
    labels = rng.integers(-1, 3, n).astype(np.int32)
    return idx, d2, labels


def test_restatement_is_the_flood_fill_on_random_graphs():
    rng = np.random.default_rng(0)
    counts = set()
    for trial in range(60):
        n, K = int(rng.integers(1, 40)), int(rng.integers(1, 5))
        idx, d2, labels = _random_graph(rng, n, K)
        for kw in (dict(), dict(d2=d2, max_d2=2.0), dict(labels=labels), dict(d2=d2, max_d2=2.0, labels=labels),
                   dict(d2=d2), dict(max_d2=0.0), dict(d2=d2, max_d2=np.nan)):
            got, want = cr.components(idx, **kw), cr.flood_fill(idx, **kw)
            assert _same(got, want), (trial, sorted(kw))
            comp, count, sizes, first = got
            C = int(count[0])
            counts.add(C)
            assert sizes[:C].sum() == (comp >= 0).sum() and not sizes[C:].any() and (first[C:] == -1).all()
            assert (np.diff(first[:C]) > 0).all() and all(comp[first[c]] == c for c in range(C))
    assert len(counts) > 10                                                 # the graphs were not all one piece or all singletons


def test_edge_rule_details():
    idx = np.array([[1], [-1], [2], [0]], np.int32)                         # 0 -> 1, 2 -> 2 (self), 3 -> 0
    d2 = np.array([[1.0], [np.inf], [0.0], [np.nan]], np.float32)
    assert cr.components(idx)[0].tolist() == [0, 0, 1, 0]                   # one-way edges join, a self slot does not
    assert cr.components(idx, d2, 1.0)[0].tolist() == [0, 0, 1, 2]          # equality joins, NaN does not
    assert cr.components(idx, d2, np.nextafter(np.float32(1), np.float32(0)))[0].tolist() == [0, 1, 2, 3]
    assert cr.components(idx, d2, np.nan)[1][0] == 4 and cr.components(idx, d2, None)[1][0] == 2
    lab = np.array([5, 5, 5, -1], np.int32)
    comp, count, sizes, first = cr.components(idx, labels=lab)
    assert comp.tolist() == [0, 0, 1, -1] and count[0] == 2 and sizes.tolist() == [2, 1, 0, 0] and first.tolist() == [0, 2, -1, -1]
    assert cr.components(idx, labels=np.full(4, -1))[1][0] == 0
    assert cr.components(np.zeros((0, 3), np.int32))[1].tolist() == [0]


def test_the_cases_hold_what_the_gpu_tests_rely_on():
    idx, p = cc.path_graph()
    where0 = int(np.nonzero(p == 0)[0][0])
    assert idx.shape == (cc.PATH_N, 1) and cc.PATH_N > 16 * cc.BLOCK_SLOTS
    assert cc.PATH_N // 4 < where0 < 3 * cc.PATH_N // 4                      # the root, row 0, far from either end of the chain
    comp, count, sizes, first = cr.components(idx)
    assert count[0] == 1 and sizes[0] == cc.PATH_N and first[0] == 0
    cut, _ = cc.path_graph(cuts=cc.PATH_CUTS)
    comp, count, sizes, first = cr.components(cut)
    lengths = np.diff((0,) + cc.PATH_CUTS + (cc.PATH_N,))
    assert count[0] == 4 and sorted(sizes[:4].tolist()) == sorted(lengths.tolist())
    for K in (1, 32):
        comp, count, sizes, first = cr.components(cc.star(K=K))
        assert count[0] == 1 and first[0] == 0 and sizes[0] == cc.STAR_N and not comp.any()
    comp, count, _, _ = cr.components(cc.one_way())
    assert count[0] == 2 and comp[8] == comp[3] == 0 and comp[9] == 1 and not (cc.one_way() == 8).any()
    junk = cc.junk_slots()
    assert all((junk == v).any() for v in (-1, 200, 201, -2, cc.I32.min, cc.I32.max)) and 10 < cr.components(junk)[1][0] < 190
    # lattice: exact distances, pieces by threshold
    pts = cc.lattice()
    idx, d2 = nr.neighbors(pts, 8)
    assert set(np.unique(d2).tolist()) <= {1.0, 2.0, 4.0, 5.0, 8.0} and (d2 == 4.0).any()
    assert cr.components(idx, d2, 1.0)[1][0] == 2                           # the two pieces either side of the gap
    assert cr.components(idx, d2, np.nextafter(np.float32(1), np.float32(0)))[1][0] == len(pts)
    assert cr.components(idx, d2, 4.0)[1][0] == 1 and cr.components(idx, d2, np.nan)[1][0] == len(pts)
    # two interleaved classes on one lattice: per-class components, joined through the diagonals only
    full = cc.lattice(gap_after=())
    idx, d2 = nr.neighbors(full, 8)
    lab = cc.checkerboard_labels(full)
    comp, count, _, _ = cr.components(idx, d2, 2.0, lab)
    assert count[0] == 2 and all(len(set(lab[comp == c])) == 1 for c in range(2))
    assert cr.components(idx, d2, 1.0, lab)[1][0] == len(full)              # the d2 = 1 neighbours are of the other class
    holes = cc.checkerboard_labels(full, holes=15)
    comp = cr.components(idx, d2, 2.0, holes)[0]
    assert ((comp == -1) == (holes == -1)).all() and (holes == -1).sum() == 15
    wall = cc.wall_labels(full)
    comp, count, _, _ = cr.components(idx, d2, 2.0, wall)
    assert count[0] == 2 and (comp[full[:, 0] < 3] == 0).all() and (comp[full[:, 0] > 3] == 1).all()
    assert cr.components(idx, d2, 2.0)[1][0] == 1                           # ... which the wall's rows would bridge
    # real tables: the threshold cuts them into many pieces, none gives a few
    for n, K in cc.TABLE_SIZES[:-1]:
        idx, d2 = nr.neighbors(cc.blobs(n, 100 + n + K), K)
        many, few = cr.components(idx, d2, cc.threshold_of(d2))[1][0], cr.components(idx)[1][0]
        assert few < many and few <= n // 2, (n, K, few, many)
    assert {n * K for n, K in cc.TABLE_SIZES} >= {cc.BLOCK_SLOTS - 4, cc.BLOCK_SLOTS, cc.BLOCK_SLOTS + 4, cc.BLOCK_SLOTS - 1,
                                                  cc.BLOCK_SLOTS + 1}


def test_permutations_keep_the_partition():
    idx, d2 = nr.neighbors(cc.blobs(257, 9), 4)
    thr = cc.threshold_of(d2)
    base = cr.components(idx, d2, thr)
    assert _same(base, cr.components(*cc.permute_slots(idx, d2, 3), thr))
    pidx, pd2, pos = cc.permute_rows(idx, d2, 4)
    moved = cr.components(pidx, pd2, thr)
    assert moved[1][0] == base[1][0] and np.array_equal(cr.canonical(moved[0][pos]), cr.canonical(base[0]))
    assert not np.array_equal(moved[0][pos], base[0])                       # the numbering itself did change


def test_size_query_is_monotone_and_non_zero():
    from opengaussian_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    q = _lib.lib().ogs_knn_components_tmp_bytes
    sizes = [q(n) for n in (1, 2, 255, 256, 257, 5000, 1 << 20, 1 << 24, (1 << 31) - 1)]
    assert all(s > 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert q(1 << 20) >= 3 * 4 * (1 << 20)                                  # parent, flag, dense
    assert q(0) == 0 and q(-1) == 0 and q(1 << 31) == 0


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from opengaussian_amd import knn, query
    idx = torch.zeros((4, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn.components(idx)
    with pytest.raises(RuntimeError, match="no CPU path"):
        query.segment_instances(torch.rand(4, 3), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        query.component_filter(torch.rand(4, 3))


@pytest.fixture
def cpu_components(monkeypatch):
    """knn.neighbors and knn.components replaced by the restatements on CPU tensors; records the calls"""
    from opengaussian_amd import knn, query
    calls = {"neighbors": 0, "components": []}
    for mod in (query, knn):
        monkeypatch.setattr(mod, "_need_gpu", lambda t, name: None)

    def neighbors(points, k, exclude_self=True):
        calls["neighbors"] += 1
        idx, d2 = nr.neighbors(points.numpy(), int(k), exclude_self)
        return torch.from_numpy(idx), torch.from_numpy(d2)

    def components(idx, d2=None, max_d2=None, labels=None):
        assert labels is None or labels.dtype is torch.int32
        assert max_d2 is None or (isinstance(max_d2, torch.Tensor) and max_d2.dtype is torch.float32 and max_d2.numel() == 1)
        calls["components"].append(None if max_d2 is None else float(max_d2))
        out = cr.components(idx.numpy(), None if d2 is None else d2.numpy(), None if max_d2 is None else max_d2.numpy()[0],
                            None if labels is None else labels.numpy())
        return tuple(torch.from_numpy(o) for o in out)

    monkeypatch.setattr(knn, "neighbors", neighbors)
    monkeypatch.setattr(knn, "components", components)
    return query, calls


def test_value_errors_of_the_wrappers(cpu_components):
    query, _ = cpu_components
    from opengaussian_amd import knn
    xyz, lab = torch.rand(6, 3), torch.zeros(6, dtype=torch.int64)
    for bad in (lambda: query.segment_instances(torch.rand(6, 2), lab), lambda: query.segment_instances(xyz, lab[:5]),
                lambda: query.segment_instances(xyz, lab, min_size=0), lambda: query.segment_instances(xyz, lab, k=0),
                lambda: query.segment_instances(xyz, lab, max_dist=-1.0),
                lambda: query.segment_instances(xyz, lab, neighbors=(torch.zeros((5, 2), dtype=torch.int32), torch.zeros(5, 2))),
                lambda: query.segment_instances(xyz, lab, ignore=torch.zeros(5, dtype=torch.bool)),
                lambda: query.component_filter(xyz, group=lab[:5]), lambda: query.component_filter(xyz, num_groups=0),
                lambda: query.component_filter(xyz, num_groups=2), lambda: query.component_filter(xyz, min_share=1.5),
                lambda: query.component_filter(torch.rand(6, 4))):
        with pytest.raises(ValueError):
            bad()


def test_components_wrapper_checks_its_arguments(monkeypatch):
    from opengaussian_amd import knn
    monkeypatch.setattr(knn, "_need_gpu", lambda t, name: None)
    idx = torch.zeros((4, 2), dtype=torch.int32)
    for bad in (lambda: knn.components(torch.zeros(4, dtype=torch.int32)), lambda: knn.components(torch.zeros((4, 0), dtype=torch.int32)),
                lambda: knn.components(idx, d2=torch.zeros(4, 3)), lambda: knn.components(idx, labels=torch.zeros(5)),
                lambda: knn.components(idx, max_d2=torch.zeros(2))):
        with pytest.raises(ValueError):
            bad()


def test_segment_instances_post_processing(cpu_components):
    query, calls = cpu_components
    pts, lab, blob = cc.instance_scene()
    idx, d2 = nr.neighbors(pts, cc.INSTANCE_K)
    T = torch.from_numpy
    # the planted geometry: with the floaters dropped, the instances ARE the blobs of the classes that count
    for min_size, ignore in ((1, ()), (cc.FLOATER + 1, ()), (cc.FLOATER + 1, (7,)), (1, (7, 0))):
        want = cr.segment_instances(idx, d2, lab, cc.INSTANCE_MAX_DIST, min_size, ignore)
        before = calls["neighbors"]
        got = query.segment_instances(T(pts), T(lab), k=cc.INSTANCE_K, max_dist=cc.INSTANCE_MAX_DIST, min_size=min_size,
                                      ignore=list(ignore) or None)
        assert calls["neighbors"] == before + 1
        assert calls["components"][-1] == float(np.float32(cc.INSTANCE_MAX_DIST) * np.float32(cc.INSTANCE_MAX_DIST))
        assert isinstance(got[1], int) and got[1] == want[1]
        assert got[0].dtype is torch.int32 and got[3].dtype is torch.int32 and got[2].dtype is torch.int64
        for g, w in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])):
            assert np.array_equal(g.numpy(), w), (min_size, ignore)
    inst, num, ilab, isize = cr.segment_instances(idx, d2, lab, cc.INSTANCE_MAX_DIST, cc.FLOATER + 1, (7,))
    blobs_that_count = [b for b in range(blob.max() + 1) if lab[blob == b][0] != 7]
    assert num == len(blobs_that_count) == 7
    for b in blobs_that_count:
        ids = np.unique(inst[blob == b])
        assert len(ids) == 1 and ids[0] >= 0 and isize[ids[0]] == (blob == b).sum() and ilab[ids[0]] == lab[blob == b][0]
    floaters = (blob == -1) & (lab >= 0)
    assert floaters.sum() == 2 * cc.FLOATER and (inst[floaters] == -1).all() and (inst[lab == -1] == -1).all() and (inst[lab == 7] == -1).all()
    with_floaters = cr.segment_instances(idx, d2, lab, cc.INSTANCE_MAX_DIST, 1, (7,))
    assert with_floaters[1] == num + 2 and (with_floaters[0][floaters] >= 0).all()
    assert sorted(with_floaters[3].tolist())[:2] == [cc.FLOATER, cc.FLOATER]
    # a table handed in is used as it is; a bool ignore marks rows; no max_dist hands none on
    before = calls["neighbors"]
    rows = T(lab == 7)
    got = query.segment_instances(T(pts), T(lab), max_dist=None, min_size=2, ignore=rows, neighbors=(T(idx), T(d2)))
    want = cr.segment_instances(idx, d2, lab, None, 2, (7,))
    assert calls["neighbors"] == before and calls["components"][-1] is None
    assert got[1] == want[1] and np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[3].numpy(), want[3])
    none = query.segment_instances(T(pts), torch.full((len(pts),), -1, dtype=torch.int64), neighbors=(T(idx), T(d2)))
    assert none[1] == 0 and (none[0] == -1).all() and none[2].numel() == 0 and none[3].numel() == 0


def test_component_filter_post_processing(cpu_components):
    query, calls = cpu_components
    pts, grp, main = cc.filter_scene()
    idx, d2 = nr.neighbors(pts, cc.FILTER_K)
    T = torch.from_numpy
    G = cc.FILTER_GROUPS
    # the planted geometry: the largest component of every group is its main blob, and the mean-distance filter keeps the floater
    want = cr.component_filter(idx, d2, grp, G)
    assert np.array_equal(want, main)
    floater = ~main & (grp >= 0) & (grp < G)
    assert kr.outlier_mask(pts, grp, G)[floater].all() and floater.sum() == 40 * G
    before = calls["neighbors"]
    got = query.component_filter(T(pts), T(grp), G, k=cc.FILTER_K)
    assert calls["neighbors"] == before + 1 and len(calls["components"]) == 1          # all groups: one call each
    assert got.dtype is torch.bool and np.array_equal(got.numpy(), want)
    for share in (0.0, 0.05, 40 / 340, 0.5, 1.0):
        want = cr.component_filter(idx, d2, grp, G, None, share)
        got = query.component_filter(T(pts), T(grp), G, k=cc.FILTER_K, min_share=share)
        assert np.array_equal(got.numpy(), want), share
    assert cr.component_filter(idx, d2, grp, G, None, 0.05)[floater].all()          # a share the floater meets ...
    assert not cr.component_filter(idx, d2, grp, G, None, 0.5)[floater].any()       # ... and one it does not
    assert not cr.component_filter(idx, d2, grp, G, None, 1.0).any()
    # with a threshold, and one group of all rows
    for md in (0.05, 0.3):
        want = cr.component_filter(idx, d2, grp, G, md)
        assert np.array_equal(query.component_filter(T(pts), T(grp), G, k=cc.FILTER_K, max_dist=md).numpy(), want), md
    want = cr.component_filter(idx, d2, None, 1)
    assert np.array_equal(query.component_filter(T(pts), k=cc.FILTER_K).numpy(), want) and 0 < want.sum() < len(pts)
    # equal sizes: the component whose smallest row comes first
    tie = np.array([[0, 0, 0], [9, 0, 0], [0.1, 0, 0], [9.1, 0, 0]], np.float32)
    assert query.component_filter(T(tie), k=1).tolist() == [True, False, True, False]
    assert query.component_filter(T(tie[[1, 0, 3, 2]]), k=1).tolist() == [True, False, True, False]
    assert query.component_filter(torch.zeros((0, 3)), k=4).shape == (0,)
