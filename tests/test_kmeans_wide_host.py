"""CPU: tests/kmeans_wide_restatement.py on planted data, what tests/test_22_kmeans_wide_gpu.py relies on in
tests/kmeans_wide_cases.py, the wide k-means symbols of the built library, and the argument checks of the Python wrappers
(they come before anything touches the GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import kmeans_wide_cases as wc
from tests import kmeans_wide_restatement as wr

NEW_SYMBOLS = ["ogs_kmeans_wide_row_tile", "ogs_kmeans_wide_centre_tile", "ogs_kmeans_wide_dim_step", "ogs_kmeans_wide_stage",
               "ogs_kmeans_wide_max_dim", "ogs_kmeans_wide_max_k", "ogs_kmeans_wide_tmp_bytes", "ogs_kmeans_wide_assign",
               "ogs_kmeans_wide_update", "ogs_kmeans_wide_inertia", "ogs_kmeans_wide_lloyd"]


@pytest.fixture(scope="module")
def lib():
    from opengaussian_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("metric", wc.METRICS)
def test_restatement_recovers_planted_partitions(metric):
    for N, D, k in [(63, 17, 5), (300, 33, 17), (200, 1, 4)]:
        if metric == "cosine" and D == 1:
            continue                                             # two directions only
        X, C, labels = wc.planted(N, D, k, metric)
        ids, dist = wr.assign(X, C, metric)
        assert np.array_equal(ids, labels), (N, D, k)
        assert dist.max() < (1e-4 if metric == "l2" else 1e-5)
        # Lloyd from one row of every cluster lands on the planted partition
        first = np.array([int(np.flatnonzero(labels == c)[0]) for c in range(k)])
        init = wc.unit(X[first]) if metric == "cosine" else X[first]
        ids2, _, C2, counts, total = wr.lloyd(X, init, 3, metric)
        assert np.array_equal(ids2, labels) and np.array_equal(counts, np.bincount(labels, minlength=k))
        assert np.abs(C2 - C).max() < 1e-2


@pytest.mark.parametrize("metric", wc.METRICS)
def test_restatement_lloyd_inertia_never_increases(metric):
    name = "uniform/17" if metric == "l2" else "normal/64"
    X, C, _ = wc.random_case(name)
    if metric == "cosine":
        X = wc.unit(X)              # 1 - cos falls monotonically for unit rows (the mean weighs a row by its norm, 1 - cos does not)
    w = wc.weights(len(X), 1)
    for weights in (None, w):
        total = wr.lloyd(X, C[:20], 6, metric, weights)[4]
        assert (np.diff(total) <= 1e-12 * total[0]).all() and total[-1] < total[0]


def test_restatement_ties_empty_centres_and_zero_rows():
    X = np.array([[1.0, 0.0], [0.0, 2.0], [0.0, 0.0]], np.float32)
    C = np.array([[0.0, 1.0], [1.0, 0.0], [1.0, 0.0], [5.0, 5.0]], np.float32)
    ids, dist = wr.assign(X, C, "l2")
    assert list(ids) == [1, 0, 0] and np.allclose(dist, [0, 1, 1])            # the duplicate 2 never wins; (0, 0) ties 0 / 1 -> 0
    ids, dist = wr.assign(X, wc.unit(C), "cosine")
    assert list(ids) == [1, 0, 0] and np.allclose(dist, [0, 0, 1])            # the zero row: id 0, dist 1
    newC, counts, scale, m = wr.update(X, ids, C, "l2", np.array([1.0, 3.0, 0.0]))
    assert np.array_equal(newC[2:], C[2:].astype(np.float64)) and list(counts) == [3, 1, 0, 0] and list(m) == [2, 1, 0, 0]
    assert np.allclose(newC[0], [0, 2]) and np.allclose(newC[1], [1, 0]) and (scale[2:] == 0).all()


def test_the_cases_hold_what_the_gpu_tests_rely_on():
    for case in wc.RANDOM_CASES:
        X, C, metric = wc.random_case(case[0])
        assert X.shape == (case[1], case[2]) and C.shape == (case[3], case[2]) and X.dtype == C.dtype == np.float32
        if metric == "cosine":
            assert np.abs(np.linalg.norm(C.astype(np.float64), axis=1) - 1).max() < 2 * wr.U
    X, C, _ = wc.random_case("uniform+100")
    assert X.min() > 99 and np.ptp(X) < 2                                       # off the origin: spread << distance from it
    # the bar of the near-minimiser test is exercised: some rows have a runner-up inside it, and it is far below what a single
    # bf16 product loses (2^-8 per factor) at the narrow widths
    inside = {}
    for case in wc.RANDOM_CASES:
        X, C, metric = wc.random_case(case[0])
        cost = np.sort(wr.cost_matrix(X, C, metric), axis=1)
        tau = (4 if metric == "l2" else 2) * wr.score_slack(X, C, metric)
        inside[case[0]] = float((cost[:, 1] - cost[:, 0] <= tau).mean())
    assert max(inside.values()) > 0 and max(inside.values()) <= 0.05, inside
    for D in (17, 33):
        assert 4 * (8 * D + 64) * wr.U < 2.0 ** -8 / 16          # tau against the 2^-8 a single bf16 factor loses of the same sum
    shapes = wc.PLANTED_SHAPES
    assert {n for n, _, _ in shapes} >= {wc.ROW_TILE - 1, wc.ROW_TILE + 1}
    assert {k for _, _, k in shapes} >= {wc.CENTRE_TILE - 1, wc.CENTRE_TILE + 1, 2 * wc.CENTRE_TILE + 1, wc.STAGE + 1}
    assert {d for _, d, _ in shapes} >= {wc.DIM_STEP - 1, wc.DIM_STEP + 1, wc.MAX_DIM, *wc.LDS_DIMS, *(d + 1 for d in wc.LDS_DIMS)}
    X, dirs, labels, init = wc.codebook_scene()
    assert X.shape == (2000, 64) and len(np.unique(labels)) == 8 and len(set(np.bincount(labels))) > 1
    assert np.array_equal(wr.assign(init, dirs, "cosine")[0], np.arange(8))


def test_new_symbols_are_bound_and_exported(lib):
    from opengaussian_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(raw, name), name


def test_sizes_are_the_ones_the_cases_bracket(lib):
    assert int(lib.ogs_kmeans_wide_row_tile()) == wc.ROW_TILE
    assert int(lib.ogs_kmeans_wide_centre_tile()) == wc.CENTRE_TILE
    assert int(lib.ogs_kmeans_wide_dim_step()) == wc.DIM_STEP
    assert int(lib.ogs_kmeans_wide_stage()) == wc.STAGE
    assert int(lib.ogs_kmeans_wide_max_dim()) == wc.MAX_DIM and int(lib.ogs_kmeans_wide_max_k()) == wc.MAX_K
    assert lib.ogs_kmeans_wide_tmp_bytes(1000, 512, 320) >= 320 * 512 * (4 + 6)          # sums and packed planes
    assert lib.ogs_kmeans_wide_tmp_bytes(0, 1, 1) > 0
    for bad in ((10, 0, 4), (10, wc.MAX_DIM + 1, 4), (10, 8, 0), (10, 8, wc.MAX_K + 1), (-1, 8, 4), (1 << 31, 8, 4)):
        assert lib.ogs_kmeans_wide_tmp_bytes(*bad) == 0, bad
    # no [N, k] buffer: the scratch of 100 000 x 64 rows against 1024 centres is far below N k floats
    assert lib.ogs_kmeans_wide_tmp_bytes(100_000, 64, 1024) < 100_000 * 1024 * 4 // 8


def test_wrappers_refuse_bad_arguments_before_the_gpu(lib):
    from opengaussian_amd import kmeans, query
    f = torch.zeros(10, 8)
    c = torch.zeros(4, 8)
    ids = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(ValueError, match="D="):
        kmeans.wide_assign(torch.zeros(3, wc.MAX_DIM + 1), torch.zeros(2, wc.MAX_DIM + 1))
    with pytest.raises(ValueError, match="k="):
        kmeans.wide_assign(f, torch.zeros(wc.MAX_K + 1, 8))
    with pytest.raises(ValueError, match="feat is 8 wide"):
        kmeans.wide_assign(f, torch.zeros(4, 9))
    with pytest.raises(ValueError, match="feat is 8 wide"):
        kmeans.wide_lloyd(f, torch.zeros(4, 7), 2)
    for call in (lambda: kmeans.wide_assign(f, c, "manhattan"), lambda: kmeans.wide_update(f, ids, c, "dot"),
                 lambda: kmeans.wide_lloyd(f, c, 2, "L2"), lambda: query.build_codebook(f, 4, metric="euclid")):
        with pytest.raises(ValueError, match="metric"):
            call()
    for call in (lambda: kmeans.wide_update(f, ids, c, "l2", torch.ones(9)), lambda: kmeans.wide_lloyd(f, c, 2, "l2", torch.ones(10, 1)),
                 lambda: query.build_codebook(f, 4, weights=torch.ones(11))):
        with pytest.raises(ValueError, match="weights"):
            call()
    with pytest.raises(ValueError, match="ids"):
        kmeans.wide_update(f, ids[:9], c)
    with pytest.raises(ValueError, match="init"):
        query.build_codebook(f, 4, init=torch.zeros(4, 7))
    with pytest.raises(ValueError, match="D="):
        query.build_codebook(torch.ones(20, 8), wc.MAX_K + 1, init=torch.zeros(wc.MAX_K + 1, 8))
    # init=None needs k valid rows: weight > 0 and not all zero
    feats = torch.ones(10, 8)
    feats[:4] = 0
    with pytest.raises(ValueError, match="valid rows"):
        query.build_codebook(feats, 7)
    w = torch.ones(10)
    w[4:8] = 0
    with pytest.raises(ValueError, match="valid rows"):
        query.build_codebook(feats, 3, weights=w)
    # valid arguments on CPU tensors get as far as the device check: no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        kmeans.wide_assign(f, c)
    with pytest.raises(RuntimeError, match="GPU"):
        query.build_codebook(feats, 2, weights=w)
