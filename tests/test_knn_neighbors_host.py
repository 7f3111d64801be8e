"""CPU: tests/knn_neighbors_restatement.py against plain per-row Python loops, and the conditions the GPU cases of
tests/test_37b_knn_neighbors_gpu.py rely on, asserted from the restatement."""
import math

import numpy as np
import pytest

from tests import knn_cases as kc
from tests import knn_neighbors_cases as nc
from tests import knn_neighbors_restatement as nr


def loop_neighbors(points, K, exclude_self):
    p = np.asarray(points, np.float32)
    n = len(p)
    idx, d2 = np.full((n, K), -1, np.int32), np.full((n, K), np.inf, np.float32)
    for i in range(n):
        cand = []
        for j in range(n):
            if exclude_self and j == i:
                continue
            dx, dy, dz = p[i, 0] - p[j, 0], p[i, 1] - p[j, 1], p[i, 2] - p[j, 2]
            cand.append((np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz), j))
        cand.sort()
        for k, (d, j) in enumerate(cand[:K]):
            idx[i, k], d2[i, k] = j, d
    return idx, d2


@pytest.mark.parametrize("exclude_self", [False, True])
def test_neighbors_against_a_loop(exclude_self):
    for pts, K in ((kc.cloud(70, 3), 5), (kc.tie_clouds(4)["dup"], 4), (kc.cloud(3, 4), 8), (nc.coincident(20), 3)):
        gi, gd = nr.neighbors(pts, K, exclude_self, chunk=32)
        wi, wd = loop_neighbors(pts, K, exclude_self)
        assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
    rows = np.array([5, 0, 69])
    gi, gd = nr.neighbors(kc.cloud(70, 3), 5, exclude_self, rows=rows)
    wi, wd = loop_neighbors(kc.cloud(70, 3), 5, exclude_self)
    assert np.array_equal(gi, wi[rows]) and np.array_equal(gd, wd[rows])


def test_aggregate_weights_and_diffusion_against_loops():
    rng = np.random.default_rng(0)
    n, K, D, R = 23, 5, 3, 19
    X = rng.standard_normal((R, D))
    idx = rng.integers(-2, R + 2, (n, K))
    w = rng.standard_normal((n, K))
    got, scale = nr.aggregate(X, idx, np.where((idx >= 0) & (idx < R), w, np.nan))          # NaN parked in skipped slots
    for i in range(n):
        want = sum((w[i, k] * X[idx[i, k]] for k in range(K) if 0 <= idx[i, k] < R), np.zeros(D))
        assert np.allclose(got[i], want, rtol=0, atol=1e-14)
    assert np.all(scale >= np.abs(got) - 1e-14)

    pts = kc.cloud(40, 9)
    ni, nd = nr.neighbors(pts, 6)
    ni[3, 4:] = -1
    nd[3, 4:] = np.inf
    valid = rng.random(40) > 0.3
    valid[ni[7]] = False                                              # row 7: no valid neighbour
    W = nr.neighbor_weights(nd, ni, valid)
    for i in range(40):
        slots = [k for k in range(6) if ni[i, k] >= 0 and valid[ni[i, k]]]
        if not slots:
            assert not W[i].any()
            continue
        h = np.mean([float(nd[i, k]) for k in slots])
        e = np.array([math.exp(-float(nd[i, k]) / (2 * h)) if k in slots else 0.0 for k in range(6)])
        assert np.allclose(W[i], e / e.sum(), rtol=1e-14, atol=0)
    assert not W[7].any() and abs(W[0].sum() - 1) < 1e-14
    Wb = nr.neighbor_weights(nd, ni, bandwidth=0.01)
    assert np.allclose(Wb[0], np.exp(-nd[0].astype(np.float64) / 0.02) / np.exp(-nd[0].astype(np.float64) / 0.02).sum())

    F = rng.standard_normal((40, 2))
    fixed = rng.random(40) > 0.5
    one, _ = nr.diffuse_step(F, ni, W, rate=0.5, fixed=fixed)
    assert np.array_equal(one[fixed], F[fixed]) and np.array_equal(one[7], F[7])
    i = int(np.nonzero(~fixed & W.any(1))[0][0])
    assert np.allclose(one[i], 0.5 * F[i] + 0.5 * (W[i][:, None] * F[np.maximum(ni[i], 0)]).sum(0))
    assert np.array_equal(nr.diffuse(F, ni, W, steps=0), F)
    two = nr.diffuse(F, ni, W, steps=2, rate=0.5, fixed=fixed)
    assert np.allclose(two, nr.diffuse_step(one, ni, W, 0.5, fixed)[0])


@pytest.mark.parametrize("K", nc.TIE_K)
def test_tie_clouds_tie_at_the_last_slot(K):
    """Rows where slot K - 1 and slot K hold the same distance and different ids: only the id decides who is listed."""
    for name, pts in kc.tie_clouds(K).items():
        for ex in (False, True):
            idx, d2 = nr.neighbors(pts, K + 1, ex)
            tied = (d2[:, K - 1] == d2[:, K]) & (idx[:, K - 1] != idx[:, K]) & (idx[:, K] >= 0)
            assert tied.sum() >= 3, (name, K, ex)


def test_clustered_cloud_has_far_rows_and_short_clouds_have_empty_slots():
    pts, lab = nc.two_clusters()
    for K in (4, 16):
        _, d2 = nr.neighbors(pts, K)
        far = d2[:, K - 1] > 10 * np.median(d2[:, K - 1])
        assert far.sum() >= 5 and far[lab < 0].sum() >= 5
    assert (lab == 0).sum() > 500 and (lab == 1).sum() > 500
    for n, ex in ((1, True), (1, False), (2, True), (5, False)):
        idx, d2 = nr.neighbors(kc.cloud(n, 2), 8, ex)
        m = n - 1 if ex else n
        assert (idx[:, m:] == -1).all() and np.isinf(d2[:, m:]).all() and (idx[:, :m] >= 0).all()
    p = nc.collinear()
    assert np.ptp(p[:, 1]) == 0 and np.ptp(p[:, 2]) == 0 and len(np.unique(p[:, 0])) < len(p)
    idx, d2 = nr.neighbors(nc.coincident(), 5, False)
    assert np.array_equal(idx, np.broadcast_to(np.arange(5), (300, 5))) and not d2.any()
