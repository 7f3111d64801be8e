"""CPU: tests/knn_query_restatement.py against plain per-row Python loops, the conditions the GPU cases of
tests/test_37d_knn_query_gpu.py rely on, asserted from the restatement, and the argument checks of the Python functions that raise
before any GPU call."""
import math

import numpy as np
import pytest
import torch

from tests import knn_cases as kc
from tests import knn_neighbors_restatement as nr
from tests import knn_query_cases as qc
from tests import knn_query_restatement as qr


def loop_query(points, queries, K):
    p, q = np.asarray(points, np.float32).reshape(-1, 3), np.asarray(queries, np.float32)
    idx, d2 = np.full((len(q), K), -1, np.int32), np.full((len(q), K), np.inf, np.float32)
    for i in range(len(q)):
        cand = []
        for j in range(len(p)):
            dx, dy, dz = q[i, 0] - p[j, 0], q[i, 1] - p[j, 1], q[i, 2] - p[j, 2]
            cand.append((np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz), j))
        cand.sort()
        for k, (d, j) in enumerate(cand[:K]):
            idx[i, k], d2[i, k] = j, d
    return idx, d2


def test_query_against_a_loop():
    dup, base = qc.tie_sets(4)["dup"]
    for ref, q, K in ((kc.cloud(70, 3), kc.cloud(50, 4), 5), (dup, base, 4), (kc.cloud(3, 4), kc.cloud(9, 5), 8),
                      (np.zeros((0, 3), np.float32), kc.cloud(4, 5), 3), (kc.cloud(70, 3), kc.cloud(70, 3)[::-1] * 7 - 3, 9)):
        gi, gd = qr.query(ref, q, K, chunk=32)
        wi, wd = loop_query(ref, q, K)
        assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
    rows = np.array([5, 0, 49])
    gi, gd = qr.query(kc.cloud(70, 3), kc.cloud(50, 4), 5, rows=rows)
    wi, wd = loop_query(kc.cloud(70, 3), kc.cloud(50, 4), 5)
    assert np.array_equal(gi, wi[rows]) and np.array_equal(gd, wd[rows])
    # the same set on both sides is the self-inclusive neighbour list
    si, sd = nr.neighbors(kc.cloud(70, 3), 5, exclude_self=False)
    gi, gd = qr.query(kc.cloud(70, 3), kc.cloud(70, 3), 5)
    assert np.array_equal(gi, si) and np.array_equal(gd, sd)


def test_transfers_against_loops():
    rng = np.random.default_rng(1)
    src, dst = kc.cloud(60, 21), kc.cloud(45, 22)
    lab = rng.integers(-1, 6, 60)
    ignore = rng.random(60) < 0.2
    X = rng.standard_normal((60, 3))
    valid = rng.random(60) > 0.3
    k, L, md = 5, 5, 0.25                                             # label 5 lies outside [0, L)
    idx, d2 = loop_query(src, dst, k)
    got, margin = qr.transfer_labels(src, lab, dst, k, L, md, ignore)
    feat = qr.transfer_features(src, X, dst, k, md, valid)
    some_none = False
    for i in range(len(dst)):
        for kind in ("labels", "features"):
            okrow = (lambda j: 0 <= lab[j] < L and not ignore[j]) if kind == "labels" else (lambda j: valid[j])
            slots = [s for s in range(k) if d2[i, s] <= np.float32(md * md) and okrow(idx[i, s])]
            if not slots:
                some_none = True
                if kind == "labels":
                    assert got[i] == -1
                else:
                    assert feat["weight"][i] == 0 and not feat["feat"][i].any()
                continue
            h = np.mean([float(d2[i, s]) for s in slots])
            e = {s: math.exp(-float(d2[i, s]) / (2 * h)) if h > 0 else 1.0 for s in slots}
            tot = sum(e.values())
            if kind == "labels":
                sums = {}
                for s in slots:
                    sums[lab[idx[i, s]]] = sums.get(lab[idx[i, s]], 0.0) + e[s] / tot
                best = max(sums.values())
                if margin[i] > 1e-9:
                    assert got[i] == min(l for l, v in sums.items() if v >= best * (1 - 1e-12))
            else:
                want = sum(e[s] / tot * X[idx[i, s]] for s in slots)
                assert np.allclose(feat["feat"][i], want, rtol=0, atol=1e-13) and abs(feat["weight"][i] - tot) < 1e-13
    assert some_none and (got >= 0).sum() > 10
    one, _ = qr.transfer_labels(src, lab, dst, 1, L)
    near = idx[:, 0]
    assert np.array_equal(one, np.where((lab[near] >= 0) & (lab[near] < L), lab[near], -1))
    # an exact tie goes to the lower label: two sources at the same distance, labels 3 and 1
    tie, m = qr.transfer_labels(np.array([[1, 0, 0], [-1, 0, 0]], np.float32), np.array([3, 1]), np.zeros((1, 3), np.float32), 2, 4)
    assert tie[0] == 1 and m[0] == 0


@pytest.mark.parametrize("K", qc.TIE_K)
def test_tie_sets_tie_at_the_last_slot(K):
    """Rows where slot K - 1 and slot K hold the same distance: only the reference row number decides who is listed."""
    tied = {}
    for name, (ref, q) in qc.tie_sets(K).items():
        idx, d2 = qr.query(ref, q, K + 1)
        tied[name] = int(((d2[:, K - 1] == d2[:, K]) & (idx[:, K] >= 0)).sum())
    assert tied["dup"] >= 1, (K, tied)                                # the point present K + 2 times: K + 2 zeros
    assert tied["lattice"] >= (0 if K == 8 else 27), (K, tied)        # K = 8 is the whole first shell: the cut falls between shells
    ref, q = qc.tie_sets(K)["lattice"]
    _, d2 = qr.query(ref, q, 32)
    inner = np.all((q > 1) & (q < 4), axis=1)                         # cells with a whole second shell around them
    assert inner.sum() == 27 and np.all(d2[:, :8] == 0.75) and np.all(d2[inner, 8:32] == 2.75)


def test_the_hard_sets_are_what_their_names_say():
    h = qc.hard()
    ref, q = h["outside"]
    assert np.any((q.min(0) > ref.max(0)) | (q.max(0) < ref.min(0)))              # separated along an axis: wholly outside
    ref, q = h["straddle"]
    inside = np.all((q >= ref.min(0)) & (q <= ref.max(0)), axis=1)
    assert inside.sum() > 5 and (~inside).sum() > 100
    ref, q, lab = qc.between()
    intra = max(float(np.sqrt(nr.neighbors(ref[lab == c], 1, rows=np.arange(50))[1].max())) for c in (0, 1))
    spread = max(float(np.linalg.norm(ref[lab == c] - qc.CLUSTER_CENTRES[c], axis=1).max()) for c in (0, 1))
    dist = np.stack([np.linalg.norm(q[:200] - qc.CLUSTER_CENTRES[c], axis=1) for c in (0, 1)], 1)
    assert np.all(dist.min(1) - spread > 2 * spread) and spread > intra           # both clusters farther than any intra-cluster distance
    _, d2 = qr.query(ref, q[200:], 1)
    assert len(q) > 200 and not d2.any()                                           # the outliers' own positions: hits at d2 = 0
    ref, q = h["coincident_ref"]
    idx, _ = qr.query(ref, q, 5)
    assert np.ptp(ref, axis=0).max() == 0 and np.array_equal(idx, np.broadcast_to(np.arange(5), (len(q), 5)))
    assert np.ptp(h["coincident_queries"][1], axis=0).max() == 0
    ref, q = h["collinear"]
    assert np.ptp(ref[:, 1]) == 0 and np.ptp(ref[:, 2]) == 0 and np.all(np.abs(q[:, 1:] - ref[0, 1:]).max(1) > 0)
    assert h["same"][0] is h["same"][1]
    for name, (ref, q, K) in qc.short().items():
        idx, d2 = qr.query(ref, q, K)
        assert (idx[:, len(ref):] == -1).all() and np.isinf(d2[:, len(ref):]).all() and (idx[:, :len(ref)] >= 0).all()
    assert {n for n, _ in qc.SIZE_PAIRS} >= {1, 63, 64, 65, 129, 4097} and {m for _, m in qc.SIZE_PAIRS} >= {1, 63, 64, 65, 129, 4097}
    ref, q = qc.medium(2000, 500)
    _, d2 = qr.query(ref, q, 1)
    assert np.median(d2) > 25.0 and np.all(np.ptp(q, axis=0) > 15)                 # most queries lie metres from either 0.05-cluster


def test_argument_checks_that_need_no_gpu():
    from opengaussian_amd import knn, query
    p, q = torch.rand(10, 3), torch.rand(4, 3)
    for call in (lambda: knn.Index(p), lambda: knn.query(p, q, 2)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    lab = torch.zeros(10, dtype=torch.int64)
    feat = torch.rand(10, 5)
    bad = [lambda: query.transfer_labels(p, lab[:9], q), lambda: query.transfer_labels(p, lab, q, ignore=torch.zeros(9, dtype=torch.bool)),
           lambda: query.transfer_labels(p, lab, q, num_labels=0), lambda: query.transfer_labels(p, lab, q, k=0),
           lambda: query.transfer_labels(p, lab, q[:, :2]), lambda: query.transfer_labels(p, lab, q, max_dist=-1.0),
           lambda: query.transfer_features(p, feat[:9], q), lambda: query.transfer_features(p, feat[:, 0], q),
           lambda: query.transfer_features(p, feat, q, valid=torch.ones(9, dtype=torch.bool)),
           lambda: query.transfer_features(p[:, :2], feat, q), lambda: query.transfer_features(p, feat, q, k=0)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError, match="no CPU path"):                         # well-formed CPU input: refused, not computed
        query.transfer_labels(p, lab, q)
