"""CPU: the k-means oracle is PINNED against vectors produced by running the reference's own
Quantize_kMeans (tests/golden/make_kmeans_golden.py).  Tolerances: centres 1e-4;
ids exact except rows whose two best distances tie within rounding of the reference's matmul-based cdist."""
import os

import numpy as np
import pytest
import torch

from oracle import kmeans_oracle as ko
from tests.golden.make_kmeans_golden import NUM_ITERS, POS_WEIGHT, case_inputs

GOLD = os.path.join(os.path.dirname(__file__), "golden", "kmeans_golden.npz")
ID_MISMATCH_FRAC = 1e-3
CENTER_TOL = 1e-4


def assert_centers_close(got, want, k_note=""):
    """Centres within 1e-4 -- except that ONE point changing cluster on a near-tie (the reference's cdist goes
    through a matmul, ours is a direct sum of squares) moves two centres by ~|x|/n.  Allow at most
    max(2, 5%) such rows, each bounded by 0.05."""
    diff = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max(axis=1)
    bad = int((diff > CENTER_TOL).sum())
    assert bad <= max(2, int(0.05 * len(diff))), f"{bad} centre rows differ by > {CENTER_TOL} {k_note}: {diff.max()}"
    assert diff.max() < 0.05, f"centre row off by {diff.max()} {k_note}"


def _cases():
    g = np.load(GOLD)
    return [tuple(int(v) for v in row) for row in g["cases"]]


def run_oracle_case(seed, N, k1, k2):
    ins_feat, xyz, init_root, init_leaf, sub = case_inputs(seed, N, k1, k2)
    feat9 = torch.cat((ins_feat, xyz * POS_WEIGHT), dim=1).numpy()
    o = ko.KMeansOracle(k1, k2, NUM_ITERS)
    o.centers = feat9[init_root.numpy()].copy()
    o.assign_root(feat9)
    return o, ins_feat, init_leaf, sub


@pytest.mark.parametrize("seed,N,k1,k2", _cases())
def test_oracle_matches_reference_golden(seed, N, k1, k2):
    g = np.load(GOLD)
    key = lambda name: g[f"s{seed}_n{N}_{name}"]
    ins_feat, xyz, *_ = case_inputs(seed, N, k1, k2)
    np.testing.assert_allclose(key("input_checksum"), [float(ins_feat.double().sum()), float(xyz.double().sum())],
                               rtol=0, atol=1e-9, err_msg="seeded inputs drifted: regenerate the goldens")
    o, ins_feat, init_leaf, sub = run_oracle_case(seed, N, k1, k2)
    ids_ref = key("root_ids").astype(np.int64)
    assert (o.nn_index != ids_ref).mean() <= ID_MISMATCH_FRAC
    assert_centers_close(o.centers, key("root_centers"), "root")
    row_ok = np.abs(o.centers - key("root_centers")).max(axis=1) <= CENTER_TOL
    same = (o.nn_index == ids_ref) & row_ok[o.nn_index]
    np.testing.assert_allclose(o.quantized("root")[same], key("root_q")[same], atol=CENTER_TOL, rtol=0)
    # leaf level, continuing from the REFERENCE's coarse ids so both sides see the same subsets
    o.cls_ids = ids_ref
    o.iLeafSubNum = sub.numpy()
    o.leaf_centers = ins_feat.numpy()[init_leaf.numpy()].copy()
    for c in key("leaf_sel"):
        o.assign_leaf(ins_feat.numpy(), int(c))
    leaf_ref = key("leaf_ids").astype(np.int64)
    assert (o.leaf_cls_ids != leaf_ref).mean() <= ID_MISMATCH_FRAC
    assert_centers_close(o.leaf_centers, key("leaf_centers"), "leaf")
    # never-visited coarse clusters keep the dummy id k1*k2 (kmeans_quantize.py:160)
    untouched = ~np.isin(ids_ref, key("leaf_sel"))
    assert (o.leaf_cls_ids[untouched] == k1 * k2).all()
    # cluster_len bookkeeping of equalize_cluster_size (:130,138)
    np.testing.assert_array_equal(np.bincount(leaf_ref, minlength=k1 * k2 + 1), key("cluster_len_leaf"))


@pytest.mark.parametrize("seed,N,k1,k2", _cases())
def test_oracle_follows_reference_trajectory_step_by_step(seed, N, k1, k2):
    """Every Lloyd iteration of the reference's own trajectory (root_centers_iter / root_ids_iter, produced by
    running the reference with num_iters = 1..5) re-done by the oracle FROM THE REFERENCE'S centres: each id and
    centre difference is attributed to a near-tie row (tests/helpers.py::kmeans_step_attribution)."""
    from tests import helpers
    g = np.load(GOLD)
    key = lambda name: g[f"s{seed}_n{N}_{name}"]
    ins_feat, xyz, init_root, _, _ = case_inputs(seed, N, k1, k2)
    feat9 = torch.cat((ins_feat, xyz * POS_WEIGHT), dim=1).numpy()
    traj_c, traj_i = key("root_centers_iter"), key("root_ids_iter").astype(np.int64)
    c_prev = feat9[init_root.numpy()].copy()
    for t in range(NUM_ITERS):
        ids_pre = ko._argmin_sqdist(feat9, c_prev)
        c_next, _ = ko.lloyd(feat9, c_prev, iters=1)
        helpers.kmeans_step_attribution(feat9, c_prev, traj_c[t], traj_i[t - 1] if t > 0 else None, ids_pre, c_next,
                                        what=f"iteration {t + 1}")
        c_prev = traj_c[t]
    assert np.array_equal(traj_c[-1], key("root_centers"))


def test_empty_cluster_collapses_to_zero():
    """kmeans_quantize.py:209,213-214: an empty cluster's centre becomes ~0 and is never re-seeded."""
    feat = np.random.default_rng(0).random((500, 6)).astype(np.float32)
    cent = np.concatenate([feat[:3], np.full((1, 6), 50.0, np.float32)])   # 4th centre far away: stays empty
    c, ids = ko.lloyd(feat, cent, iters=1)
    assert np.abs(c[3]).max() == 0.0          # 0 / (2e-6) == 0: collapsed onto the origin
    assert np.abs(c[:3]).min() > 0.0


def test_chunk_boundary_extra_trip():
    """N % 10000 == 0 makes the reference loop once more over an empty chunk (:193): only counts change."""
    feat = np.random.default_rng(1).random((10000, 6)).astype(np.float32)
    c1, i1 = ko.lloyd(feat, feat[:8], iters=2, nchunks=2)
    c2, i2 = ko.lloyd(feat, feat[:8], iters=2, nchunks=1)
    assert np.array_equal(i1, i2)
    np.testing.assert_allclose(c1, c2, atol=1e-6)


def _step_attribution_one_block(feat, c_prev, c_next_ref, ids_prev_ref, ids_prev_got, c_next_got, what="", c_prev_got=None):
    """helpers.kmeans_step_attribution as it stood before its distances were chunked over rows (one [N, k, d] float64
    block): kept here as the pin of the chunked form."""
    from tests.helpers import KM_CENTER_TOL, KM_TIE
    X = np.asarray(feat, np.float64)
    C = np.asarray(c_prev, np.float64)
    Cg = C if c_prev_got is None else np.asarray(c_prev_got, np.float64)
    delta = float(np.abs(Cg - C).max())
    dist = lambda cc: np.sqrt(((X[:, None, :] - cc[None, :, :]) ** 2).sum(-1))
    d_ref = dist(C)
    d_got = d_ref if c_prev_got is None else dist(Cg)
    rows = np.arange(len(X))
    for ids, d in ((ids_prev_got, d_got), (ids_prev_ref, d_ref)):
        if ids is None:
            continue
        ids = np.asarray(ids, np.int64)
        assert (d[rows, ids] - d.min(1) < KM_TIE).all(), f"{what}: ids are not the f64 nearest centre"
    got = np.asarray(ids_prev_got, np.int64)
    ref = d_ref.argmin(1) if ids_prev_ref is None else np.asarray(ids_prev_ref, np.int64)
    cg, cr = np.asarray(c_next_got, np.float64), np.asarray(c_next_ref, np.float64)
    flipped = np.nonzero(got != ref)[0]
    gap = np.abs(d_ref[flipped, got[flipped]] - d_ref[flipped, ref[flipped]])
    assert (gap < 2 * KM_TIE + 2 * delta).all(), f"{what}: ids differ on rows that are not near ties"
    for j in range(C.shape[0]):
        members = got == j
        n = int(members.sum())
        if n:
            assert np.abs(cg[j] - X[members].mean(0)).max() < 2e-5, f"{what}: centre {j} is not the mean of its members"
        else:
            assert np.abs(cg[j]).max() < 1e-5, f"{what}: empty cluster {j} must collapse to ~0"
        touching = flipped[(got[flipped] == j) | (ref[flipped] == j)]
        allowed = KM_CENTER_TOL + sum(np.abs(X[r] - cr[j]).max() for r in touching) / max(min(n, int((ref == j).sum())), 1)
        assert np.abs(cg[j] - cr[j]).max() <= allowed, f"{what}: centre {j} off"
    return len(flipped), float(np.abs(cg - cr).max())


def _planted_near_tie_case():
    """N = 3000 rows, k = 12 centres, one oracle iteration -- and row 0 moved ONTO the bisector of its two nearest centres
    (then 4e-6 to the far side), so that both forms have a flipped row inside the tie width to attribute."""
    rng = np.random.default_rng(5)
    X = rng.random((3000, 6)).astype(np.float32)
    C = X[rng.permutation(3000)[:12]].copy()
    d = np.sqrt(((X[0].astype(np.float64) - C.astype(np.float64)) ** 2).sum(-1))
    a, b = np.argsort(d)[:2]
    ca, cb = C[a].astype(np.float64), C[b].astype(np.float64)
    u = (cb - ca) / np.linalg.norm(cb - ca)
    x = X[0].astype(np.float64)
    x = x + (np.dot((ca + cb) / 2 - x, u) + 2e-6) * u           # 2e-6 past the bisector: b is nearer by ~4e-6 < KM_TIE
    X[0] = x.astype(np.float32)
    ids = ko._argmin_sqdist(X, C)
    c_next, _ = ko.lloyd(X, C, iters=1)
    return X, C, ids, c_next, int(a), int(b)


def test_chunked_step_attribution_equals_the_one_block_form(monkeypatch):
    """tests/helpers.py::kmeans_step_attribution evaluates its float64 distances in row chunks.  On N = 3000 it returns what
    the one-block form returns -- with several chunks, one chunk, own previous centres and a given reference trajectory --
    and raises on the same planted errors: one row moved across a gap > KM_TIE, one centre off by 1e-3."""
    from tests import helpers
    X, C, ids, c_next, a, b = _planted_near_tie_case()
    flip = ids.copy()
    flip[0] = a if ids[0] == b else b                            # the other side of a < KM_TIE tie: attributed, not an error
    member = lambda idv: np.stack([X[idv == j].astype(np.float64).mean(0) for j in range(len(C))])
    Cg = (C.astype(np.float64) + 1e-6).astype(np.float32)
    ids_g = ko._argmin_sqdist(X, Cg)
    variants = [
        dict(ids_prev_ref=None, ids_prev_got=ids, c_next_got=c_next),
        dict(ids_prev_ref=ids, ids_prev_got=flip, c_next_got=member(flip)),
        dict(ids_prev_ref=flip, ids_prev_got=ids, c_next_got=c_next),
        dict(ids_prev_ref=ids, ids_prev_got=ids_g, c_next_got=member(ids_g), c_prev_got=Cg),
    ]
    for elems in (1 << 22, 500 * C.size, 7 * C.size):            # one chunk, six chunks, 429 chunks
        monkeypatch.setattr(helpers, "KM_CHUNK_ELEMS", elems)
        for kw in variants:
            want = _step_attribution_one_block(X, C, c_next, **kw)
            assert helpers.kmeans_step_attribution(X, C, c_next, **kw) == want
        assert helpers.kmeans_step_attribution(X, C, c_next, **variants[1])[0] == 1        # the planted flip was seen
        # planted error 1: a row given to a centre that is farther than its nearest by more than KM_TIE
        wrong = ids.copy()
        r = 1234
        dr = np.sqrt(((X[r].astype(np.float64) - C.astype(np.float64)) ** 2).sum(-1))
        wrong[r] = int(np.argsort(dr)[1])
        assert np.sort(dr)[1] - np.sort(dr)[0] > helpers.KM_TIE
        # planted error 2: one centre coordinate off by 1e-3
        c_bad = c_next.copy()
        c_bad[5, 2] += np.float32(1e-3)
        for fn in (helpers.kmeans_step_attribution, _step_attribution_one_block):
            with pytest.raises(AssertionError):
                fn(X, C, c_next, None, wrong, member(wrong))
            with pytest.raises(AssertionError):
                fn(X, C, c_next, ids, ids, c_bad)


def test_final_ids_attribution_raises_on_planted_errors():
    """kmeans_final_ids_attribution needs no chunking (it touches the differing rows only); pinned all the same: a flip inside
    the tie width is counted, a row moved across a gap > KM_TIE raises."""
    from tests import helpers
    X, C, ids, _, a, b = _planted_near_tie_case()
    flip = ids.copy()
    flip[0] = a if ids[0] == b else b
    assert helpers.kmeans_final_ids_attribution(X, C, ids, C, ids) == 0
    assert helpers.kmeans_final_ids_attribution(X, C, ids, C, flip) == 1
    wrong = ids.copy()
    dr = np.sqrt(((X[77].astype(np.float64) - C.astype(np.float64)) ** 2).sum(-1))
    wrong[77] = int(np.argsort(dr)[1])
    assert np.sort(dr)[1] - np.sort(dr)[0] > helpers.KM_TIE
    with pytest.raises(AssertionError):
        helpers.kmeans_final_ids_attribution(X, C, ids, C, wrong)
