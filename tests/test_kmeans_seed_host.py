"""CPU: the pieces of the wide seeding that need no GPU -- the restatement's draw (tests/kmeans_seed_restatement.py), the quality and
pruning conditions on the restatement alone, the wrappers' argument checks and the scratch-size query."""
import numpy as np
import pytest
import torch

from tests import kmeans_seed_cases as sc
from tests import kmeans_seed_restatement as sr


def test_splitmix64_known_values():
    # the first three outputs of splitmix64 from state 0 (the published test vector of the generator), and one with a carry out
    # of the 64 bits: seed = 2^64 - 1 makes r = 0 start from GAMMA - 1
    assert sr.rand64(0, 0) == 0xE220A8397B1DCDAF
    assert sr.rand64(0, 1) == 0x6E789E6AA1B965F4
    assert sr.rand64(0, 2) == 0x06C45D188009454F
    assert sr.rand64((1 << 64) - 1, 0) == sr.rand64(sr.GAMMA - 1 - sr.GAMMA, 0)
    assert sr.rand64(5, 3) == sr.rand64(5 + sr.GAMMA, 2)


def _brute_pick(q, rnd):
    T = sum(int(v) for v in q)
    if T == 0:
        return None
    t = (rnd * T) >> 64
    run = 0
    for i, v in enumerate(q):
        run += int(v)
        if run > t:
            return i
    raise AssertionError("t < T always")


def test_pick_matches_brute_force():
    rng = np.random.default_rng(3)
    for trial in range(300):
        n = int(rng.integers(1, 40))
        q = rng.integers(0, 1 << 31, size=n)
        q[rng.random(n) < 0.3] = 0
        rnd = sr.rand64(trial, 0)
        got = sr.pick(q, rnd)
        assert got == _brute_pick(q, rnd)
        assert got is None or q[got] > 0
    # the ends of the range of the draw
    q = np.array([0, 5, 0, 7, 0])
    assert sr.pick(q, 0) == 1 and sr.pick(q, (1 << 64) - 1) == 3
    assert sr.pick(np.zeros(4, np.int64), 123) is None


def test_masses_are_below_2_31_and_exact_for_the_maximum():
    w = np.array([0.0, 1e-30, 0.75, 3.0, 4.0, 7.9999995], np.float32)
    E = sr.exponent(w)
    q = sr.masses(w, E)
    assert E == 3 and q.max() < 1 << 31 and q[0] == 0 and q[1] == 0
    assert q[4] == 1 << 30 and q[3] == 3 << 28
    assert sr.exponent(np.zeros(3, np.float32)) == 0


def test_first_pick_frequencies():
    """masses 1 : 2 : 3 : 4 over 20 000 seeds: every count within 4 sigma of n p"""
    w = np.array([1, 2, 3, 4], np.float32)
    n = 20000
    counts = np.bincount([sr.first_pick(w, s) for s in range(n)], minlength=4)
    p = w.astype(np.float64) / w.sum()
    assert (np.abs(counts - n * p) <= 4 * np.sqrt(n * p * (1 - p))).all(), counts


def test_dist_is_one_order_for_every_width():
    """zero padding is exact: a row and the same row padded to another width have the same dist bits"""
    rng = np.random.default_rng(9)
    for D in (1, 3, 63, 65, 255, 257, 700):
        Y = rng.normal(size=(5, D)).astype(np.float32)
        c = rng.normal(size=D).astype(np.float32)
        want = sr.dist(Y, c)
        for Dp in (256, 1024):
            if Dp >= D:
                Yp, cp = np.zeros((5, Dp), np.float32), np.zeros(Dp, np.float32)
                Yp[:, :D], cp[:D] = Y, c
                assert np.array_equal(sr.dist(Yp, cp), want)
        ref = ((Y.astype(np.float64) - c.astype(np.float64)) ** 2).sum(axis=1)
        assert (np.abs(want - ref) <= (D + 4) * sr.U * ref).all()


@pytest.mark.parametrize("D", sc.MIXTURE_DIMS)
def test_quality_on_the_restatement(D):
    """the issue's condition: D^2 seeding hits at least 30 of the 32 planted clusters, random rows at most 12"""
    for seed in sc.MIXTURE_SEEDS:
        X, labels = sc.mixture(D, seed)
        out = sc.mixture_seeded(D, seed)[0]
        assert out.seeded == sc.MIXTURE_K
        hit = sc.clusters_hit(labels, out.rows)
        rand = sc.clusters_hit(labels, sc.randperm_rows(len(X), sc.MIXTURE_K, seed))
        print(f"D={D} seed={seed}: seeded centres hit {hit} clusters, random rows {rand}")
        assert hit >= 30 and rand <= 12, (D, seed, hit, rand)


@pytest.mark.parametrize("D", sc.MIXTURE_DIMS)
def test_pruning_rule_on_the_restatement(D):
    """the rule never skips a row that would have changed, and skips at least half of the (row, round) pairs"""
    for seed in sc.MIXTURE_SEEDS:
        out, skipped, pairs, wrong = sc.mixture_seeded(D, seed)
        print(f"D={D} seed={seed}: {skipped} of {pairs} pairs skipped ({skipped / pairs:.3f})")
        assert wrong == 0 and pairs == 4096 * (sc.MIXTURE_K - 1)
        assert 2 * skipped >= pairs


def test_restatement_runs_out_of_mass():
    X, which = sc.duplicated()
    out = sr.seed(X, 12, seed=1, C_fill=-1.0)
    assert out.seeded == 7 and (out.rows[7:] == -1).all() and (out.C[7:] == -1.0).all()
    assert sorted(which[out.rows[:7]].tolist()) == list(range(7)) and (out.d2 == 0).all()
    none = sr.seed(X, 3, w=np.zeros(len(X), np.float32))
    assert none.seeded == 0 and (none.rows == -1).all()


def test_tmp_bytes():
    from opengaussian_amd import _lib
    lib = _lib.lib()
    assert lib.ogs_kmeans_wide_seed_rows() == sc.SEED_ROWS
    assert lib.ogs_kmeans_wide_max_dim() == sc.MAX_DIM and lib.ogs_kmeans_wide_max_k() == sc.MAX_K
    f = lib.ogs_kmeans_wide_seed_tmp_bytes
    for N, D, k in ((-1, 8, 4), (1 << 31, 8, 4), (10, 0, 4), (10, sc.MAX_DIM + 1, 4), (10, 8, 0), (10, 8, sc.MAX_K + 1)):
        assert f(N, D, k) == 0, (N, D, k)
    sizes = [f(N, 64, 320) for N in (0, 1, 1023, 1024, 1025, 5000, 500_000, 2_000_000, (1 << 31) - 1)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] >= 8 * ((1 << 31) - 1)
    assert f(5000, sc.MAX_DIM, sc.MAX_K) >= f(5000, 1, 1)


def test_wide_seed_argument_checks():
    from opengaussian_amd import kmeans
    x = torch.zeros(10, 8)
    with pytest.raises(ValueError, match="metric"):
        kmeans.wide_seed(x, 3, metric="l1")
    with pytest.raises(ValueError, match=r"\[N, D\]"):
        kmeans.wide_seed(torch.zeros(10), 3)
    with pytest.raises(ValueError, match="k=0"):
        kmeans.wide_seed(x, 0)
    with pytest.raises(ValueError, match="k="):
        kmeans.wide_seed(x, sc.MAX_K + 1)
    with pytest.raises(ValueError, match="D="):
        kmeans.wide_seed(torch.zeros(4, sc.MAX_DIM + 1), 2)
    with pytest.raises(ValueError, match="weights"):
        kmeans.wide_seed(x, 3, weights=torch.ones(9))
    with pytest.raises(ValueError, match="seed"):
        kmeans.wide_seed(x, 3, seed=-1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        kmeans.wide_seed(x, 3)


def test_build_codebook_init_checks():
    from opengaussian_amd import query
    x = torch.ones(10, 8)
    with pytest.raises(ValueError, match="init"):
        query.build_codebook(x, 3, init="kmeans")
    with pytest.raises(ValueError, match="init"):
        query.build_codebook(x, 3, init=torch.ones(2, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        query.build_codebook(x, 3, init="k-means++")
