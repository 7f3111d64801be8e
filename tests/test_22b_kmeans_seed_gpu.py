"""GPU: the wide seeding (include/ogs_kmeans.h: ogs_kmeans_wide_seed) through the C ABI and through opengaussian_amd.kmeans.wide_seed /
query.build_codebook(init="k-means++"), against tests/kmeans_seed_restatement.py.

The header fixes every step, so rows, C, ids, d2 and stats[0] are np.array_equal to the restatement: no tolerance anywhere.  Every
buffer the library writes has canaries on both sides, and every shape runs with its fp32 arrays 16-byte aligned and 4 bytes past
that.  The conditions of the pruning and quality tests (at least half of the pairs skipped; lower inertia than random rows; one leaf
per seeded planted cluster) are the issue's; tests/test_kmeans_seed_host.py checks the first two on the restatement alone."""
import numpy as np
import pytest
import torch

from tests import kmeans_seed_cases as sc
from tests import kmeans_seed_restatement as sr

pytestmark = pytest.mark.gpu

GUARD = 256
I_CANARY, F_CANARY, B_CANARY, S_CANARY = -77777, sc.C_FILL, 0xA5, -4242424242


def _L():
    from opengaussian_amd import _lib
    return _lib


def _guarded(numel, dtype, fill, dev, off=0):
    buf = torch.full((numel + 2 * GUARD + 4,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD + off:GUARD + off + numel]


def _intact(buf, view, fill):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == fill).all()) and bool((buf[lo + view.numel():] == fill).all())


class Got:
    pass


def run_seed(dev, X, k, w=None, scale=None, seed=0, prune=1, misalign=False, ids=True, d2=True, stats=True):
    """one ogs_kmeans_wide_seed call on guarded buffers; every canary is checked; outputs as NumPy (None where not asked for)"""
    L = _L()
    lib = L.lib()
    off = 1 if misalign else 0
    N, D = X.shape
    bufs = []

    def put(a):
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        buf, v = _guarded(a.size, torch.float32, F_CANARY, dev, off)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4 * off
        bufs.append((buf, v, F_CANARY))
        return v

    def out(n, dtype, fill, o=off):
        buf, v = _guarded(n, dtype, fill, dev, o)
        bufs.append((buf, v, fill))
        return v

    p = lambda t: L.ptr(t) if t is not None and t.numel() else None
    Xd = put(X)
    wd = None if w is None else put(w)
    sd = None if scale is None else put(scale)
    nbytes = int(lib.ogs_kmeans_wide_seed_tmp_bytes(N, D, k))
    assert nbytes > 0
    tmp = out(nbytes, torch.uint8, B_CANARY, 0)
    Cd = out(k * D, torch.float32, F_CANARY)
    rows_d = out(k, torch.int32, I_CANARY)
    ids_d = out(N, torch.int32, I_CANARY) if ids else None
    d2_d = out(N, torch.float32, F_CANARY) if d2 else None
    stats_d = out(4, torch.int64, S_CANARY, 0) if stats else None
    rc = lib.ogs_kmeans_wide_seed(p(Xd), p(wd), p(sd), N, D, k, int(seed), int(prune), p(Cd), p(rows_d), p(ids_d), p(d2_d), p(stats_d),
                                  p(tmp), nbytes, torch.cuda.current_stream().cuda_stream)
    L.check(rc, "ogs_kmeans_wide_seed")
    torch.cuda.synchronize()
    for buf, v, fill in bufs:
        assert _intact(buf, v, fill), ("canary", N, D, k, misalign)
    assert bool((Xd.cpu() == torch.from_numpy(np.ascontiguousarray(X, np.float32).reshape(-1))).all())
    g = Got()
    g.C = Cd.cpu().numpy().reshape(k, D)
    g.rows = rows_d.cpu().numpy().astype(np.int64)
    g.ids = None if ids_d is None else ids_d.cpu().numpy().astype(np.int64)
    g.d2 = None if d2_d is None else d2_d.cpu().numpy()
    g.stats = None if stats_d is None else stats_d.cpu().numpy()
    return g


def assert_equal(got, want, N, what):
    assert np.array_equal(got.rows, want.rows), (what, got.rows, want.rows)
    assert np.array_equal(got.C.view(np.uint32), want.C.view(np.uint32)), what
    if want.seeded > 0:
        if got.ids is not None:
            assert np.array_equal(got.ids, want.ids), what
        if got.d2 is not None:
            assert np.array_equal(got.d2.view(np.uint32), want.d2.view(np.uint32)), what
    if got.stats is not None:
        assert got.stats[0] == want.seeded, (what, got.stats)
        assert got.stats[1] >= 0 and got.stats[2] >= 0 and got.stats[3] == 0, (what, got.stats)
        assert got.stats[1] + got.stats[2] == N * max(want.seeded - 1, 0), (what, got.stats)


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


def test_block_size_is_what_the_shapes_assume():
    assert _L().lib().ogs_kmeans_wide_seed_rows() == sc.SEED_ROWS


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "plus4"])
@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "N%d-D%d-k%d" % s)
def test_shapes_equal_the_restatement(dev, shape, misalign):
    N, D, k = shape
    X, w, scale, seed, want = sc.shape_case(N, D, k)
    got = run_seed(dev, X, k, w, scale, seed, prune=1, misalign=misalign)
    assert_equal(got, want, N, shape)


def test_zero_weights_and_the_row_a_uniform_draw_takes(dev):
    N, D, k = 700, 24, 9
    rng = np.random.default_rng(31)
    X = rng.normal(size=(N, D)).astype(np.float32)
    uniform_row = sr.first_pick(np.ones(N, np.float32), 77)
    w = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
    w[::3] = 0.0
    w[uniform_row] = 0.0
    want = sr.seed(X, k, w, None, 77, C_fill=sc.C_FILL)
    assert uniform_row not in want.rows and (w[want.rows] > 0).all()
    for misalign in (False, True):
        assert_equal(run_seed(dev, X, k, w, None, 77, misalign=misalign), want, N, "zero weights")


def test_all_weight_on_the_last_row(dev):
    N, D, k = 2 * sc.SEED_ROWS + 5, 10, 3
    X = np.random.default_rng(32).normal(size=(N, D)).astype(np.float32)
    w = np.zeros(N, np.float32)
    w[-1] = 0.375
    want = sr.seed(X, k, w, None, 5, C_fill=sc.C_FILL)
    got = run_seed(dev, X, k, w, None, 5)
    assert want.seeded == 1 and want.rows[0] == N - 1
    assert_equal(got, want, N, "last row")
    assert got.stats[0] == 1 and (got.rows[1:] == -1).all()


def test_all_weights_zero(dev):
    N, D, k = 300, 7, 4
    X = np.random.default_rng(33).normal(size=(N, D)).astype(np.float32)
    got = run_seed(dev, X, k, np.zeros(N, np.float32), None, 1)
    assert got.stats[0] == 0 and (got.rows == -1).all() and (got.C == F_CANARY).all()
    assert got.stats[1] == 0 and got.stats[2] == 0


def test_fewer_distinct_points_than_k(dev):
    X, which = sc.duplicated()
    m, k = 7, 12
    want = sr.seed(X, k, None, None, 1, C_fill=sc.C_FILL)
    for prune in (0, 1):
        got = run_seed(dev, X, k, None, None, 1, prune=prune)
        assert_equal(got, want, len(X), "duplicates")
        assert got.stats[0] == m and (got.rows[m:] == -1).all() and (got.C[m:] == F_CANARY).all()
        assert sorted(which[got.rows[:m]].tolist()) == list(range(m)) and (got.d2 == 0).all()


def test_row_scale_gives_unit_centres(dev):
    """cosine: row_scale = 1 / |x| (float64, rounded once): a centre is a row scaled element by element, so its norm is within
    (1/2 + 1/2) 2^-24 of 1 to first order -- inside the issue's 4 * 2^-24"""
    N, D, k = 1500, 67, 20
    rng = np.random.default_rng(34)
    X = (rng.normal(size=(N, D)) * np.exp2(rng.integers(-4, 5, size=(N, 1)))).astype(np.float32)
    scale = (1.0 / np.linalg.norm(X.astype(np.float64), axis=1)).astype(np.float32)
    want = sr.seed(X, k, None, scale, 3, C_fill=sc.C_FILL)
    for misalign in (False, True):
        got = run_seed(dev, X, k, None, scale, 3, misalign=misalign)
        assert_equal(got, want, N, "row_scale")
        norms = np.linalg.norm(got.C.astype(np.float64), axis=1)
        assert (np.abs(norms - 1.0) <= 4 * sr.U).all(), float(np.abs(norms - 1.0).max())


def test_null_outputs(dev):
    N, D, k = 1300, 33, 6
    X = np.random.default_rng(35).normal(size=(N, D)).astype(np.float32)
    want = sr.seed(X, k, None, None, 8, C_fill=sc.C_FILL)
    assert_equal(run_seed(dev, X, k, None, None, 8, ids=False, d2=False, stats=False), want, N, "all NULL")
    assert_equal(run_seed(dev, X, k, None, None, 8, ids=False), want, N, "ids NULL")
    assert_equal(run_seed(dev, X, k, None, None, 8, d2=False, misalign=True), want, N, "d2 NULL")


def test_two_identical_calls_give_the_same_bytes(dev):
    X, _ = sc.mixture(67, 0)
    a = run_seed(dev, X, 32, None, None, 0)
    b = run_seed(dev, X, 32, None, None, 0)
    for name in ("C", "rows", "ids", "d2", "stats"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name


def test_bad_arguments(dev):
    L = _L()
    lib = L.lib()
    x = torch.zeros(64, 8, device=dev)
    C = torch.zeros(4, 8, device=dev)
    rows = torch.zeros(4, dtype=torch.int32, device=dev)
    nbytes = int(lib.ogs_kmeans_wide_seed_tmp_bytes(64, 8, 4))
    tmp = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda X, N, D, k, Cp, rp, tp, tb: lib.ogs_kmeans_wide_seed(X, None, None, N, D, k, 0, 1, Cp, rp, None, None, None, tp, tb, s)
    good = (L.ptr(x), 64, 8, 4, L.ptr(C), L.ptr(rows), L.ptr(tmp), nbytes)
    assert call(*good) == 0
    for i, bad in ((0, None), (1, -1), (1, 1 << 31), (2, 0), (2, sc.MAX_DIM + 1), (3, 0), (3, sc.MAX_K + 1), (4, None), (5, None),
                   (6, None), (6, L.ptr(tmp) + 4), (7, nbytes - 1)):
        args = list(good)
        args[i] = bad
        assert call(*args) < 0, (i, bad)
    assert call(None, 0, 8, 4, None, None, None, 0) == 0            # N = 0: nothing is launched, nothing is needed
    torch.cuda.synchronize()


@pytest.mark.parametrize("D", sc.MIXTURE_DIMS)
def test_pruning_changes_no_byte_and_skips_most_pairs(dev, D):
    for seed in sc.MIXTURE_SEEDS:
        X, _ = sc.mixture(D, seed)
        want, skipped, pairs, _ = sc.mixture_seeded(D, seed)
        on = run_seed(dev, X, sc.MIXTURE_K, None, None, seed, prune=1)
        off = run_seed(dev, X, sc.MIXTURE_K, None, None, seed, prune=0)
        assert_equal(on, want, len(X), ("prune", D, seed))
        assert_equal(off, want, len(X), ("no prune", D, seed))
        for name in ("C", "rows", "ids", "d2"):
            assert getattr(on, name).tobytes() == getattr(off, name).tobytes(), (name, D, seed)
        total = len(X) * (on.stats[0] - 1)
        print(f"D={D} seed={seed}: {on.stats[2]} of {total} pairs skipped ({on.stats[2] / total:.3f})")
        assert on.stats[1] + on.stats[2] == total and off.stats[1] + off.stats[2] == total
        assert 2 * on.stats[2] >= total
        assert off.stats[2] == 0
        assert on.stats[2] == skipped               # the rule is fp32 arithmetic on equal bytes: the same count as the restatement


def test_wrapper_equals_the_restatement(dev):
    from opengaussian_amd import kmeans
    X, _ = sc.mixture(16, 2)
    want = sc.mixture_seeded(16, 2)[0]
    for prune in (True, False):
        C, rows, ids, d2, stats = kmeans.wide_seed(torch.from_numpy(X).to(dev), sc.MIXTURE_K, "l2", None, 2, prune)
        assert rows.dtype == torch.int64 and ids.dtype == torch.int64 and stats.dtype == torch.int64 and C.dtype == torch.float32
        assert np.array_equal(rows.cpu().numpy(), want.rows) and np.array_equal(ids.cpu().numpy(), want.ids)
        assert np.array_equal(C.cpu().numpy(), want.C) and np.array_equal(d2.cpu().numpy(), want.d2)
        assert int(stats[0]) == sc.MIXTURE_K


def test_wrapper_cosine(dev):
    """the wrapper's row scale is torch's 1 / |x|; zero rows weigh nothing and are never picked"""
    from opengaussian_amd import kmeans
    N, D, k = 900, 40, 12
    rng = np.random.default_rng(36)
    X = (rng.normal(size=(N, D)) * np.exp2(rng.integers(-2, 3, size=(N, 1)))).astype(np.float32)
    X[::7] = 0.0
    w = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
    Xd = torch.from_numpy(X).to(dev)
    norm = Xd.norm(dim=1)
    scale = torch.where(norm > 0, 1.0 / norm, torch.zeros_like(norm)).cpu().numpy()
    want = sr.seed(X, k, np.where(np.arange(N) % 7 == 0, 0.0, w).astype(np.float32), scale, 6)
    C, rows, ids, d2, stats = kmeans.wide_seed(Xd, k, "cosine", torch.from_numpy(w).to(dev), 6)
    assert np.array_equal(rows.cpu().numpy(), want.rows) and (rows.cpu().numpy() % 7 != 0).all()
    assert np.array_equal(C.cpu().numpy(), want.C) and np.array_equal(ids.cpu().numpy(), want.ids)
    assert np.array_equal(d2.cpu().numpy(), want.d2) and int(stats[0]) == k


def _own_leaves(labels, leaf_ind, clusters):
    """the leaf most rows of each cluster went to"""
    return {c: int(np.bincount(leaf_ind[labels == c]).argmax()) for c in clusters}


@pytest.mark.parametrize("D", sc.MIXTURE_DIMS)
def test_codebook_from_seeded_centres(dev, D):
    """build_codebook(init="k-means++", iters=5): lower inertia than init=None for every seed, and no two planted clusters that
    hold a seeded centre end up sharing a leaf"""
    from opengaussian_amd import query
    for seed in sc.MIXTURE_SEEDS:
        X, labels = sc.mixture(D, seed)
        Xd = torch.from_numpy(X).to(dev)
        pp = query.build_codebook(Xd, sc.MIXTURE_K, metric="l2", iters=5, init="k-means++", seed=seed)
        rnd = query.build_codebook(Xd, sc.MIXTURE_K, metric="l2", iters=5, init=None, seed=seed)
        i_pp, i_rnd = float(pp.dist.double().sum()), float(rnd.dist.double().sum())
        print(f"D={D} seed={seed}: inertia {i_pp:.1f} from k-means++, {i_rnd:.1f} from random rows")
        assert i_pp < i_rnd, (D, seed, i_pp, i_rnd)
        seeded = sorted(set(labels[sc.mixture_seeded(D, seed)[0].rows].tolist()))
        leaves = _own_leaves(labels, pp.leaf_ind.cpu().numpy(), seeded)
        assert len(set(leaves.values())) == len(seeded), (D, seed, leaves)
        assert int(pp.occu_count.sum()) == len(X) and pp.leaf_feat.shape == (sc.MIXTURE_K, D)


def test_codebook_refuses_too_few_distinct_rows(dev):
    from opengaussian_amd import query
    X, which = sc.duplicated()
    with pytest.raises(ValueError, match="7 of k=12"):
        query.build_codebook(torch.from_numpy(X).to(dev), 12, metric="l2", init="k-means++")
    cb = query.build_codebook(torch.from_numpy(X).to(dev), 7, metric="l2", init="k-means++", iters=2)
    # one leaf per distinct point (a centre is the rounded mean of equal rows, so dist is tiny, not 0)
    assert len(set(zip(which.tolist(), cb.leaf_ind.cpu().tolist()))) == 7 and (cb.occu_count > 0).all()


def test_init_none_keeps_its_bytes(dev):
    """init=None and a tensor init do not go near the seeding: the same codebook as before, run after run"""
    from opengaussian_amd import query
    X, _ = sc.mixture(16, 0)
    Xd = torch.from_numpy(X).to(dev)
    a = query.build_codebook(Xd, 8, metric="l2", iters=2, seed=3)
    gen = torch.Generator().manual_seed(3)
    init = Xd[torch.randperm(len(X), generator=gen)[:8].to(dev)]
    b = query.build_codebook(Xd, 8, metric="l2", iters=2, init=init)
    assert torch.equal(a.leaf_feat, b.leaf_feat) and torch.equal(a.leaf_ind, b.leaf_ind)
