"""GPU: the wide k-means (include/ogs_kmeans.h: ogs_kmeans_wide_assign / _update / _inertia / _lloyd) through the C ABI and through
opengaussian_amd.kmeans / query.build_codebook, against tests/kmeans_wide_restatement.py (NumPy float64).

Every buffer the library writes has canaries on both sides, and every case runs with its fp32 arrays 16-byte aligned and 4 bytes
past that.  Bars (U = 2^-24, inputs exact fp32; all of them hold for ANY summation order):
  ids, planted     EQUAL to the float64 arg-min: the gaps are orders of magnitude above any rounding
  ids, random      cost64(x, c_got) - min_c cost64(x, c) <= tau_i, tau_i = 4 (8 D + 64) U max_c S for L2 (two scores compared, and
                   a squared distance is minus twice a score), 2 (8 D + 64) U max_c S for cosine (restatement.score_slack: S and
                   why 8 D + 64); and at most 1 % of the rows differ from the float64 arg-min at all
  dist (L2)        |got - d2_64| <= (D + 4) U d2_64 + 2 U d2_64: the sum of D rounded squares in any order, plus the rounding of
                   every difference (it is squared: twice)
  dist (cosine)    |got - (1 - cos_64)| <= (D + 4) U sum |x c| / |x| + 2 U: dot and norm chains, the square root, the quotient and
                   the subtraction from 1
  centres (L2)     |got - f64| <= (m + 6) U sum |w x| / sum w per element, m = the centre's rows; counts within (m + 2) U sum w
  centres (cos)    unit norm within 4 U; per element the L2 bound e_j of the mean v carried through c = v / |v|:
                   e_j / |v| + |c_j| (|e| / |v| + 2 U)
  inertia          |got - f64| <= (N + D + 8) U sum w dist, f64 = the float64 sum over the float64 distances to the centres the GPU
                   held at that assignment (the distances' own bound, N roundings of the fp64 sum to spare)"""
import numpy as np
import pytest
import torch

from tests import kmeans_wide_cases as wc
from tests import kmeans_wide_restatement as wr

pytestmark = pytest.mark.gpu

U = wr.U
GUARD = 256
I_CANARY, F_CANARY, B_CANARY = -77777, -12345.0, 0xA5
CODE = {"l2": 0, "cosine": 1}


def _L():
    from opengaussian_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(numel, dtype, fill, dev, off=0):
    """a buffer with canaries on both sides; off: elements past the aligned start (fp32: 1 = 4 bytes off a 16-byte boundary)"""
    buf = torch.full((numel + 2 * GUARD + 4,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD + off:GUARD + off + numel]


def _intact(buf, view, fill):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == fill).all()) and bool((buf[lo + view.numel():] == fill).all())


def _floats(a, dev, off=0):
    """a's values on the device, aligned to 16 bytes or 4 bytes past that, with canaries around them"""
    a = np.ascontiguousarray(a, np.float32)
    buf, v = _guarded(a.size, torch.float32, F_CANARY, dev, off)
    v.copy_(torch.from_numpy(a.reshape(-1)))
    assert v.data_ptr() % 16 == 4 * off
    return buf, v


class Run:
    """device copies of one problem (X, C, optional w) and guarded outputs; every call checks all canaries"""

    def __init__(self, dev, X, C, metric, w=None, misalign=False):
        self.L = _L()
        self.lib = self.L.lib()
        self.dev, self.metric, self.off = dev, CODE[metric], 1 if misalign else 0
        (self.N, self.D), self.k = X.shape, C.shape[0]
        self.bufs = []
        self.X = self._in(X)
        self.C = self._in(C)
        self.w = None if w is None else self._in(w)
        self.nbytes = int(self.lib.ogs_kmeans_wide_tmp_bytes(self.N, self.D, self.k))
        assert self.nbytes > 0
        self.tmp = self._out(self.nbytes, torch.uint8, B_CANARY, off=0)
        self.ids = self._out(self.N, torch.int32, I_CANARY)
        self.dist = self._out(self.N, torch.float32, F_CANARY)
        self.counts = self._out(self.k, torch.float32, F_CANARY)

    def _in(self, a):
        buf, v = _floats(a, self.dev, self.off)
        self.bufs.append((buf, v, F_CANARY))
        return v

    def _out(self, n, dtype, fill, off=None):
        buf, v = _guarded(n, dtype, fill, self.dev, self.off if off is None else off)
        self.bufs.append((buf, v, fill))
        return v

    def _done(self, rc, what):
        self.L.check(rc, what)
        torch.cuda.synchronize()
        for buf, v, fill in self.bufs:
            assert _intact(buf, v, fill), (what, self.N, self.D, self.k)

    def p(self, t):
        return self.L.ptr(t) if t is not None and t.numel() else None

    def assign(self, dist=True):
        self._done(self.lib.ogs_kmeans_wide_assign(self.p(self.X), self.N, self.D, self.p(self.C), self.k, self.metric, self.p(self.ids),
                                                   self.p(self.dist) if dist else None, self.p(self.tmp), self.nbytes, _stream()),
                   "ogs_kmeans_wide_assign")
        return self.ids.cpu().numpy().astype(np.int64), self.dist.cpu().numpy()

    def update(self):
        self._done(self.lib.ogs_kmeans_wide_update(self.p(self.X), self.p(self.w), self.N, self.D, self.p(self.ids), self.k, self.metric,
                                                   self.p(self.C), self.p(self.counts), self.p(self.tmp), self.nbytes, _stream()),
                   "ogs_kmeans_wide_update")
        return self.C.cpu().numpy().reshape(self.k, self.D), self.counts.cpu().numpy()

    def inertia(self):
        total = self._out(1, torch.float64, -1.0, off=0)
        self._done(self.lib.ogs_kmeans_wide_inertia(self.p(self.dist), self.p(self.w), self.N, self.p(total), self.p(self.tmp), self.nbytes,
                                                    _stream()), "ogs_kmeans_wide_inertia")
        return float(total.cpu()[0])

    def lloyd(self, iters):
        total = self._out(iters + 1, torch.float64, -1.0, off=0)
        self._done(self.lib.ogs_kmeans_wide_lloyd(self.p(self.X), self.p(self.w), self.N, self.D, self.p(self.C), self.k, self.metric, iters,
                                                  self.p(self.ids), self.p(self.dist), self.p(self.counts), self.p(total), self.p(self.tmp),
                                                  self.nbytes, _stream()), "ogs_kmeans_wide_lloyd")
        return (self.ids.cpu().numpy().astype(np.int64), self.dist.cpu().numpy(), self.C.cpu().numpy().reshape(self.k, self.D),
                self.counts.cpu().numpy(), total.cpu().numpy())


def assert_dist(got, X, C, ids, metric, what):
    want = wr.dist_of(X, C, ids, metric)
    D = X.shape[1]
    if metric == "l2":
        bar = (D + 4) * U * want + 2 * U * want
    else:
        x, c = X.astype(np.float64), C.astype(np.float64)[ids]
        n = np.linalg.norm(x, axis=1)
        bar = (D + 4) * U * np.abs(x * c).sum(axis=1) / np.where(n > 0, n, 1.0) + 2 * U
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bar).all(), (what, float((err / np.maximum(bar, 1e-300)).max()))


# ---- 1. planted clusters ------------------------------------------------------------------------------------------------------
def test_sizes_are_the_ones_the_cases_bracket():
    lib = _L().lib()
    assert (int(lib.ogs_kmeans_wide_row_tile()), int(lib.ogs_kmeans_wide_centre_tile()), int(lib.ogs_kmeans_wide_dim_step()),
            int(lib.ogs_kmeans_wide_stage()), int(lib.ogs_kmeans_wide_max_dim()), int(lib.ogs_kmeans_wide_max_k())) == \
        (wc.ROW_TILE, wc.CENTRE_TILE, wc.DIM_STEP, wc.STAGE, wc.MAX_DIM, wc.MAX_K)


@pytest.mark.parametrize("metric", wc.METRICS)
@pytest.mark.parametrize("shape", wc.PLANTED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_planted_ids_equal_the_float64_argmin(gpu_device, shape, metric):
    X, C, labels = wc.planted(*shape, metric)
    want, _ = wr.assign(X, C, metric)
    assert np.array_equal(want, labels)
    for misalign in (False, True):
        run = Run(gpu_device, X, C, metric, misalign=misalign)
        ids, dist = run.assign()
        assert np.array_equal(ids, want), (shape, metric, misalign, int((ids != want).sum()))
        assert_dist(dist, X, C, ids, metric, (shape, metric, misalign))
        run.ids.fill_(I_CANARY)
        ids2, _ = run.assign(dist=False)                                       # dist is optional
        assert np.array_equal(ids2, want)


def test_planted_through_python(gpu_device):
    from opengaussian_amd import kmeans
    for metric in wc.METRICS:
        X, C, labels = wc.planted(1000, 100, 37, metric)
        ids, dist = kmeans.wide_assign(torch.from_numpy(X).to(gpu_device), torch.from_numpy(C).to(gpu_device), metric)
        assert ids.dtype == torch.int64 and dist.dtype == torch.float32 and ids.shape == dist.shape == (1000,)
        assert np.array_equal(ids.cpu().numpy(), labels)
        assert_dist(dist.cpu().numpy(), X, C, labels, metric, metric)


def test_no_rows_and_bad_arguments(gpu_device):
    L = _L()
    lib = L.lib()
    X, C, _ = wc.planted(63, 17, 5, "l2")
    run = Run(gpu_device, X, C, "l2")
    s, INVALID = _stream(), -1
    before = run.C.clone()
    # N = 0: nothing is read or written, an update keeps every centre and reports empty counts
    assert lib.ogs_kmeans_wide_assign(None, 0, 17, run.p(run.C), 5, 0, None, None, None, 0, s) == 0
    assert lib.ogs_kmeans_wide_update(None, None, 0, 17, None, 5, 0, run.p(run.C), run.p(run.counts), None, 0, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(run.C, before) and bool((run.counts == 0).all())
    a = (run.p(run.X), 63, 17, run.p(run.C), 5, 0, run.p(run.ids), run.p(run.dist), run.p(run.tmp), run.nbytes, s)

    def bad(i, v):
        b = list(a)
        b[i] = v
        return lib.ogs_kmeans_wide_assign(*b)
    rcs = [bad(1, -1), bad(2, 0), bad(2, wc.MAX_DIM + 1), bad(4, 0), bad(4, wc.MAX_K + 1), bad(5, 2), bad(0, None), bad(3, None),
           bad(6, None), bad(8, None), bad(9, run.nbytes - 1)]
    assert all(rc < 0 for rc in rcs), rcs
    assert lib.ogs_kmeans_wide_inertia(run.p(run.dist), None, 63, None, run.p(run.tmp), run.nbytes, s) < 0
    assert lib.ogs_kmeans_wide_lloyd(run.p(run.X), None, 63, 17, run.p(run.C), 5, 0, -1, run.p(run.ids), None, None, None, run.p(run.tmp),
                                     run.nbytes, s) < 0
    torch.cuda.synchronize()
    assert bool((run.ids == I_CANARY).all())                                   # the refused calls launched nothing


# ---- 2. random data: near-minimiser bar, 4. dist -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in wc.RANDOM_CASES])
def test_random_ids_are_near_minimisers(gpu_device, name):
    X, C, metric = wc.random_case(name)
    cost = wr.cost_matrix(X, C, metric)
    want = cost.argmin(axis=1)
    tau = (4 if metric == "l2" else 2) * wr.score_slack(X, C, metric)
    rows = np.arange(len(X))
    for misalign in (False, True):
        ids, dist = Run(gpu_device, X, C, metric, misalign=misalign).assign()
        assert ids.min() >= 0 and ids.max() < len(C)
        excess = cost[rows, ids] - cost[rows, want]
        differ = float((ids != want).mean())
        print(f"{name} misalign={misalign}: rows off the float64 arg-min {differ:.4f}, max excess / tau {float((excess / tau).max()):.3g}")
        assert (excess <= tau).all(), (name, float((excess / tau).max()))
        assert differ <= 0.01, (name, differ)
        assert_dist(dist, X, C, ids, metric, name)


# ---- 3. ties, duplicates, scaling ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", wc.METRICS)
def test_duplicate_centres_go_to_the_lower_index(gpu_device, metric):
    X, C, labels = wc.planted(300, 33, 17, metric)
    # every centre twice: in the same tile (c, c + 17 -> 34 centres, three tiles) and, with the pair order reversed, across tiles
    for order in (np.concatenate([np.arange(17), np.arange(17)]), np.concatenate([np.arange(17), np.arange(16, -1, -1)])):
        CC = C[order]
        want = np.array([int(np.flatnonzero(order == l)[0]) for l in labels])
        ids, _ = Run(gpu_device, X, CC, metric).assign()
        assert np.array_equal(ids, want) and np.array_equal(ids, wr.assign(X, CC, metric)[0])
    # a duplicate past one stage of packed centres
    X, C, labels = wc.planted(50, 17, wc.STAGE + 1, metric)
    CC = np.concatenate([C, C[labels[:7]]])
    ids, _ = Run(gpu_device, X, CC, metric).assign()
    assert np.array_equal(ids, labels)


def test_rows_equal_to_a_centre(gpu_device):
    X, C, metric = wc.random_case("uniform+100")
    XX = np.concatenate([C[:40], X[:100]])
    ids, dist = Run(gpu_device, XX, C, metric).assign()
    assert np.array_equal(ids[:40], np.arange(40))
    n2 = (XX[:40].astype(np.float64) ** 2).sum(axis=1)
    assert (dist[:40] <= (XX.shape[1] + 4) * U * n2).all() and (dist[:40] == 0).all()


def test_cosine_scaling_and_the_zero_row(gpu_device):
    X, C, metric = wc.random_case("normal/64")
    base, _ = Run(gpu_device, X, C, metric).assign()
    scale = np.exp2(np.random.default_rng(5).integers(-20, 21, size=(len(X), 1))).astype(np.float32)
    ids, _ = Run(gpu_device, X * scale, C, metric, misalign=True).assign()
    assert ids.tobytes() == base.tobytes()
    Z = X.copy()
    Z[[0, 63, 64, 500, len(Z) - 1]] = 0
    ids, dist = Run(gpu_device, Z, C, metric).assign()
    for r in (0, 63, 64, 500, len(Z) - 1):
        assert ids[r] == 0 and dist[r] == 1.0, r


# ---- 5. update ------------------------------------------------------------------------------------------------------------------
def assert_update(gotC, gotN, X, ids, prev, metric, w, what):
    wantC, wantN, scale, m = wr.update(X, ids, prev, metric, w)
    e = (m[:, None] + 6) * U * scale
    moved = scale.any(axis=1) | (wantN > 0)
    if metric == "cosine":
        sums = np.zeros_like(wantC)
        ww = np.ones(len(X)) if w is None else w.astype(np.float64)
        np.add.at(sums, ids, ww[:, None] * X.astype(np.float64))
        vn = np.linalg.norm(sums / np.where(wantN > 0, wantN, 1.0)[:, None], axis=1)
        vn = np.where(vn > 0, vn, 1.0)
        e = e / vn[:, None] + np.abs(wantC) * (np.linalg.norm(e, axis=1) / vn + 2 * U)[:, None]
        norms = np.linalg.norm(gotC.astype(np.float64)[moved], axis=1)
        assert (np.abs(norms - 1) <= 4 * U).all(), (what, float(np.abs(norms - 1).max() / U))
    err = np.abs(gotC.astype(np.float64) - wantC)
    assert (err[moved] <= e[moved]).all(), (what, float((err[moved] / np.maximum(e[moved], 1e-300)).max()))
    assert gotC[~moved].tobytes() == prev[~moved].tobytes(), what                 # an empty centre keeps its bytes
    assert (np.abs(gotN - wantN) <= (m + 2) * U * wantN).all() and (gotN[wantN == 0] == 0).all(), what


@pytest.mark.parametrize("metric", wc.METRICS)
def test_update_against_float64(gpu_device, metric):
    X, C, _ = wc.random_case("uniform/17" if metric == "l2" else "normal/512")
    N, k = len(X), len(C)
    rng = np.random.default_rng(9)
    ids = rng.integers(0, k, size=N)
    ids[ids % 7 == 3] = 0                                                      # empty centres, and one with many rows
    w = wc.weights(N, 2)
    for weights, misalign in ((None, False), (w, True)):
        run = Run(gpu_device, X, C, metric, weights, misalign)
        run.ids.copy_(torch.from_numpy(ids.astype(np.int32)))
        gotC, gotN = run.update()
        assert_update(gotC, gotN, X, ids, C, metric, weights, (metric, misalign))
        assert (np.bincount(ids, minlength=k) == 0).any()
    # rows of weight 0 change nothing beyond the bound: the same update without them
    keep = w > 0
    run = Run(gpu_device, X[keep], C, metric, w[keep])
    run.ids.copy_(torch.from_numpy(ids[keep].astype(np.int32)))
    gotC, gotN = run.update()
    assert_update(gotC, gotN, X, ids, C, metric, w, (metric, "zero-weight rows left out"))
    # a centre whose rows all weigh 0 keeps its bytes
    w0 = w.copy()
    w0[ids == 1] = 0
    assert (ids == 1).any()
    run = Run(gpu_device, X, C, metric, w0)
    run.ids.copy_(torch.from_numpy(ids.astype(np.int32)))
    gotC, gotN = run.update()
    assert gotC[1].tobytes() == C[1].tobytes() and gotN[1] == 0


def test_update_through_python(gpu_device):
    from opengaussian_amd import kmeans
    X, C, labels = wc.planted(257, 512, 64, "l2")
    centers = torch.from_numpy(C + 1.0).to(gpu_device)
    counts = kmeans.wide_update(torch.from_numpy(X).to(gpu_device), torch.from_numpy(labels).to(gpu_device), centers, "l2")
    assert_update(centers.cpu().numpy(), counts.cpu().numpy(), X, labels, C + 1.0, "l2", None, "python")
    assert np.abs(centers.cpu().numpy() - C).max() < 1e-2


# ---- 6. Lloyd -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", wc.METRICS)
def test_lloyd_is_the_sequence_of_the_three_calls(gpu_device, metric):
    X, C, _ = wc.random_case("uniform+100" if metric == "l2" else "normal/64")
    C, w, iters = C[:23], wc.weights(len(X), 3), 3
    N, D = X.shape
    step = Run(gpu_device, X, C, metric, w, misalign=True)
    totals = []
    for t in range(iters + 1):
        held = step.C.cpu().numpy().reshape(len(C), D)
        ids, dist = step.assign()
        totals.append(step.inertia())
        want = wr.inertia(wr.dist_of(X, held, ids, metric), w)
        assert abs(totals[-1] - want) <= (N + D + 8) * U * want, (metric, t, totals[-1], want)
        if t < iters:
            step.update()
    one = Run(gpu_device, X, C, metric, w, misalign=True)
    got = one.lloyd(iters)
    seq = (ids, dist, step.C.cpu().numpy().reshape(len(C), D), step.counts.cpu().numpy(), np.array(totals))
    for a, b, what in zip(got, seq, ("ids", "dist", "centres", "counts", "inertia")):
        assert a.tobytes() == b.tobytes(), (metric, what)
    again = Run(gpu_device, X, C, metric, w, misalign=True).lloyd(iters)
    for a, b, what in zip(got, again, ("ids", "dist", "centres", "counts", "inertia")):
        assert a.tobytes() == b.tobytes(), (metric, what, "two runs")
    # every L2 update lowers the weighted inertia, up to the rounding of the distances (the dist bar, on both sides).  Cosine: that
    # holds for unit rows only (the mean weighs a row by its norm, 1 - cos does not): test_lloyd_recovers_a_planted_partition
    if metric == "l2":
        assert (np.diff(got[4]) <= 2 * (D + 6) * U * got[4][:-1]).all() and got[4][-1] < got[4][0], got[4]


@pytest.mark.parametrize("metric", wc.METRICS)
def test_lloyd_recovers_a_planted_partition(gpu_device, metric):
    from opengaussian_amd import kmeans
    X, C, labels = wc.planted(1000, 100, 37, metric)
    if metric == "cosine":
        X = wc.unit(X)
    first = np.array([int(np.flatnonzero(labels == c)[0]) for c in range(37)])
    init = X[first]
    ids, dist, centres, counts, total = Run(gpu_device, X, init, metric).lloyd(3)
    assert np.array_equal(ids, labels) and np.array_equal(counts, np.bincount(labels, minlength=37))
    assert np.abs(centres - C).max() < 1e-2
    # non-increasing within the dist bar on both sides: relative to the distances for L2, absolute (D + 6) U per unit row for cosine
    slack = 2 * (100 + 6) * U * (total[:-1] if metric == "l2" else len(X))
    assert (np.diff(total) <= slack).all(), total
    centers = torch.from_numpy(init).to(gpu_device)
    pids, pdist, pcounts, ptotal = kmeans.wide_lloyd(torch.from_numpy(X).to(gpu_device), centers, 3, metric)
    assert pids.dtype == torch.int64 and ptotal.dtype == torch.float64 and ptotal.shape == (4,)
    assert np.array_equal(pids.cpu().numpy(), ids) and pdist.cpu().numpy().tobytes() == dist.tobytes()
    assert centers.cpu().numpy().tobytes() == centres.tobytes() and ptotal.cpu().numpy().tobytes() == total.tobytes()
    assert pcounts.cpu().numpy().tobytes() == counts.tobytes()


# ---- 7. build_codebook ------------------------------------------------------------------------------------------------------------
def test_build_codebook_feeds_the_text_queries(gpu_device):
    from opengaussian_amd import query
    X, dirs, labels, init = wc.codebook_scene()
    k = len(dirs)
    feats = torch.from_numpy(X).to(gpu_device).to(torch.float64)               # what features_from_votes returns
    weight = torch.ones(len(X), dtype=torch.float64, device=gpu_device)
    book = query.build_codebook(feats, k, weights=weight, metric="cosine", iters=5, init=torch.from_numpy(init).to(gpu_device))
    # init row c came from planted cluster c, so leaf c is planted cluster c
    assert book.leaf_ind.dtype == torch.int64 and book.leaf_feat.shape == (k, 64) and book.leaf_feat.dtype == torch.float32
    assert np.array_equal(book.leaf_ind.cpu().numpy(), labels)
    assert np.array_equal(book.occu_count.cpu().numpy(), np.bincount(labels, minlength=k))
    assert bool(book.valid.all()) and float(book.dist.max()) < 1e-2
    text = torch.from_numpy(dirs).to(gpu_device)
    pred = query.classify_points(text, book.leaf_feat, book.occu_count, book.leaf_ind)
    assert np.array_equal(pred.cpu().numpy(), labels + 1)
    sim, selected, count = query.select_leaves_by_text(text, book.leaf_feat, book.occu_count, book.leaf_feat, leaf_num=1, top=3,
                                                       max_dist=0.0)
    assert np.array_equal(selected[:, 0].cpu().numpy(), np.arange(k))
    # unseen rows (weight 0, zero feature) are assigned but counted nowhere; a seeded start gives the same bytes twice
    feats[:10] = 0
    weight[:10] = 0
    a = query.build_codebook(feats, k, weights=weight, iters=4, seed=1)
    b = query.build_codebook(feats, k, weights=weight, iters=4, seed=1)
    assert not bool(a.valid[:10].any()) and bool(a.valid[10:].all()) and int(a.occu_count.sum()) == len(X) - 10
    assert bool((a.leaf_ind[:10] == 0).all()) and bool((a.dist[:10] == 1).all())
    for x, y in zip(a, b):
        assert torch.equal(x, y)
