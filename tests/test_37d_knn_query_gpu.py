"""GPU: the search between two point sets (include/ogs_knn.h: ogs_knn_index_build, ogs_knn_query) through its C ABI and through
opengaussian_amd.knn / query, against tests/knn_query_restatement.py.

The lists are unique (ordered by (d2, reference row)), so `idx` and `d2` must be EQUAL to the restatement's, bit for bit: there is
no tolerance to choose.  transfer_features is one fp32 fmaf chain of at most 32 links per element over fp32-rounded weights:
|got - f64| <= AGG_BAR * sum_k |w * x|, the bar and the scale of tests/test_37b_knn_neighbors_gpu.py::test_aggregate."""
import numpy as np
import pytest
import torch

from tests import knn_cases as kc
from tests import knn_query_cases as qc
from tests import knn_query_restatement as qr

pytestmark = pytest.mark.gpu

AGG_BAR = 4e-6             # tests/test_37b_knn_neighbors_gpu.py
GUARD = 256                # canary elements (or bytes) on either side of a buffer
I_CANARY, F_CANARY, B_CANARY = -77777, -12345.0, 0xA5


def _lib():
    from opengaussian_amd import _lib
    return _lib


def _guarded(numel, dtype, fill, dev):
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def capi_build(dev, points):
    """ogs_knn_index_build with canaries around the index and tmp; returns (guarded buffer, index view, bytes)."""
    L = _lib()
    n = len(points)
    pts = torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(dev)
    ibytes, tbytes = int(L.lib().ogs_knn_index_bytes(n)), int(L.lib().ogs_knn_index_build_tmp_bytes(n))
    assert (ibytes > 0 and tbytes > 0) or n == 0
    xbuf, index = _guarded(ibytes, torch.uint8, B_CANARY, dev)
    tbuf, tmp = _guarded(tbytes, torch.uint8, B_CANARY, dev)
    L.check(L.lib().ogs_knn_index_build(n, L.ptr(pts), L.ptr(index), ibytes, L.ptr(tmp), tbytes,
                                        torch.cuda.current_stream().cuda_stream), "ogs_knn_index_build")
    torch.cuda.synchronize()
    assert _guards_intact(xbuf, B_CANARY) and _guards_intact(tbuf, B_CANARY), n
    pts.fill_(float("nan"))                                     # the index is a copy
    return xbuf, index


def capi_query(dev, n, xbuf, index, queries, K):
    """ogs_knn_query with canaries around idx, d2, tmp and (still) the index; returns (idx, d2) as NumPy."""
    L = _lib()
    m = len(queries)
    q = torch.from_numpy(np.ascontiguousarray(queries, np.float32)).to(dev)
    nbytes = int(L.lib().ogs_knn_query_tmp_bytes(n, m))
    ibuf, idx = _guarded(m * K, torch.int32, I_CANARY, dev)
    dbuf, d2 = _guarded(m * K, torch.float32, F_CANARY, dev)
    tbuf, tmp = _guarded(nbytes, torch.uint8, B_CANARY, dev)
    L.check(L.lib().ogs_knn_query(n, L.ptr(index), m, L.ptr(q), K, L.ptr(idx), L.ptr(d2), L.ptr(tmp), nbytes,
                                  torch.cuda.current_stream().cuda_stream), "ogs_knn_query")
    torch.cuda.synchronize()
    assert _guards_intact(ibuf, I_CANARY) and _guards_intact(dbuf, F_CANARY) and _guards_intact(tbuf, B_CANARY), (n, m, K)
    assert _guards_intact(xbuf, B_CANARY), (n, m, K)
    return idx.reshape(m, K).cpu().numpy(), d2.reshape(m, K).cpu().numpy()


def assert_lists(got, want, K, what):
    (gi, gd), (wi, wd) = got, want
    assert np.array_equal(gi, wi[:, :K]), (what, "idx", int((gi != wi[:, :K]).any(1).sum()))
    assert np.array_equal(gd, wd[:, :K]), (what, "d2")


def py_query(dev, ref, q, K):
    from opengaussian_amd import knn
    idx, d2 = knn.query(torch.from_numpy(ref).to(dev), torch.from_numpy(q).to(dev), K)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == (len(q), K) and d2.shape == (len(q), K)
    return idx.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize("n,m", qc.SIZE_PAIRS)
def test_every_size_pair_every_k_on_the_c_abi_with_canaries(gpu_device, n, m):
    assert int(_lib().lib().ogs_knn_box_points()) == 64 and int(_lib().lib().ogs_knn_max_k()) == qc.MAX_K
    ref, q = qc.size_pair(n, m)
    want = qr.query(ref, q, qc.MAX_K)                           # the first K columns are the lists of every smaller K
    xbuf, index = capi_build(gpu_device, ref)
    for K in qc.KS:
        assert_lists(capi_query(gpu_device, n, xbuf, index, q, K), want, K, (n, m, K))


@pytest.mark.parametrize("name", ["same", "outside", "straddle", "between", "coincident_ref", "coincident_queries", "collinear"])
def test_hard_sets(gpu_device, name):
    from opengaussian_amd import knn
    ref, q = qc.hard()[name]
    want = qr.query(ref, q, qc.MAX_K)
    for K in qc.KS:
        got = py_query(gpu_device, ref, q, K)
        assert_lists(got, want, K, (name, K))
        if name == "coincident_ref":
            assert np.array_equal(got[0], np.broadcast_to(np.arange(K), (len(q), K)))
        if name == "same":                                      # byte-equal to the one-set search with the row itself listed
            ni, nd = knn.neighbors(torch.from_numpy(ref).to(gpu_device), K, exclude_self=False)
            assert np.array_equal(got[0], ni.cpu().numpy()) and np.array_equal(got[1], nd.cpu().numpy())


@pytest.mark.parametrize("K", qc.TIE_K)
def test_exact_ties_go_to_the_smaller_reference_row(gpu_device, K):
    for name, (ref, q) in qc.tie_sets(K).items():
        assert_lists(py_query(gpu_device, ref, q, K), qr.query(ref, q, K), K, (name, K))


def test_short_lists_are_padded(gpu_device):
    for name, (ref, q, K) in qc.short().items():
        gi, gd = py_query(gpu_device, ref, q, K)
        assert_lists((gi, gd), qr.query(ref, q, K), K, name)
        assert (gi[:, len(ref):] == -1).all() and np.isposinf(gd[:, len(ref):]).all()


def test_one_index_many_queries_and_the_index_is_a_copy(gpu_device):
    from opengaussian_amd import knn
    ref = torch.from_numpy(kc.cloud(3000, 41)).to(gpu_device)
    qa = torch.from_numpy(kc.cloud(700, 42)).to(gpu_device)
    qb = torch.from_numpy(kc.cloud(1300, 43) * 2 - 0.5).to(gpu_device)
    one_a, one_b = knn.query(ref, qa, 8), knn.query(ref, qb, 5)
    points = ref.clone()
    index = knn.Index(points)
    assert index.n == 3000 and index.device == ref.device
    for _ in range(2):
        ia, da = index.query(qa, 8)
        ib, db = index.query(qb, 5)
        assert torch.equal(ia, one_a[0]) and torch.equal(da, one_a[1]) and torch.equal(ib, one_b[0]) and torch.equal(db, one_b[1])
        points.copy_(torch.rand_like(points) * 9)              # the next round searches the index, not this tensor
        torch.cuda.synchronize()


@pytest.mark.parametrize("K", [1, 16])
def test_medium_size_memory_determinism_and_order_independence(gpu_device, K):
    from opengaussian_amd import knn
    ref_np, q_np = qc.medium()
    n, m = len(ref_np), len(q_np)
    ref, q = torch.from_numpy(ref_np).to(gpu_device), torch.from_numpy(q_np).to(gpu_device)
    knn.query(ref[:100], q[:100], K)                            # load the library outside the measured window
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    idx, d2 = knn.query(ref, q, K)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"query n={n} m={m} K={K}: peak {peak} bytes = {peak / (n + m):.1f} per point of either set")
    assert peak < (8 * K + 64) * (n + m)
    rows = np.random.default_rng(3).choice(m, 256, replace=False)
    wi, wd = qr.query(ref_np, q_np, K, rows=rows)
    assert np.array_equal(idx.cpu().numpy()[rows], wi) and np.array_equal(d2.cpu().numpy()[rows], wd)
    idx2, d22 = knn.query(ref, q, K)
    assert torch.equal(idx, idx2) and torch.equal(d2, d22)      # same bytes
    perm = torch.from_numpy(np.random.default_rng(4).permutation(m)).to(gpu_device)
    idx3, d23 = knn.query(ref, q[perm], K)
    assert torch.equal(idx3, idx[perm]) and torch.equal(d23, d2[perm])
    rperm = torch.from_numpy(np.random.default_rng(5).permutation(n)).to(gpu_device)
    idx4, d24 = knn.query(ref[rperm], q, K)
    assert torch.equal(d24, d2)                                 # the same distances, whatever the reference order
    _, wd2 = qr.query(ref_np, q_np, K + 1, rows=rows)
    r = torch.from_numpy(rows[(wd2[:, 1:] != wd2[:, :-1]).all(1)]).to(gpu_device)
    assert len(r) > 200 and torch.equal(rperm[idx4[r].long()], idx[r].long())    # and the same rows under new numbers, where no tie decides


def test_bad_arguments_are_errors_and_empty_input_is_fine(gpu_device):
    L = _lib()
    from opengaussian_amd import knn
    lib = L.lib()
    n, m, K = 100, 70, 4
    pts, q = torch.rand(n, 3, device=gpu_device), torch.rand(m, 3, device=gpu_device)
    ibytes, bbytes, qbytes = int(lib.ogs_knn_index_bytes(n)), int(lib.ogs_knn_index_build_tmp_bytes(n)), int(lib.ogs_knn_query_tmp_bytes(n, m))
    assert ibytes > 0 and bbytes > 0 and qbytes > 0
    index = torch.empty(ibytes, dtype=torch.uint8, device=gpu_device)
    btmp = torch.empty(bbytes, dtype=torch.uint8, device=gpu_device)
    qtmp = torch.empty(qbytes, dtype=torch.uint8, device=gpu_device)
    idx = torch.full((m, K), I_CANARY, dtype=torch.int32, device=gpu_device)
    d2 = torch.full((m, K), F_CANARY, dtype=torch.float32, device=gpu_device)
    s = torch.cuda.current_stream().cuda_stream
    P = L.ptr
    build = lambda n_, p, ix, ib, t, tb: lib.ogs_knn_index_build(n_, p, ix, ib, t, tb, s)
    assert build(n, P(pts), P(index), ibytes - 1, P(btmp), bbytes) == -1 and b"index" in lib.ogs_last_error()
    assert build(n, P(pts), P(index), ibytes, P(btmp), bbytes - 1) == -1 and b"tmp" in lib.ogs_last_error()
    assert build(-1, P(pts), P(index), ibytes, P(btmp), bbytes) == -1 and build(2 ** 31, P(pts), P(index), ibytes, P(btmp), bbytes) == -1
    for args in ((None, P(index), P(btmp)), (P(pts), None, P(btmp)), (P(pts), P(index), None)):
        assert build(n, args[0], args[1], ibytes, args[2], bbytes) == -1
    assert build(0, None, None, 0, None, 0) == 0
    assert build(n, P(pts), P(index), ibytes, P(btmp), bbytes) == 0
    ask = lambda n_, ix, m_, qq, K_, i_, d_, t, tb: lib.ogs_knn_query(n_, ix, m_, qq, K_, i_, d_, t, tb, s)
    good = (n, P(index), m, P(q), K, P(idx), P(d2), P(qtmp), qbytes)
    swap = lambda pos, v: good[:pos] + (v,) + good[pos + 1:]
    assert ask(*swap(8, qbytes - 1)) == -1 and b"tmp" in lib.ogs_last_error()
    assert ask(*swap(4, 0)) == -1 and ask(*swap(4, qc.MAX_K + 1)) == -1 and ask(*swap(0, -1)) == -1 and ask(*swap(2, -1)) == -1
    assert ask(*swap(4, 32)[:2], 2 ** 26, *swap(4, 32)[3:]) == -1 and b"2^31" in lib.ogs_last_error()      # m * K = 2^31, by sizes alone
    for pos in (1, 3, 5, 6, 7):
        assert ask(*swap(pos, None)) == -1, pos
    assert ask(*swap(2, 0)) == 0                                # m = 0: nothing to do
    torch.cuda.synchronize()
    assert bool((idx == I_CANARY).all()) and bool((d2 == F_CANARY).all())       # none of these calls wrote anything
    assert ask(0, None, m, None, K, P(idx), P(d2), None, 0) == 0                # n = 0: every list is empty
    torch.cuda.synchronize()
    assert bool((idx == -1).all()) and bool(torch.isposinf(d2).all())
    assert ask(*good) == 0
    torch.cuda.synchronize()
    assert_lists((idx.cpu().numpy(), d2.cpu().numpy()), qr.query(pts.cpu().numpy(), q.cpu().numpy(), K), K, "after the errors")
    with pytest.raises(L.OgsError):
        knn.query(pts, q, 33)
    with pytest.raises(L.OgsError):
        knn.Index(pts).query(q, 0)
    with pytest.raises(ValueError):
        knn.query(pts, q[:, :2], 4)
    with pytest.raises(ValueError):
        knn.Index(pts[:, :2])
    e_idx, e_d2 = knn.query(pts, torch.zeros(0, 3, device=gpu_device), 4)
    assert e_idx.shape == (0, 4) and e_d2.shape == (0, 4)
    z_idx, z_d2 = knn.query(torch.zeros(0, 3, device=gpu_device), q, 3)
    assert bool((z_idx == -1).all()) and bool(torch.isposinf(z_d2).all()) and z_idx.shape == (m, 3)


def test_transfer_labels(gpu_device):
    from opengaussian_amd import knn, query
    ref, q, cluster = qc.between()
    rng = np.random.default_rng(81)
    lab = np.where(cluster >= 0, cluster * 3 + rng.integers(0, 3, len(ref)), 7)        # labels 0..5 in the clusters, 7 outside
    L_ = 7                                                                           # label 7 lies outside [0, num_labels)
    ignore = rng.random(len(ref)) < 0.3
    dst = np.concatenate([q, ref[::7] + np.float32(0.01)]).astype(np.float32)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(gpu_device)
    index = knn.Index(t(ref))
    for k in (1, 5):
        for kw in (dict(), dict(max_dist=1.0), dict(ignore=ignore), dict(max_dist=30.0, ignore=ignore)):
            want, margin = qr.transfer_labels(ref, lab, dst, k, L_, **kw)
            tkw = {key: (t(v) if isinstance(v, np.ndarray) else v) for key, v in kw.items()}
            got = query.transfer_labels(t(ref), t(lab), t(dst), k=k, num_labels=L_, index=index if k == 5 else None, **tkw)
            assert got.dtype == torch.int64 and got.shape == (len(dst),)
            sure = margin > 1e-5                                                     # fp32 weights cannot order closer sums
            assert sure.mean() > 0.95 and np.array_equal(got.cpu().numpy()[sure], want[sure]), (k, kw)
            if "max_dist" in kw and kw["max_dist"] == 1.0:
                assert (want[:200] == -1).all() and bool((got[:200] == -1).all())      # the midpoint queries: nothing within 1
            if k == 1 and not kw:
                assert bool((got[200:200 + (cluster < 0).sum()] == -1).all())          # an outlier's own position: label 7 does not count
    assert (qr.transfer_labels(ref, lab, dst, 5, L_, ignore=ignore)[0] == -1).sum() > 0
    # an exact tie goes to the lower label, whichever row carries it
    src = np.array([[1, 0, 0], [-1, 0, 0], [0, 50, 0], [0, 50, 2]], np.float32)
    for labels, low in (([3, 1, 2, 0], 1), ([1, 3, 2, 0], 1)):
        got = query.transfer_labels(t(src), t(np.array(labels)), t(np.array([[0, 0, 0], [0, 50, 1]], np.float32)), k=2)
        assert got.cpu().tolist() == [low, 0]
    # chunked over rows: a budget of 64 table rows at a time gives the same labels
    whole = query.transfer_labels(t(ref), t(lab), t(dst[:300]), k=5, num_labels=L_)
    budget, query.LABEL_TABLE_BYTES = query.LABEL_TABLE_BYTES, 4 * L_ * 64
    try:
        assert torch.equal(query.transfer_labels(t(ref), t(lab), t(dst[:300]), k=5, num_labels=L_), whole)
    finally:
        query.LABEL_TABLE_BYTES = budget


@pytest.mark.parametrize("D", [6, 64])
def test_transfer_features_and_its_gradient(gpu_device, D):
    from opengaussian_amd import query
    ref, q, _ = qc.between()
    rng = np.random.default_rng(90 + D)
    dst = np.concatenate([q, ref[::5] + np.float32(0.02)]).astype(np.float32)
    X = rng.standard_normal((len(ref), D)).astype(np.float32)
    valid = rng.random(len(ref)) > 0.3
    t = lambda a: torch.from_numpy(np.asarray(a)).to(gpu_device)
    for kw in (dict(k=8), dict(k=8, max_dist=1.0, valid=valid), dict(k=3, bandwidth=0.01, valid=valid)):
        want = qr.transfer_features(ref, X, dst, **kw)
        tkw = {key: (t(v) if isinstance(v, np.ndarray) else v) for key, v in kw.items()}
        feat, weight = query.transfer_features(t(ref), t(X), t(dst), **tkw)
        assert feat.dtype == torch.float32 and feat.shape == (len(dst), D) and weight.shape == (len(dst),) and not feat.requires_grad
        err = np.abs(feat.cpu().numpy() - want["feat"])
        assert np.all(err <= AGG_BAR * want["scale"]), (kw, float(err.max()))
        assert np.all(np.abs(weight.cpu().numpy() - want["weight"]) <= 1e-6 * np.maximum(want["weight"], 1e-30))
        empty = want["weight"].astype(np.float32) == 0
        assert np.array_equal(weight.cpu().numpy() == 0, empty) and not feat.cpu().numpy()[empty].any()
        if "max_dist" in kw:
            assert empty[:200].all() and not empty.all()
        # the gradient with respect to the features, against torch autograd of the composition on the same table
        Xg = t(X).requires_grad_(True)
        out, _ = query.transfer_features(t(ref), Xg, t(dst), **tkw)
        assert torch.equal(out.detach(), feat)
        G = t(rng.standard_normal((len(dst), D)).astype(np.float32))
        out.backward(G)
        idx, w = t(want["idx"]).long().clamp_min(0), t(want["w"])
        Xr = t(X).double().requires_grad_(True)
        ((w[..., None] * Xr[idx]).sum(1) * G.double()).sum().backward()
        scale = torch.zeros_like(Xr).index_put_((idx.reshape(-1),), (w[..., None] * G.double().abs()[:, None, :]).reshape(-1, D),
                                                accumulate=True)
        gerr = (Xg.grad.double() - Xr.grad).abs()
        assert bool((gerr <= AGG_BAR * scale).all()), (kw, float((gerr / scale.clamp_min(1e-300)).max()))
