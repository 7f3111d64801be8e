"""GPU: the neighbour search and the gather-sum (include/ogs_knn.h: ogs_knn_neighbors, ogs_knn_aggregate) through their C ABI
and through opengaussian_amd.knn / query, against tests/knn_neighbors_restatement.py.

Neighbour lists are unique (ordered by (d2, id)), so `idx` and `d2` must be EQUAL to the restatement's, bit for bit.  The
gather-sum is one fp32 fmaf chain of at most 32 links per element: |got - f64| <= 4e-6 * sum_k |w * x| (32 roundings of 2^-24,
doubled).  A diffusion step adds one multiply and one add per side of the blend; with K <= 16 there that is 19 roundings, inside
the same 4e-6 of (1 - rate) * |X| + rate * sum_k |w * x|."""
import os

import numpy as np
import pytest
import torch

from tests import knn_cases as kc
from tests import knn_neighbors_cases as nc
from tests import knn_neighbors_restatement as nr
from tests import knn_restatement as kr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_golden.npz")
SUM_RTOL = 1e-12           # tests/test_37_knn_gpu.py
DIST_RTOL = 1e-6           # the bar of the dist/* goldens there
AGG_BAR = 4e-6
GUARD = 256                # canary elements (or bytes) on either side of a buffer
I_CANARY, F_CANARY, B_CANARY = -77777, -12345.0, 0xA5


def _lib():
    from opengaussian_amd import _lib
    return _lib


def _box():
    return int(_lib().lib().ogs_knn_box_points())


def _guarded(numel, dtype, fill, dev):
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def capi_neighbors(dev, points, K, exclude_self):
    """ogs_knn_neighbors with canaries around idx, d2 and tmp; returns (idx, d2) as NumPy."""
    L = _lib()
    n = len(points)
    pts = torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(dev)
    nbytes = int(L.lib().ogs_knn_neighbors_tmp_bytes(n))
    ibuf, idx = _guarded(n * K, torch.int32, I_CANARY, dev)
    dbuf, d2 = _guarded(n * K, torch.float32, F_CANARY, dev)
    tbuf, tmp = _guarded(nbytes, torch.uint8, B_CANARY, dev)
    assert tmp.data_ptr() % 256 == 0 or nbytes == 0
    L.check(L.lib().ogs_knn_neighbors(n, L.ptr(pts), K, int(exclude_self), L.ptr(idx), L.ptr(d2), L.ptr(tmp), nbytes,
                                      torch.cuda.current_stream().cuda_stream), "ogs_knn_neighbors")
    torch.cuda.synchronize()
    assert _guards_intact(ibuf, I_CANARY) and _guards_intact(dbuf, F_CANARY) and _guards_intact(tbuf, B_CANARY), (n, K)
    return idx.reshape(n, K).cpu().numpy(), d2.reshape(n, K).cpu().numpy()


_REF = {}


def ref_lists(name, points, exclude_self):
    """the restatement at the largest K, once per cloud; the first K columns are the lists of every smaller K"""
    key = (name, bool(exclude_self))
    if key not in _REF:
        _REF[key] = nr.neighbors(points, nc.MAX_K, exclude_self)
    return _REF[key]


def assert_lists(got, want, K, what):
    (gi, gd), (wi, wd) = got, want
    assert np.array_equal(gi, wi[:, :K]), (what, "idx", int((gi != wi[:, :K]).any(1).sum()))
    assert np.array_equal(gd, wd[:, :K]), (what, "d2")


def test_box_size_is_the_one_the_sizes_bracket():
    assert _box() == 64 and int(_lib().lib().ogs_knn_max_k()) == nc.MAX_K


@pytest.mark.parametrize("n", nc.sizes(64))
def test_every_size_every_k_on_the_c_abi_with_canaries(gpu_device, n):
    assert nc.sizes(_box()) == nc.sizes(64)
    pts = kc.cloud(n, 300 + n)
    for ex in (False, True):
        want = ref_lists(("cloud", n), pts, ex)
        for K in nc.KS:
            assert_lists(capi_neighbors(gpu_device, pts, K, ex), want, K, (n, K, ex))


@pytest.mark.parametrize("name", ["offset", "coincident", "collinear", "clusters"])
def test_hard_clouds(gpu_device, name):
    from opengaussian_amd import knn
    pts = nc.clouds(4)[name]
    p = torch.from_numpy(pts).to(gpu_device)
    for ex in (False, True):
        want = ref_lists(name, pts, ex)
        for K in nc.KS:
            idx, d2 = knn.neighbors(p, K, exclude_self=ex)
            assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == (len(pts), K)
            assert_lists((idx.cpu().numpy(), d2.cpu().numpy()), want, K, (name, K, ex))
            if name == "coincident" and not ex:
                assert np.array_equal(idx.cpu().numpy(), np.broadcast_to(np.arange(K), (len(pts), K)))


@pytest.mark.parametrize("K", nc.TIE_K)
def test_exact_ties_go_to_the_smaller_index(gpu_device, K):
    for name, pts in kc.tie_clouds(K).items():
        for ex in (False, True):
            want = nr.neighbors(pts, K, ex)
            assert_lists(capi_neighbors(gpu_device, pts, K, ex), want, K, (name, K, ex))


def test_twenty_thousand_rows_memory_determinism_and_order_independence(gpu_device):
    from opengaussian_amd import knn
    n, K = 20000, 16
    pts = kc.cloud(n, 21)
    p = torch.from_numpy(pts).to(gpu_device)
    knn.neighbors(p[:100], K)                                   # load the library outside the measured window
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    idx, d2 = knn.neighbors(p, K)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"neighbors n={n} K={K}: peak {peak} bytes = {peak / n:.1f} per point")
    assert peak < (8 * K + 64) * n
    rows = np.random.default_rng(3).choice(n, 256, replace=False)
    wi, wd = nr.neighbors(pts, K, True, rows=rows)
    assert np.array_equal(idx.cpu().numpy()[rows], wi) and np.array_equal(d2.cpu().numpy()[rows], wd)
    idx2, d22 = knn.neighbors(p, K)
    assert torch.equal(idx, idx2) and torch.equal(d2, d22)      # same bytes
    perm = torch.from_numpy(np.random.default_rng(4).permutation(n)).to(gpu_device)
    idx3, d23 = knn.neighbors(p[perm], K)
    assert torch.equal(d23, d2[perm])                           # the same rows of distances, whatever the input order
    # the clustered cloud at a size where most boxes are pruned
    cl, _ = nc.two_clusters(n, seed=47, outliers=40)
    rows = np.random.default_rng(5).choice(n, 256, replace=False)
    for ex, K2 in ((False, 4), (True, 32)):
        gi, gd = knn.neighbors(torch.from_numpy(cl).to(gpu_device), K2, exclude_self=ex)
        wi, wd = nr.neighbors(cl, K2, ex, rows=rows)
        assert np.array_equal(gi.cpu().numpy()[rows], wi) and np.array_equal(gd.cpu().numpy()[rows], wd)


@pytest.mark.parametrize("K", [4, 16])
def test_agrees_with_the_threshold_kernel(gpu_device, K):
    """d2[:, K - 1] is group_ksum's K-th value bit for bit, the fp64 row sum its sum1 (another summation order)."""
    from opengaussian_amd import knn
    for pts in (kc.cloud(4097, 31), kc.tie_clouds(K)["lattice"], nc.two_clusters()[0]):
        p = torch.from_numpy(pts).to(gpu_device)
        kth, s1, _ = knn.group_ksum(p, None, 1, K)
        _, d2 = knn.neighbors(p, K, exclude_self=False)
        assert torch.equal(d2[:, K - 1], kth)
        got = d2.to(torch.float64).sum(dim=1)
        assert bool(((got - s1).abs() <= SUM_RTOL * s1.abs()).all())


def test_bad_arguments_are_errors_and_empty_input_is_fine(gpu_device):
    L = _lib()
    from opengaussian_amd import knn
    n = 100
    pts = torch.rand(n, 3, device=gpu_device)
    nbytes = int(L.lib().ogs_knn_neighbors_tmp_bytes(n))
    assert nbytes > 0
    idx = torch.full((n, 4), I_CANARY, dtype=torch.int32, device=gpu_device)
    d2 = torch.full((n, 4), F_CANARY, dtype=torch.float32, device=gpu_device)
    tmp = torch.empty(nbytes, dtype=torch.uint8, device=gpu_device)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda n_, K, nb: L.lib().ogs_knn_neighbors(n_, L.ptr(pts), K, 1, L.ptr(idx), L.ptr(d2), L.ptr(tmp), nb, s)
    assert call(n, 4, nbytes - 1) == -1 and b"tmp" in L.lib().ogs_last_error()
    assert call(n, 0, nbytes) == -1 and call(n, nc.MAX_K + 1, nbytes) == -1 and call(-1, 4, nbytes) == -1
    assert L.lib().ogs_knn_neighbors(n, None, 4, 1, L.ptr(idx), L.ptr(d2), L.ptr(tmp), nbytes, s) == -1
    assert call(0, 4, 0) == 0
    torch.cuda.synchronize()
    assert bool((idx == I_CANARY).all()) and bool((d2 == F_CANARY).all())       # none of these calls wrote anything
    with pytest.raises(L.OgsError):
        knn.neighbors(pts, 33)
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn.neighbors(torch.rand(10, 3), 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn.aggregate(torch.rand(10, 3), torch.zeros(10, 2, dtype=torch.int32), torch.rand(10, 2))
    e_idx, e_d2 = knn.neighbors(torch.zeros(0, 3, device=gpu_device), 4)
    assert e_idx.shape == (0, 4) and e_d2.shape == (0, 4)
    assert L.lib().ogs_knn_aggregate(5, 2, 5, 0, None, None, None, None, s) == -1
    assert L.lib().ogs_knn_aggregate(0, 2, 5, 3, None, None, None, None, s) == 0


def test_dist_cuda2_by_boxes(gpu_device):
    from opengaussian_amd import knn
    gold = np.load(GOLD)
    for name in gold["dist_cases"]:
        got = knn.distCUDA2(torch.from_numpy(gold[f"dist/{name}/points"]).to(gpu_device), route="boxes")
        want = gold[f"dist/{name}/out"].astype(np.float64)
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert np.all(np.abs(got.cpu().numpy() - want) <= DIST_RTOL * np.abs(want)), name
    clouds = dict(nc.clouds(4), cloud=kc.cloud(4097, 33), tiny=kc.cloud(3, 1), one=kc.cloud(1, 1))
    for name, pts in clouds.items():
        p = torch.from_numpy(pts).to(gpu_device)
        boxes = knn.distCUDA2(p, route="boxes").cpu().numpy().astype(np.float64)
        brute = knn.distCUDA2(p, route="brute").cpu().numpy().astype(np.float64)
        want = kr.dist_cuda2(pts).astype(np.float64)
        assert np.all(np.abs(boxes - want) <= DIST_RTOL * np.abs(want)), name
        assert np.all(np.abs(boxes - brute) <= DIST_RTOL * np.abs(brute)), name
        auto = knn.distCUDA2(p).cpu().numpy().astype(np.float64)
        assert np.all(np.abs(auto - want) <= DIST_RTOL * np.abs(want)), name
    with pytest.raises(ValueError):
        knn.distCUDA2(p, route="tree")


# ---- the gather-sum -----------------------------------------------------------------------------------------------------------
def capi_aggregate(dev, X, idx, w, misalign=False):
    """ogs_knn_aggregate with canaries around out; misalign: X and out start 4 bytes past a 16-byte boundary."""
    L = _lib()
    R, D = X.shape
    n, K = idx.shape
    off = 1 if misalign else 0
    xbuf = torch.zeros(R * D + 4, dtype=torch.float32, device=dev)
    xv = xbuf[off:off + R * D]
    xv.copy_(torch.from_numpy(np.ascontiguousarray(X, np.float32)).reshape(-1))
    obuf = torch.full((n * D + 2 * GUARD + 4,), F_CANARY, dtype=torch.float32, device=dev)
    out = obuf[GUARD + off:GUARD + off + n * D]
    assert (xv.data_ptr() % 16 == 4) == misalign and (out.data_ptr() % 16 == 4) == misalign
    it = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dev)
    wt = torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(dev)
    L.check(L.lib().ogs_knn_aggregate(n, K, R, D, L.ptr(it), L.ptr(wt), L.ptr(xv), L.ptr(out),
                                      torch.cuda.current_stream().cuda_stream), "ogs_knn_aggregate")
    torch.cuda.synchronize()
    assert bool((obuf[:GUARD + off] == F_CANARY).all()) and bool((obuf[GUARD + off + n * D:] == F_CANARY).all())
    return out.reshape(n, D).cpu().numpy()


@pytest.mark.parametrize("D", [1, 3, 4, 5, 6, 64, 65, 257])
def test_aggregate(gpu_device, D):
    rng = np.random.default_rng(500 + D)
    n, R = 1031, 977                                            # more than one workgroup at every D; R != n
    X = rng.standard_normal((R, D)).astype(np.float32)
    for K in (1, 16, 32):
        idx = rng.integers(0, R, (n, K)).astype(np.int32)
        w = rng.standard_normal((n, K)).astype(np.float32)
        bad = rng.random((n, K)) < 0.2
        idx[bad] = rng.choice(np.array([-1, R, np.iinfo(np.int32).min, np.iinfo(np.int32).max], np.int64), bad.sum()).astype(np.int32)
        idx[5], idx[6, :] = -1, R                               # rows with no slot at all
        w[(idx < 0) | (idx >= R)] = np.nan                      # a skipped slot's weight is never read as a value
        want, scale = nr.aggregate(X, idx, w)
        for misalign in (False, True):
            got = capi_aggregate(gpu_device, X, idx, w, misalign)
            assert np.isfinite(got).all() and not got[5].any() and not got[6].any()
            assert np.all(np.abs(got - want) <= AGG_BAR * scale), (D, K, misalign, float(np.abs(got - want).max()))
            assert np.array_equal(got, capi_aggregate(gpu_device, X, idx, w, misalign))        # same bytes
        assert np.array_equal(capi_aggregate(gpu_device, X, idx, w, False), capi_aggregate(gpu_device, X, idx, w, True))


def test_aggregate_through_knn_py(gpu_device):
    from opengaussian_amd import knn
    rng = np.random.default_rng(9)
    X = torch.from_numpy(rng.standard_normal((400, 6)).astype(np.float32)).to(gpu_device).requires_grad_(True)
    idx = torch.from_numpy(rng.integers(-1, 400, (400, 8)).astype(np.int32)).to(gpu_device)
    w = torch.from_numpy(rng.random((400, 8)).astype(np.float32)).to(gpu_device)
    out = knn.aggregate(X, idx, w)
    assert out.dtype == torch.float32 and out.shape == (400, 6) and not out.requires_grad      # forward only
    want, scale = nr.aggregate(X.detach().cpu().numpy(), idx.cpu().numpy(), w.cpu().numpy())
    assert np.all(np.abs(out.cpu().numpy() - want) <= AGG_BAR * scale)
    torch_route = (w[..., None] * X.detach()[idx.clamp_min(0).long()] * (idx >= 0)[..., None]).sum(1)
    assert torch.allclose(out, torch_route, rtol=0, atol=1e-5)


# ---- weights and diffusion ------------------------------------------------------------------------------------------------------
def test_neighbor_weights(gpu_device):
    from opengaussian_amd import knn, query
    pts = kc.cloud(500, 51)
    p = torch.from_numpy(pts).to(gpu_device)
    idx, d2 = knn.neighbors(p, 8)
    valid = torch.from_numpy(np.random.default_rng(1).random(500) > 0.4).to(gpu_device)
    valid[idx[7].long()] = False
    for kw in (dict(), dict(valid=valid), dict(bandwidth=0.003)):
        w = query.neighbor_weights(d2, idx, **kw)
        np_kw = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in kw.items()}
        want = nr.neighbor_weights(d2.cpu().numpy(), idx.cpu().numpy(), **np_kw)
        assert w.dtype == torch.float32 and np.all(np.abs(w.cpu().numpy() - want) <= 1e-6)
    assert not w.isnan().any() and not query.neighbor_weights(d2, idx, valid=valid)[7].any()
    i1, dd1 = knn.neighbors(p[:3], 8)                             # empty slots weigh nothing
    w1 = query.neighbor_weights(dd1, i1)
    assert bool((w1[:, 2:] == 0).all()) and torch.allclose(w1.sum(1), torch.ones(3, device=gpu_device))


def test_diffuse_features(gpu_device):
    from opengaussian_amd import knn, query
    rng = np.random.default_rng(61)
    pts, lab = nc.two_clusters()
    n = len(pts)
    p = torch.from_numpy(pts).to(gpu_device)
    idx, d2 = knn.neighbors(p, 16)
    # general: random features, some rows fixed, some rows without a neighbour, rate < 1, step by step
    w = query.neighbor_weights(d2, idx)
    w[11] = 0
    w[12] = 0
    fixed = torch.from_numpy(rng.random(n) > 0.7).to(gpu_device)
    fixed[11] = False
    X0 = torch.from_numpy(rng.standard_normal((n, 5)).astype(np.float32)).to(gpu_device)
    assert torch.equal(query.diffuse_features(X0, idx, w, steps=0), X0)
    for rate in (1.0, 0.4):
        X = X0
        for step in range(3):
            new = query.diffuse_features(X, idx, w, steps=1, rate=rate, fixed=fixed)
            want, scale = nr.diffuse_step(X.cpu().numpy(), idx.cpu().numpy(), w.cpu().numpy(), rate, fixed.cpu().numpy())
            assert new.dtype == torch.float32
            assert np.all(np.abs(new.cpu().numpy() - want) <= AGG_BAR * scale), (rate, step)
            assert torch.equal(new[fixed], X[fixed]) and torch.equal(new[11], X[11]) and torch.equal(new[12], X[12])
            X = new
        assert torch.equal(query.diffuse_features(X0, idx, w, steps=3, rate=rate, fixed=fixed), X)
    # fill: one-hot cluster features, a third of the rows zeroed and invalid; every such row ends in its own cluster
    hot = np.zeros((n, 2), np.float32)
    hot[lab == 0, 0] = 1
    hot[lab == 1, 1] = 1
    lost = (rng.random(n) < 1 / 3) & (lab >= 0)
    hot[lost] = 0
    ok = torch.from_numpy(~lost & (lab >= 0)).to(gpu_device)
    assert lost.sum() > n // 4
    wf = query.neighbor_weights(d2, idx, valid=ok)
    F0 = torch.from_numpy(hot).to(gpu_device)
    filled = query.diffuse_features(F0, idx, wf, steps=1, fixed=ok)
    assert torch.equal(filled[ok], F0[ok])
    got = filled.cpu().numpy()
    assert np.array_equal(got[lost].argmax(1), lab[lost]) and np.all(got[lost].max(1) > 0.99)
