"""GPU: the kNN graph backwards (include/ogs_knn.h: ogs_knn_transpose, ogs_knn_aggregate_t, ogs_knn_edge_dots,
ogs_knn_smoothness_fwd / _bwd) through the C ABI and through opengaussian_amd.knn / query, against
tests/knn_graph_restatement.py and float64 torch autograd on the CPU.

Reverse lists are unique: `begin` and `slots[:begin[R]]` must be EQUAL to the restatement's.  The sums are held to first-order
rounding bounds that hold for ANY summation order (U = 2^-24, inputs exact fp32):
  aggregate_t   |got - f64| <= (m + 2) U sum |w g|, m = the row's in-degree (m fmaf roundings and the partial adds)
  edge_dots     |got - f64| <= (D + 2) U sum_c |g x|
  row energy    |got - f64| <= (K D + 8) U e_row (w >= 0: every term is non-negative)
  gF            |got - f64| <= (m + 6) U sum |2 scale w dF|, m = valid out-slots + in-degree: per term one rounding of the
                difference and one of the fmaf, the adds of any order, then the product with 2 * scale (one rounding) of a scale
                that is itself an fp32 rounding of 1 / count (one more); two spare for the second-order terms at m ~ 800
  gw            |got - f64| <= (D + 6) U scale d2: per column the difference (counted twice: it is squared), D adds, then the
                scale as above
  autograd through several steps (diffuse): every path product of the gradient passes, per step, an aggregate_t or aggregate
                (at most max(K, in-degree) + 2 roundings), the blend (3) and the sum of the two uses of a tensor (1), and for w
                one edge-dot reduction (D + 2); so with S = the same gradient computed from |X|, |w|, |G| (the sum of the
                absolute path products) the bar is steps * (max(K, max in-degree) + 6) + D + 2 roundings of S."""
import numpy as np
import pytest
import torch

from tests import knn_cases as kc
from tests import knn_graph_cases as gc
from tests import knn_graph_restatement as gr
from tests import knn_neighbors_restatement as nr

pytestmark = pytest.mark.gpu

U = gr.U
GUARD = 256
I_CANARY, F_CANARY, B_CANARY = -77777, -12345.0, 0xA5


def _lib():
    from opengaussian_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _guarded(numel, dtype, fill, dev, off=0):
    """a buffer with canaries on both sides; off: elements past the aligned start (fp32: 1 = 4 bytes off a 16-byte boundary)"""
    buf = torch.full((numel + 2 * GUARD + 4,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD + off:GUARD + off + numel]


def _intact(buf, view, fill):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == fill).all()) and bool((buf[lo + view.numel():] == fill).all())


def _floats(a, dev, off=0):
    """a's values on the device, aligned to 16 bytes or 4 bytes past that"""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=dev)
    v = buf[off:off + a.size]
    v.copy_(torch.from_numpy(a.reshape(-1)))
    assert v.data_ptr() % 16 == 4 * off
    return v


# ---- reverse lists ------------------------------------------------------------------------------------------------------------
def capi_transpose(dev, idx, R):
    """ogs_knn_transpose with canaries around begin, slots and tmp; (begin, slots as written) as NumPy."""
    L = _lib()
    n, K = idx.shape
    it = _dev(idx, dev, torch.int32)
    nbytes = int(L.lib().ogs_knn_transpose_tmp_bytes(n, K, R))
    bbuf, begin = _guarded(R + 1, torch.int32, I_CANARY, dev)
    sbuf, slots = _guarded(n * K, torch.int32, I_CANARY, dev)
    tbuf, tmp = _guarded(nbytes, torch.uint8, B_CANARY, dev)
    L.check(L.lib().ogs_knn_transpose(n, K, R, L.ptr(it), L.ptr(begin), L.ptr(slots), L.ptr(tmp), nbytes, _stream()),
            "ogs_knn_transpose")
    torch.cuda.synchronize()
    assert _intact(bbuf, begin, I_CANARY) and _intact(sbuf, slots, I_CANARY) and _intact(tbuf, tmp, B_CANARY), (n, K, R)
    return begin.cpu().numpy(), slots.cpu().numpy()


def assert_lists(dev, idx, R, what):
    want_b, want_s = gr.reverse_lists(idx, R)
    got_b, got_s = capi_transpose(dev, idx, R)
    assert np.array_equal(got_b, want_b), (what, "begin")
    assert np.array_equal(got_s[:want_b[R]], want_s), (what, "slots")
    again_b, again_s = capi_transpose(dev, idx, R)
    assert np.array_equal(again_b, got_b) and np.array_equal(again_s[:want_b[R]], got_s[:want_b[R]]), (what, "two runs")


def test_chunk_is_the_one_the_cases_bracket():
    assert int(_lib().lib().ogs_knn_transpose_chunk()) == gc.CHUNK


@pytest.mark.parametrize("n", gc.TABLE_N)
def test_transpose_of_neighbour_tables(gpu_device, n):
    from opengaussian_amd import knn
    pts = torch.from_numpy(kc.cloud(n, 300 + n)).to(gpu_device)
    for K in gc.TABLE_K:
        idx = knn.neighbors(pts, K)[0].cpu().numpy()
        assert (idx == -1).any() == (n <= K)
        assert_lists(gpu_device, idx, n, (n, K))
        begin, slots = knn.reverse_edges(torch.from_numpy(idx).to(gpu_device))              # the public route, R = n
        wb, ws = gr.reverse_lists(idx, n)
        assert begin.dtype == torch.int32 and slots.dtype == torch.int32 and slots.shape == (n * K,)
        assert np.array_equal(begin.cpu().numpy(), wb) and np.array_equal(slots.cpu().numpy()[:wb[n]], ws)


@pytest.mark.parametrize("n,K", [(1, 1), (5, 3), (65, 4), (257, 16)])
def test_transpose_row_counts_and_invalid_values(gpu_device, n, K):
    for R in (0, 1, 7, n, n + 3):
        assert_lists(gpu_device, gc.random_idx(n, K, R, 10 * n + R), R, (n, K, R))


def test_transpose_one_target_many_rows_and_the_hub_graph(gpu_device):
    assert_lists(gpu_device, gc.one_target(), 9, "one target")
    assert_lists(gpu_device, gc.sparse_rows(), 70_000, "70 000 rows")
    assert_lists(gpu_device, gc.hub_graph(), 400, "hubs")
    from opengaussian_amd import knn
    idx = torch.from_numpy(gc.sparse_rows()).to(gpu_device)
    begin, slots = knn.reverse_edges(idx, 70_000)
    wb, ws = gr.reverse_lists(gc.sparse_rows(), 70_000)
    assert np.array_equal(begin.cpu().numpy(), wb) and np.array_equal(slots.cpu().numpy()[:wb[-1]], ws)


# ---- transposed gather-sum and edge dots --------------------------------------------------------------------------------------
def capi_aggregate_t(dev, G, w, idx, R, begin, slots, misalign=False):
    L = _lib()
    n, K = idx.shape
    D = G.shape[1]
    off = 1 if misalign else 0
    gv = _floats(G, dev, off)
    obuf, out = _guarded(R * D, torch.float32, F_CANARY, dev, off)
    assert (out.data_ptr() % 16 == 4) == misalign
    nbytes = int(L.lib().ogs_knn_aggregate_t_tmp_bytes(n, K, R, D))
    tbuf, tmp = _guarded(nbytes, torch.uint8, B_CANARY, dev)
    bt, st, wt = _dev(begin, dev, torch.int32), _dev(slots, dev, torch.int32), _dev(w, dev, torch.float32)
    L.check(L.lib().ogs_knn_aggregate_t(n, K, R, D, L.ptr(bt), L.ptr(st), L.ptr(wt), L.ptr(gv), L.ptr(out), L.ptr(tmp), nbytes,
                                        _stream()), "ogs_knn_aggregate_t")
    torch.cuda.synchronize()
    assert _intact(obuf, out, F_CANARY) and _intact(tbuf, tmp, B_CANARY), (n, K, R, D)
    return out.reshape(R, D).cpu().numpy()


def capi_edge_dots(dev, G, X, idx):
    L = _lib()
    n, K = idx.shape
    R, D = X.shape
    gbuf, gw = _guarded(n * K, torch.float32, F_CANARY, dev)
    it, gv, xv = _dev(idx, dev, torch.int32), _floats(G, dev), _floats(X, dev)
    L.check(L.lib().ogs_knn_edge_dots(n, K, R, D, L.ptr(it), L.ptr(gv), L.ptr(xv), L.ptr(gw), _stream()), "ogs_knn_edge_dots")
    torch.cuda.synchronize()
    assert _intact(gbuf, gw, F_CANARY)
    return gw.reshape(n, K).cpu().numpy()


def _full_slots(slots, E):
    """the restatement's slots padded to the [n * K] the entry points take; the padding is never read"""
    return np.concatenate((slots, np.full(E - len(slots), I_CANARY, np.int32)))


def _graph_cases():
    yield "hubs", gc.hub_graph(), 400
    yield "random", gc.random_idx(131, 16, 97, 5), 97                              # R != n, several workgroups at every D
    yield "K=1", gc.random_idx(300, 1, 300, 6), 300
    yield "K=32", gc.random_idx(70, 32, 75, 7), 75


@pytest.mark.parametrize("D", gc.WIDTHS)
def test_aggregate_t(gpu_device, D):
    for name, idx, R in _graph_cases():
        n, K = idx.shape
        G = gc.features(n, D, 100 + D)
        w = gc.weights(idx, R, 200 + D)                                            # NaN in the invalid slots
        begin, slots = gr.reverse_lists(idx, R)
        slots = _full_slots(slots, n * K)
        want, scale, m = gr.aggregate_t(G, w, idx, R)
        got = {mis: capi_aggregate_t(gpu_device, G, w, idx, R, begin, slots, mis) for mis in (False, True)}
        for mis, g in got.items():
            assert np.isfinite(g).all(), (name, D, mis)
            err = np.abs(g - want)
            assert np.all(err <= (m[:, None] + 2) * U * scale), (name, D, mis, float((err / np.maximum(scale, 1e-30)).max()))
            assert not g[m == 0].any() and not np.signbit(g[m == 0]).any()         # an empty list gives +0
        assert np.array_equal(got[False], got[True])                               # both column forms, the same bytes (D % 4 == 0)
        assert np.array_equal(got[False], capi_aggregate_t(gpu_device, G, w, idx, R, begin, slots))


def test_aggregate_t_survives_lists_that_contradict_themselves(gpu_device):
    """begin values outside [0, n * K], decreasing pairs and slots outside [0, n * K): values are unspecified, addresses are not"""
    idx = gc.hub_graph()
    n, K = idx.shape
    begin, slots = gr.reverse_lists(idx, n)
    slots = _full_slots(slots, n * K)
    begin = begin.copy()
    begin[10], begin[20], begin[30], begin[40] = gc.I32.max, gc.I32.min, -5, n * K + 7
    begin[50:60] = begin[50:60][::-1]
    slots[::7] = np.array([-1, n * K, gc.I32.min, gc.I32.max], np.int32)[np.arange(len(slots[::7])) % 4]
    w = np.ones((n, K), np.float32)
    for D in (4, 5):
        got = capi_aggregate_t(gpu_device, gc.features(n, D, 1), w, idx, n, begin, slots)     # the canaries are the assertion
        assert np.isfinite(got).all()
    everything = np.zeros(n + 1, np.int32)
    everything[1:] = n * K                                                          # every row claims every slot
    capi_aggregate_t(gpu_device, gc.features(n, 4, 1), w, idx, n, everything, slots)


@pytest.mark.parametrize("D", gc.WIDTHS)
def test_edge_dots(gpu_device, D):
    for name, idx, R in _graph_cases():
        n, K = idx.shape
        G, X = gc.features(n, D, 300 + D), gc.features(R, D, 400 + D)
        want, scale = gr.edge_dots(G, X, idx)
        got = capi_edge_dots(gpu_device, G, X, idx)
        err = np.abs(got - want)
        assert np.all(err <= (D + 2) * U * scale), (name, D, float((err / np.maximum(scale, 1e-30)).max()))
        bad = ~gr.valid_slots(idx, R)
        assert bad.any() and not got[bad].any()                                    # exactly 0
        assert np.array_equal(got, capi_edge_dots(gpu_device, G, X, idx))


def test_adjoint_identity_through_the_public_api(gpu_device):
    from opengaussian_amd import knn
    for name, idx, R in _graph_cases():
        n, K = idx.shape
        for D in (6, 64):
            Xn, Gn = gc.features(R, D, 1), gc.features(n, D, 2)
            wn = np.nan_to_num(gc.weights(idx, R, 3))                              # autograd's own w * 0 must stay finite
            X = _dev(Xn, gpu_device).requires_grad_(True)
            out = knn.gather_sum(X, _dev(idx, gpu_device), _dev(wn, gpu_device))
            assert out.requires_grad and torch.equal(out, knn.aggregate(X, _dev(idx, gpu_device), _dev(wn, gpu_device)))
            out.backward(_dev(Gn, gpu_device))
            lhs = float((out.detach().cpu().numpy().astype(np.float64) * Gn).sum())
            rhs = float((Xn.astype(np.float64) * X.grad.cpu().numpy()).sum())
            _, fscale = nr.aggregate(Xn, idx, wn)
            _, tscale, m = gr.aggregate_t(Gn, wn, idx, R)
            bar = ((K + 2) * U * fscale * np.abs(Gn)).sum() + ((m[:, None] + 2) * U * tscale * np.abs(Xn)).sum()
            assert abs(lhs - rhs) <= bar, (name, D, abs(lhs - rhs), bar)


# ---- autograd -----------------------------------------------------------------------------------------------------------------
def _table(dev, n, K, seed):
    from opengaussian_amd import knn, query
    pts = torch.from_numpy(kc.cloud(n, seed)).to(dev)
    idx, d2 = knn.neighbors(pts, K)
    return idx, query.neighbor_weights(d2, idx)


def _f64_grads(fn, X, w, G):
    """(gX, gw) of <fn(X, w), G> in float64 on the CPU"""
    X = torch.from_numpy(np.asarray(X, np.float64)).requires_grad_(True)
    w = torch.from_numpy(np.asarray(w, np.float64)).requires_grad_(True)
    (fn(X, w) * torch.from_numpy(np.asarray(G, np.float64))).sum().backward()
    return X.grad.numpy(), w.grad.numpy()


@pytest.mark.parametrize("K,D", [(1, 6), (16, 6), (1, 65), (16, 65)])
def test_gather_sum_gradients(gpu_device, K, D):
    from opengaussian_amd import knn
    n = 257
    idx, w0 = _table(gpu_device, n, K, 70 + K)
    rng = np.random.default_rng(K * D)
    wn = (w0.cpu().numpy() * rng.uniform(0.5, 1.5, (n, K))).astype(np.float32)
    Xn, Gn = gc.features(n, D, 1), gc.features(n, D, 2)
    il = idx.long().cpu()
    want_x, want_w = _f64_grads(lambda X, w: (w[..., None] * X[il]).sum(1), Xn, wn, Gn)
    _, sx, m = gr.aggregate_t(Gn, wn, idx.cpu().numpy(), n)
    _, sw = gr.edge_dots(Gn, Xn, idx.cpu().numpy())
    grads = []
    for reverse in (None, knn.reverse_edges(idx)):
        X, w = _dev(Xn, gpu_device).requires_grad_(True), _dev(wn, gpu_device).requires_grad_(True)
        out = knn.gather_sum(X, idx, w, reverse)
        assert torch.equal(out, knn.aggregate(X, idx, w))                          # the forward's bytes
        out.backward(_dev(Gn, gpu_device))
        gx, gw = X.grad.cpu().numpy(), w.grad.cpu().numpy()
        assert np.all(np.abs(gx - want_x) <= (m[:, None] + 2) * U * sx), (K, D, "gX")
        assert np.all(np.abs(gw - want_w) <= (D + 2) * U * sw), (K, D, "gw")
        grads.append((gx, gw))
    assert np.array_equal(grads[0][0], grads[1][0]) and np.array_equal(grads[0][1], grads[1][1])     # lazy and given lists
    X = _dev(Xn, gpu_device).requires_grad_(True)                                  # w without a gradient: no edge dots
    knn.gather_sum(X, idx, _dev(wn, gpu_device)).backward(_dev(Gn, gpu_device))
    assert np.array_equal(X.grad.cpu().numpy(), grads[0][0])


@pytest.mark.parametrize("K,D", [(1, 6), (16, 6), (16, 65)])
def test_diffuse_gradients(gpu_device, K, D):
    from opengaussian_amd import knn, query
    n, steps, rate = 257, 2, 0.5
    idx, w0 = _table(gpu_device, n, K, 80 + K)
    rng = np.random.default_rng(K + D)
    wn = (w0.cpu().numpy() * rng.uniform(0.5, 1.5, (n, K))).astype(np.float32)
    wn[11] = 0                                                                      # a row without a neighbour keeps its value
    fixed = rng.random(n) > 0.7
    fixed[11] = False
    Xn, Gn = gc.features(n, D, 3), gc.features(n, D, 4)
    il = idx.long().cpu()
    keep = torch.from_numpy(fixed | ~(wn != 0).any(1))

    def f64(X, w):
        for _ in range(steps):
            X = torch.where(keep[:, None], X, (1.0 - rate) * X + rate * (w[..., None] * X[il]).sum(1))
        return X

    want_x, want_w = _f64_grads(f64, Xn, wn, Gn)
    sx, sw = _f64_grads(f64, np.abs(Xn), np.abs(wn), np.abs(Gn))                    # the sums of the absolute path products
    deg = int(gr.in_degree(idx.cpu().numpy(), n).max())
    roundings = steps * (max(K, deg) + 6) + D + 2
    fx, ft = _dev(fixed, gpu_device), _dev(Gn, gpu_device)
    grads = []
    for reverse in (None, knn.reverse_edges(idx)):
        X, w = _dev(Xn, gpu_device).requires_grad_(True), _dev(wn, gpu_device).requires_grad_(True)
        out = query.diffuse(X, idx, w, steps=steps, rate=rate, fixed=fx, reverse=reverse)
        assert torch.equal(out, query.diffuse_features(X, idx, w, steps=steps, rate=rate, fixed=fx))
        out.backward(ft)
        gx, gw = X.grad.cpu().numpy(), w.grad.cpu().numpy()
        assert np.all(np.abs(gx - want_x) <= roundings * U * sx), (K, D, "gX", float(np.abs(gx - want_x).max()))
        assert np.all(np.abs(gw - want_w) <= roundings * U * sw), (K, D, "gw", float(np.abs(gw - want_w).max()))
        grads.append((gx, gw))
    assert np.array_equal(grads[0][0], grads[1][0]) and np.array_equal(grads[0][1], grads[1][1])
    assert torch.equal(query.diffuse(_dev(Xn, gpu_device), idx, _dev(wn, gpu_device), steps=0), _dev(Xn, gpu_device))


# ---- neighbour smoothness -----------------------------------------------------------------------------------------------------
def _smoothness_checks(dev, F, idx, w, what):
    """energies, total, both reductions and both gradients of one graph; returns the gradients' bytes"""
    from opengaussian_amd import knn, query
    n, K = idx.shape
    D = F.shape[1]
    it = _dev(idx, dev, torch.int32)
    e_want, e_scale, d2, ok = gr.smoothness(F, idx, w)
    energy, total = knn.smoothness_energy(_dev(F, dev), it, _dev(w, dev))
    e_got = energy.cpu().numpy()
    assert energy.dtype == torch.float32 and total.dtype == torch.float64
    assert np.all(np.abs(e_got - e_want) <= (K * D + 8) * U * e_scale), (what, "row energies")
    assert not e_got[~ok.any(1)].any()                                             # no valid slot: energy 0
    tot = total.cpu().numpy()
    ref_total = float(e_got.astype(np.float64).sum())
    assert abs(tot[0] - ref_total) <= 1e-12 * abs(ref_total) and tot[1] == ok.sum(), (what, "total")
    out = {}
    for reduction in ("sum", "mean"):
        norm = 1.0 if reduction == "sum" else (1.0 / ok.sum() if ok.any() else 0.0)
        for reverse in (None, knn.reverse_edges(it)):
            Ft, wt = _dev(F, dev).requires_grad_(True), _dev(w, dev).requires_grad_(True)
            loss = query.neighbor_smoothness(Ft, it, wt, reverse=reverse, reduction=reduction)
            assert loss.dtype == torch.float32 and loss.dim() == 0
            assert abs(float(loss.detach()) - tot[0] * norm) <= U * abs(tot[0] * norm)      # the fp64 total, rounded once
            loss.backward()
            gF, gw = Ft.grad.cpu().numpy(), wt.grad.cpu().numpy()
            want_F, sF, m, want_w = gr.smoothness_grad(F, idx, w, norm)
            assert np.all(np.abs(gF - want_F) <= (m[:, None] + 6) * U * sF), (what, reduction, "gF", float(np.abs(gF - want_F).max()))
            assert np.all(np.abs(gw - want_w) <= (D + 6) * U * np.abs(want_w)), (what, reduction, "gw")
            assert not gw[~ok].any()
            key = (reduction, "gF"), (reduction, "gw")
            if key[0] in out:                                                      # lazy and given lists: the same bytes
                assert np.array_equal(out[key[0]], gF) and np.array_equal(out[key[1]], gw)
            out[key[0]], out[key[1]] = gF, gw
    return out, e_got, tot


def _autograd_smoothness(F, idx, w, norm):
    """float64 torch autograd of the composition on the CPU: (gF, gw)"""
    ok = torch.from_numpy(gr.valid_slots(idx, len(F)))
    il = torch.from_numpy(np.where(ok.numpy(), idx, 0).astype(np.int64))
    Ft = torch.from_numpy(np.asarray(F, np.float64)).requires_grad_(True)
    wt = torch.from_numpy(np.nan_to_num(np.asarray(w, np.float64))).requires_grad_(True)
    d2 = ((Ft[:, None, :] - Ft[il]) ** 2).sum(-1)
    (norm * (torch.where(ok, wt * d2, torch.zeros_like(d2))).sum()).backward()
    return Ft.grad.numpy(), wt.grad.numpy()


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_neighbor_smoothness_on_neighbour_tables(gpu_device, n):
    from opengaussian_amd import knn
    pts = torch.from_numpy(kc.cloud(n, 500 + n)).to(gpu_device)
    for K in (1, 4, 16):
        idx = knn.neighbors(pts, K)[0].cpu().numpy()
        for D in (1, 6, 65):
            F = gc.features(n, D, n + K + D)
            w = gc.weights(idx, n, n * K + D, positive=True)
            out, _, _ = _smoothness_checks(gpu_device, F, idx, w, (n, K, D))
            ok = gr.valid_slots(idx, n)
            want_F, want_w = _autograd_smoothness(F, idx, w, 1.0)                  # the restatement's gradient IS autograd's
            ref_F, sF, m, ref_w = gr.smoothness_grad(F, idx, w, 1.0)
            assert np.all(np.abs(ref_F - want_F) <= 1e-12 * np.maximum(sF, 1e-300)) and np.allclose(ref_w, want_w, rtol=1e-12, atol=0)
            assert np.all(np.abs(out[("sum", "gF")] - want_F) <= (m[:, None] + 6) * U * sF)
            assert np.all(np.abs(out[("sum", "gw")] - want_w) <= (D + 6) * U * np.abs(want_w)) and ok.shape == (n, K)


def test_neighbor_smoothness_hubs_invalid_rows_and_coincident_features(gpu_device):
    from opengaussian_amd import query
    idx = gc.hub_graph()
    n, K = idx.shape
    for D in (4, 5):                                                               # both column forms past the chunk size
        F = gc.features(n, D, 9 + D)
        w = gc.weights(idx, n, 10 + D, positive=True)
        out, e_got, _ = _smoothness_checks(gpu_device, F, idx, w, ("hubs", D))
        assert e_got[n - 1] == 0                                                   # a row whose slots are all invalid ...
        want_F, want_w = _autograd_smoothness(F, idx, w, 1.0)
        _, sF, m, _ = gr.smoothness_grad(F, idx, w, 1.0)
        assert np.all(np.abs(out[("sum", "gF")] - want_F) <= (m[:, None] + 6) * U * sF)
        assert np.all(np.abs(out[("sum", "gw")] - want_w) <= (D + 6) * U * np.abs(want_w))
    # ... takes its gradient from its in-edges alone: point two slots at it
    idx2 = idx.copy()
    idx2[200, 0], idx2[201, 1] = n - 1, n - 1
    F = gc.features(n, 6, 21)
    w = gc.weights(idx2, n, 22, positive=True)
    out, e_got, _ = _smoothness_checks(gpu_device, F, idx2, w, "in-edges only")
    want = 2.0 * (w[200, 0] * (F[n - 1].astype(np.float64) - F[200]) + w[201, 1] * (F[n - 1].astype(np.float64) - F[201]))
    assert e_got[n - 1] == 0 and out[("sum", "gF")][n - 1].any()
    assert np.all(np.abs(out[("sum", "gF")][n - 1] - want) <= 8 * U * 2.0 * (np.abs(w[200, 0] * (F[n - 1] - F[200])) +
                                                                             np.abs(w[201, 1] * (F[n - 1] - F[201]))))
    # coincident features: exactly 0 everywhere, whatever the weights
    same = np.tile(gc.features(1, 6, 5), (n, 1))
    it, wt = _dev(idx2, gpu_device), _dev(np.nan_to_num(w) * 1e6, gpu_device)
    Ft = _dev(same, gpu_device).requires_grad_(True)
    for reduction in ("sum", "mean"):
        loss = query.neighbor_smoothness(Ft, it, wt, reduction=reduction)
        assert float(loss.detach()) == 0.0
        Ft.grad = None
        loss.backward()
        assert not Ft.grad.any()
    none = np.full((5, 3), -1, np.int32)                                           # a graph without an edge: loss 0, not 0 / 0
    Ft = _dev(gc.features(5, 4, 1), gpu_device).requires_grad_(True)
    loss = query.neighbor_smoothness(Ft, _dev(none, gpu_device), _dev(np.ones((5, 3), np.float32), gpu_device))
    loss.backward()
    assert float(loss.detach()) == 0.0 and not Ft.grad.any()


def test_bad_arguments_are_errors_and_empty_input_is_fine(gpu_device):
    L = _lib()
    from opengaussian_amd import knn, query
    s = _stream()
    n, K, R, D = 10, 2, 10, 3
    idx = torch.zeros((n, K), dtype=torch.int32, device=gpu_device)
    f = torch.full((64,), F_CANARY, dtype=torch.float32, device=gpu_device)
    b = torch.full((64,), I_CANARY, dtype=torch.int32, device=gpu_device)
    tmp = torch.empty(1 << 16, dtype=torch.uint8, device=gpu_device)
    lib = L.lib()
    assert lib.ogs_knn_transpose(-1, K, R, L.ptr(idx), L.ptr(b), L.ptr(b), L.ptr(tmp), 1 << 16, s) == -1
    assert lib.ogs_knn_transpose(1 << 27, 16, R, L.ptr(idx), L.ptr(b), L.ptr(b), L.ptr(tmp), 1 << 16, s) == -1      # n * K = 2^31
    assert lib.ogs_knn_transpose(n, K, 1 << 31, L.ptr(idx), L.ptr(b), L.ptr(b), L.ptr(tmp), 1 << 16, s) == -1
    assert lib.ogs_knn_transpose(n, K, R, None, L.ptr(b), L.ptr(b), L.ptr(tmp), 1 << 16, s) == -1
    assert lib.ogs_knn_transpose(n, K, R, L.ptr(idx), L.ptr(b), L.ptr(b), L.ptr(tmp), 8, s) == -1 and b"tmp" in lib.ogs_last_error()
    assert lib.ogs_knn_aggregate_t(n, K, R, 0, L.ptr(b), L.ptr(b), L.ptr(f), L.ptr(f), L.ptr(f), L.ptr(tmp), 1 << 16, s) == -1
    assert lib.ogs_knn_aggregate_t(n, K, R, D, None, L.ptr(b), L.ptr(f), L.ptr(f), L.ptr(f), L.ptr(tmp), 1 << 16, s) == -1
    assert lib.ogs_knn_aggregate_t(n, K, R, D, L.ptr(b), L.ptr(b), L.ptr(f), L.ptr(f), L.ptr(f), L.ptr(tmp), 8, s) == -1
    assert lib.ogs_knn_edge_dots(n, K, R, 0, L.ptr(idx), L.ptr(f), L.ptr(f), L.ptr(f), s) == -1
    assert lib.ogs_knn_edge_dots(n, K, R, D, L.ptr(idx), None, L.ptr(f), L.ptr(f), s) == -1
    assert lib.ogs_knn_smoothness_fwd(n, K, D, L.ptr(idx), L.ptr(f), L.ptr(f), L.ptr(f), None, L.ptr(tmp), 1 << 16, s) == -1
    assert lib.ogs_knn_smoothness_fwd(n, K, D, L.ptr(idx), L.ptr(f), L.ptr(f), L.ptr(f), L.ptr(tmp), L.ptr(tmp), 8, s) == -1
    assert lib.ogs_knn_smoothness_bwd(n, K, D, L.ptr(idx), L.ptr(f), L.ptr(f), L.ptr(b), L.ptr(b), None, L.ptr(f), None,
                                      L.ptr(tmp), 1 << 16, s) == -1
    assert lib.ogs_knn_smoothness_bwd(n, K, 0, L.ptr(idx), L.ptr(f), L.ptr(f), L.ptr(b), L.ptr(b), L.ptr(f), L.ptr(f), None,
                                      L.ptr(tmp), 1 << 16, s) == -1
    torch.cuda.synchronize()
    assert bool((f == F_CANARY).all()) and bool((b == I_CANARY).all())             # none of these calls wrote anything
    begin, slots = knn.reverse_edges(torch.zeros((0, 4), dtype=torch.int32, device=gpu_device))
    assert begin.tolist() == [0] and slots.numel() == 0
    begin, _ = knn.reverse_edges(torch.zeros((0, 4), dtype=torch.int32, device=gpu_device), 3)
    assert begin.tolist() == [0, 0, 0, 0]
    X = torch.rand(5, 3, device=gpu_device, requires_grad=True)                    # a table without a row: an empty sum, a zero gradient
    out = knn.gather_sum(X, torch.zeros((0, 2), dtype=torch.int32, device=gpu_device), torch.zeros((0, 2), device=gpu_device))
    out.sum().backward()
    assert out.shape == (0, 3) and not X.grad.any()
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn.reverse_edges(torch.zeros((4, 2), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn.gather_sum(torch.rand(4, 3), torch.zeros((4, 2), dtype=torch.int32), torch.rand(4, 2))
    with pytest.raises(ValueError):
        query.neighbor_smoothness(X, idx[:5], torch.rand(5, 2, device=gpu_device), reduction="max")
    with pytest.raises(ValueError):
        query.neighbor_smoothness(X, idx, torch.rand(10, 2, device=gpu_device))    # not square
    with pytest.raises(ValueError):
        knn.gather_sum(X, idx, torch.rand(10, 2, device=gpu_device), reverse=knn.reverse_edges(idx, 7))
