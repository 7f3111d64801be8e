"""CPU: tests/knn_graph_restatement.py pinned to per-row Python loops, and what tests/test_37c_knn_graph_gpu.py relies on in
tests/knn_graph_cases.py."""
import numpy as np

from tests import knn_cases as kc
from tests import knn_graph_cases as gc
from tests import knn_graph_restatement as gr
from tests import knn_neighbors_restatement as nr


def _graphs():
    """(name, idx, R) small enough for the loops"""
    pts = kc.cloud(65, 11)
    out = [("table", nr.neighbors(pts, 4)[0], 65), ("short", nr.neighbors(kc.cloud(3, 2), 4)[0], 3)]
    out += [(f"random/R={R}", gc.random_idx(23, 3, R, 40 + R), R) for R in (0, 1, 7, 23, 26)]
    out.append(("one", gc.one_target(7, 3, 9, 5), 9))
    return out


def _lists_by_loop(idx, R):
    flat = idx.reshape(-1)
    return [[e for e in range(len(flat)) if flat[e] == r] for r in range(R)]


def test_reverse_lists_are_the_per_row_lists():
    for name, idx, R in _graphs():
        begin, slots = gr.reverse_lists(idx, R)
        lists = _lists_by_loop(idx, R)
        assert begin.dtype == np.int32 and slots.dtype == np.int32 and len(begin) == R + 1 and begin[0] == 0, name
        assert begin[R] == len(slots) == int(gr.valid_slots(idx, R).sum()), name
        for r in range(R):
            assert list(slots[begin[r]:begin[r + 1]]) == lists[r], (name, r)
        assert np.array_equal(gr.in_degree(idx, R), [len(l) for l in lists]), name


def test_aggregate_t_and_edge_dots_are_the_loops():
    for name, idx, R in _graphs():
        n, K = idx.shape
        for D in (1, 5):
            G, X = gc.features(n, D, 1).astype(np.float64), gc.features(R, D, 2).astype(np.float64)
            w = gc.weights(idx, R, 3)
            out, scale, m = gr.aggregate_t(G, w, idx, R)
            gw, gscale = gr.edge_dots(G, X, idx)
            lists = _lists_by_loop(idx, R)
            for r in range(R):
                want = sum((float(w.reshape(-1)[e]) * G[e // K] for e in lists[r]), np.zeros(D))
                assert np.allclose(out[r], want, rtol=1e-13, atol=1e-13) and m[r] == len(lists[r]), (name, r)
                assert np.all(scale[r] >= np.abs(out[r]) - 1e-13)
            for i in range(n):
                for k in range(K):
                    j = int(idx[i, k])
                    want = float(G[i] @ X[j]) if 0 <= j < R else 0.0
                    assert abs(gw[i, k] - want) <= 1e-13 and (0 <= j < R or (gw[i, k] == 0 and gscale[i, k] == 0)), (name, i, k)
            assert np.isfinite(out).all() and np.isfinite(gw).all(), name           # the parked NaNs were not read
            # adjoint: <aggregate(X), G> = <X, aggregate_t(G)>
            if R > 0:
                fwd, _ = nr.aggregate(X, idx, w)
                assert abs((fwd * G).sum() - (X * out).sum()) <= 1e-10 * max(1.0, scale.sum()), name


def test_smoothness_is_the_loop_and_its_gradient_is_the_difference_quotient():
    for name, idx, R in _graphs():
        n, K = idx.shape
        if R != n:
            continue
        F = gc.features(n, 3, 5).astype(np.float64)
        w = gc.weights(idx, n, 6, positive=True)
        e, scale, d2, ok = gr.smoothness(F, idx, w)
        for i in range(n):
            want = sum(float(w[i, k]) * float(((F[i] - F[idx[i, k]]) ** 2).sum()) for k in range(K) if 0 <= idx[i, k] < n)
            assert abs(e[i] - want) <= 1e-12 * max(1.0, abs(want)), (name, i)
        assert np.array_equal(scale, e) and np.isfinite(e).all()                  # positive weights
        gF, sF, m, gw = gr.smoothness_grad(F, idx, w, scale=0.5)
        assert np.array_equal(m, ok.sum(1) + gr.in_degree(idx, n)) and np.array_equal(gw, 0.5 * d2)
        h = 1e-6
        rng = np.random.default_rng(0)
        for _ in range(12):
            i, c = int(rng.integers(n)), int(rng.integers(3))
            Fp, Fm = F.copy(), F.copy()
            Fp[i, c] += h
            Fm[i, c] -= h
            fd = 0.5 * (gr.smoothness(Fp, idx, w)[0].sum() - gr.smoothness(Fm, idx, w)[0].sum()) / (2 * h)
            assert abs(gF[i, c] - fd) <= 1e-6 * max(1.0, sF[i, c]), (name, i, c)


def test_the_cases_hold_what_the_gpu_tests_rely_on():
    idx = gc.hub_graph()
    n, K = idx.shape
    deg = gr.in_degree(idx, n)
    assert tuple(deg[:4]) == gc.HUB_DEGREES == (gc.CHUNK - 1, gc.CHUNK, gc.CHUNK + 1, 2 * gc.CHUNK + 3)
    assert (deg[n // 2:] == 0).all() and (deg[4:n // 2] > 0).any() and deg[4:].max() < gc.CHUNK
    assert n * K - sum(gc.HUB_DEGREES) >= 300
    assert not gr.valid_slots(idx[n - 1], n).any()                               # a row without a valid slot
    for name, table, R in (("hub", idx, n), ("random", gc.random_idx(64, 4, 64, 1), 64), ("sparse", gc.sparse_rows(), 70_000)):
        for v in gc.invalid_values(R):
            assert (table == v).any(), (name, int(v))
        assert (gr.in_degree(table, R) == 0).any(), name
    assert (gr.in_degree(gc.sparse_rows(), 70_000) == 0).mean() > 0.9 and 70_000 > 1 << 16
    assert not gr.valid_slots(gc.random_idx(5, 3, 0, 1), 0).any()
    one = gc.one_target()
    assert gr.in_degree(one, 9)[5] == one.size > gc.CHUNK
    w = gc.weights(idx, n, 1)
    assert np.isnan(w[~gr.valid_slots(idx, n)]).all() and np.isfinite(w[gr.valid_slots(idx, n)]).all()
    # the short clouds' tables hold -1 slots
    for nn in (1, 2, 5):
        assert (nr.neighbors(kc.cloud(nn, 300 + nn), 16)[0] == -1).any()


def test_the_chunk_size_is_the_library_s():
    from opengaussian_amd import _lib, build
    import os
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    assert int(_lib.lib().ogs_knn_transpose_chunk()) == gc.CHUNK
    assert _lib.lib().ogs_knn_transpose_tmp_bytes(100, 16, 100) >= 3 * 4 * 1600
    assert _lib.lib().ogs_knn_transpose_tmp_bytes(1 << 27, 16, 100) == 0       # n * K = 2^31
    assert _lib.lib().ogs_knn_aggregate_t_tmp_bytes(100, 16, 100, 6) > 0
