"""GPU: the open-vocabulary query kernels (include/ogs_query.h) through opengaussian_amd.query, against the NumPy restatement
(tests/query_restatement.py), the goldens made by the reference's own code (tests/golden/query_golden.npz) and, for
render_queries, against one render(selected_leaf_id=...) call per query.

Similarities: 2 * D * 2^-24 absolute from the fp64 restatement (the summation-order bound of a dot product of two unit
vectors, doubled for the two normalisations).  Everything else is exact: ids and counts on inputs whose decisions have margins
(tests/test_query_host.py checks them on the CPU), integer tables, row lists, and images bit for bit."""
import os

import numpy as np
import pytest
import torch

from tests import query_cases as qc
from tests import query_restatement as qr
from tests.test_query_host import GOLD, _expected_sets, _scene_model, _words_i64, gold_case, same_scalars

pytestmark = pytest.mark.gpu

TOP = 10


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _lib():
    from opengaussian_amd import _lib
    return _lib.lib()


def sim_bar(D):
    return 2.0 * D * 2.0 ** -24


def run_select(dev, c, min_occu=5, top=TOP):
    from opengaussian_amd import query
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sim, sel, cnt = query.select_leaves_by_text(T(c["text"]), T(c["leaf"]), T(c["occu"]), T(c["centers"]), float(c["leaf_num"]),
                                                min_occu=min_occu, top=top)
    return sim.cpu().numpy(), sel.cpu().numpy(), cnt.cpu().numpy()


# ---- similarity / selection ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", qc.SHAPE_DS)
@pytest.mark.parametrize("K", qc.SHAPE_KS)
def test_similarity_and_selection_shapes(gpu_device, K, D):
    """Every (K, D) at Q = 1 and 21.  `selected` / `count` are compared exactly on the rows qc.shape_decided keeps: ranks
    apart by the margins, or tied at a similarity that is exactly 0 on both sides (a fifth of the leaves are zeroed, so at
    K <= top + 1 every row ranks some of them).  At D > 1 that is at least qc.SHAPE_MIN_EXACT of the 22 rows of every K
    (tests/test_query_host.py asserts the same without a GPU); at D = 1 every similarity is +-1 or 0: the zero text row is always
    compared, the others when the similarities came out exact (see below)."""
    assert int(_lib().ogs_query_max_leaves()) == qc.MAX_LEAVES
    worst, exact_rows = 0.0, 0
    for Q in qc.SHAPE_QS:
        c = qc.shape_case(K, D, Q)
        sim, sel, cnt = run_select(gpu_device, c)
        s64, want_sel, want_cnt = qr.select_leaves(c["text"], c["leaf"], c["occu"], c["centers"], c["leaf_num"], top=TOP)
        err = float(np.abs(sim - s64).max())
        worst = max(worst, err)
        assert err <= sim_bar(D), (K, D, Q, err)
        assert not sim[:, c["occu"] < 5].any()                  # zeroed leaves: exact zeros
        assert (cnt >= 1).all() and (cnt <= min(TOP, K)).all() and (sel[np.arange(TOP)[None, :] >= cnt[:, None]] == -1).all()
        assert ((sel >= -1) & (sel < K)).all()
        # D = 1: the kernel's fl(t * l) / fl(|t| * |l|) is +-1 exactly where sqrt and the quotient are correctly rounded; then
        # the ties among them are the restatement's ties and every row is compared (the bar above does not demand it)
        ok = qc.shape_decided(c, s64, all_exact=D == 1 and err == 0.0)
        assert np.array_equal(sel[ok], want_sel[ok]) and np.array_equal(cnt[ok], want_cnt[ok]), (K, D, Q)
        exact_rows += int(ok.sum())
        if Q > 1:
            assert ok[2] and not sim[2].any() and sel[2, 0] == 0            # the zero text row: every leaf ties at exactly 0
    print(f"similarity K={K} D={D}: worst |sim - fp64| = {worst:.3e} (bar {sim_bar(D):.3e}), rows compared exactly: {exact_rows}")
    assert exact_rows >= (qc.SHAPE_MIN_EXACT if D > 1 else 1)


@pytest.mark.parametrize("K,D", [(640, 512), ("limit", 513)])
def test_selection_exact_on_planted_ranks(gpu_device, K, D):
    K = int(_lib().ogs_query_max_leaves()) if K == "limit" else K
    c = qc.planted_case(K, D, 21)
    sim, sel, cnt = run_select(gpu_device, c)
    s64, want_sel, want_cnt = qr.select_leaves(c["text"], c["leaf"], c["occu"], c["centers"], c["leaf_num"], top=TOP)
    err = float(np.abs(sim - s64).max())
    print(f"planted K={K} D={D}: worst |sim - fp64| = {err:.3e} (bar {sim_bar(D):.3e})")
    assert err <= sim_bar(D)
    assert np.array_equal(sel, want_sel) and np.array_equal(cnt, want_cnt)
    assert not sim[0].any() and list(sel[0]) == [0] + [-1] * 9          # the zero text: every leaf ties, the lowest index wins


def test_selection_equals_the_goldens(gpu_device, gold):
    for seed in gold["seeds"]:
        g = gold_case(gold, seed)
        sim, sel, cnt = run_select(gpu_device, g)
        assert np.array_equal(sel, g["selected"]) and np.array_equal(cnt, g["count"]), seed
        assert np.abs(sim - qr.similarity(g["text"], g["leaf"], g["occu"], 5)).max() <= sim_bar(qc.GOLD_D)
    small = qc.small_case()                                             # K < top: only K are ranked, and every one is appended
    sim, sel, cnt = run_select(gpu_device, small)
    s64, want_sel, _ = qr.select_leaves(small["text"], small["leaf"], small["occu"], small["centers"], small["leaf_num"], top=TOP)
    assert (cnt == 7).all() and (sel[:, 7:] == -1).all()
    assert np.array_equal(sel, want_sel) and np.array_equal(sel[:, :7], np.argsort(-s64, axis=1, kind="stable"))   # the rank ORDER
    every = qc.text_case(6)                                             # every leaf zeroed: best 0, candidates 1 .. 9
    sim, sel, cnt = run_select(gpu_device, dict(every, occu=np.zeros(qc.GOLD_K, np.int64), centers=np.zeros((61, 6), np.float32),
                                                leaf_num=60.0))
    assert not sim.any() and (cnt == 10).all() and (sel == np.arange(10)).all()


# ---- point classes, confusion table, metrics -----------------------------------------------------------------------------------
def test_classes_and_metrics_equal_the_goldens(gpu_device, gold):
    from opengaussian_amd import query
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    for seed in gold["seeds"]:
        g = gold_case(gold, seed)
        assert (g["leaf_ind"] == qc.GOLD_K).any()                       # ids that are clamped at K - 1
        pred = query.classify_points(T(g["text"]), T(g["leaf"]), T(g["occu"]), T(g["leaf_ind"]))
        assert pred.dtype == torch.int64 and np.array_equal(pred.cpu().numpy(), g["pred"]), seed
        for tag, ign in (("plain", None), ("ignore", g["ignore"])):
            conf = query.confusion_table(T(g["gt"]), pred, qc.GOLD_Q + 1, None if ign is None else T(ign))
            assert np.array_equal(conf.cpu().numpy(), qr.confusion(g["gt"], g["pred"], qc.GOLD_Q + 1, ign))
            ious, *scalars = query.segmentation_metrics(T(g["gt"]), pred, qc.GOLD_Q + 1, None if ign is None else T(ign))
            assert np.array_equal(ious.numpy(), gold[f"s{seed}/{tag}/ious"]) and same_scalars(scalars, gold[f"s{seed}/{tag}/scalars"])
            r_ious, *r_scalars = qr.metrics(conf.cpu().numpy())
            assert np.array_equal(ious.numpy(), r_ious) and same_scalars(scalars, r_scalars)


def _conf_sizes():
    block = int(_lib().ogs_query_confusion_block())
    return [0, 1, 65, block - 1, block, block + 1, 100_003]


@pytest.mark.parametrize("C", [2, 20, 41])
def test_confusion_table_sizes(gpu_device, C):
    from opengaussian_amd import query
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    for n in _conf_sizes():
        rng = np.random.default_rng(9000 + n + C)
        gt, pred, ign = rng.integers(0, C, n), rng.integers(0, C, n), rng.random(n) < 0.1
        for ignore in (None, ign):
            conf = query.confusion_table(T(gt), T(pred), C, None if ignore is None else T(ignore)).cpu().numpy()
            want = qr.confusion(gt, pred, C, ignore)
            assert conf.dtype == np.int64 and np.array_equal(conf, want) and conf.sum() == n, (n, C)
            ious, *scalars = query.metrics_from_confusion(torch.from_numpy(conf))
            r_ious, *r_scalars = qr.metrics(want)
            assert np.array_equal(ious.numpy(), r_ious) and same_scalars(scalars, r_scalars)
    n = 100_003
    one = query.confusion_table(T(np.full(n, C - 1)), T(np.full(n, 1)), C).cpu().numpy()                   # every point in one cell
    assert one[C - 1, 1] == n and one.sum() == n
    ious, *scalars = query.segmentation_metrics(T(np.zeros(n, np.int64)), T(np.full(n, 1)), C)             # unlabelled: nan
    assert not ious.any() and all(np.isnan(s) for s in scalars)
    with pytest.raises(ValueError, match="outside"):
        query.confusion_table(T(np.array([0, C])), T(np.array([0, 0])), C)
    # a sentinel where the reference overwrites it: a prediction at an unlabelled point, a label under `ignore`
    held = query.confusion_table(T(np.array([0, 1, 99, 1])), T(np.array([-1, 1, C, 0])), C, T(np.array([False, False, True, False])))
    assert np.array_equal(held.cpu().numpy(), qr.confusion([0, 1, 0, 1], [0, 1, 0, 0], C))


# ---- the split ------------------------------------------------------------------------------------------------------------
def _split_sizes():
    block = int(_lib().ogs_query_split_block())
    return [0, 1, 63, 64, 65, block, block + 1, 3 * block + 17]


@pytest.mark.parametrize("Q", [1, 2, 33, 64])
def test_multi_split_sizes(gpu_device, Q):
    from opengaussian_amd import query
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    for n in _split_sizes():
        assert int(_lib().ogs_query_split_tmp_bytes(n, Q)) > 0
        for holes in (False, True):
            c = qc.split_case(n, Q, holes=holes)
            for row_ok, keep in ((None, None), (c["row_ok"], None), (None, c["group_keep"]), (c["row_ok"], c["group_keep"])):
                begin, rows, counts = query.multi_split(T(c["leaf_ind"]), _words_i64(c["words"]).to(gpu_device), Q,
                                                        None if row_ok is None else T(row_ok), None if keep is None else T(keep))
                w_begin, w_rows, w_counts = qr.multi_split(c["leaf_ind"], c["words"], Q, row_ok, keep)
                assert np.array_equal(begin.cpu().numpy(), w_begin), (n, Q, holes)
                assert np.array_equal(rows.cpu().numpy(), w_rows), (n, Q, holes)
                assert np.array_equal(counts.cpu().numpy(), w_counts), (n, Q, holes)
                member = torch.from_numpy(qr.membership(c["leaf_ind"], c["words"], Q, row_ok, keep))
                for q in range(Q):                                      # the statement itself: torch.nonzero per group
                    assert torch.equal(rows[begin[q]:begin[q + 1]].cpu(), torch.nonzero(member[:, q]).flatten())


def test_split_scatter_stays_inside_its_capacity(gpu_device):
    """A capacity below the counts (count and scatter disagreeing): nothing is written at or past it, and the library's sticky
    status reports it."""
    from opengaussian_amd import _lib, query
    c = qc.split_case(3000, 8, holes=False)
    ind = torch.from_numpy(c["leaf_ind"]).to(gpu_device)
    sp = query._Split(ind, _words_i64(c["words"]).to(gpu_device), 8, None)
    total = int(sp.counts.sum())
    want = qr.multi_split(c["leaf_ind"], c["words"], 8)[1]
    assert total == len(want) and total > 100
    rows = torch.full((total,), -7, dtype=torch.int64, device=gpu_device)
    cap = total - 50
    status = 0
    try:
        _lib.check(_lib.lib().ogs_query_split_scatter(3000, _lib.ptr(ind), c["K"], _lib.ptr(sp.words), None, 8, None,
                                                      _lib.ptr(sp.tmp), _lib.ptr(rows), cap,
                                                      torch.cuda.current_stream().cuda_stream), "scatter")
    finally:                                                            # the status word is the library's: never leave it set
        torch.cuda.synchronize()
        status = _lib.lib().ogs_check_async_status()                    # read and cleared, whatever follows
        message = _lib.lib().ogs_last_error()
    assert status != 0 and b"capacity" in message
    assert np.array_equal(rows[:cap].cpu().numpy(), want[:cap]) and (rows[cap:] == -7).all()
    assert _lib.lib().ogs_check_async_status() == 0


def test_limits_raise(gpu_device):
    from opengaussian_amd import _lib, query
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=gpu_device)
    K = int(_lib.lib().ogs_query_max_leaves()) + 1
    with pytest.raises(ValueError, match="leaves"):
        query.select_leaves_by_text(z(1, 2), z(K, 2), z(K), z(K + 1, 6), 1.0)
    with pytest.raises(ValueError, match="classes"):
        query.segmentation_metrics(z(4, dt=torch.int64), z(4, dt=torch.int64), int(_lib.lib().ogs_query_max_classes()) + 1)
    tmp = z(4096, dt=torch.uint8)
    rc = _lib.lib().ogs_query_split_count(10, _lib.ptr(z(10, dt=torch.int64)), 4, _lib.ptr(z(4, dt=torch.int64)), None, 65,
                                          _lib.ptr(tmp), torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"at most 64" in _lib.lib().ogs_last_error()


# ---- all queries of a view against one render() per query -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_scene(gpu_device):
    from tests.golden import render_cases as rc
    s, _, pipe = _scene_model()
    model = rc.TinyModel(s["params"], gpu_device, requires_grad=False)
    cpu_model = rc.TinyModel(s["params"], "cpu", requires_grad=False)
    return s, model, cpu_model, pipe, s["cam"].to(gpu_device), s["bg"].to(gpu_device), s["leaf"].to(gpu_device)


@pytest.mark.parametrize("flags", [dict(), dict(post_process=False), dict(better_vis=False), dict(seg_rgb=False),
                                   dict(better_vis=False, post_process=False, seg_rgb=False)],
                         ids=["default", "no_knn", "no_better_vis", "features", "plain_features"])
@pytest.mark.parametrize("masked", [True, False])
def test_render_queries_equals_one_render_per_query(gpu_scene, gpu_device, masked, flags):
    from opengaussian_amd import query
    from opengaussian_amd.renderer import render
    s, model, cpu_model, pipe, cam, bg, leaf = gpu_scene
    kw = dict(better_vis=True, seg_rgb=True, post_process=True)
    kw.update(flags)
    pre = s["pre_mask"].to(gpu_device) if masked else None
    sels = [torch.tensor(sel, dtype=torch.int64, device=gpu_device) for sel in qc.SCENE_SELECTIONS]
    with torch.no_grad():
        out = query.render_queries(cam, model, pipe, bg, 0, leaf, sels, pre_mask=pre, root_num=4, leaf_num=3, **kw)
        viewed = None
        for q, sel in enumerate(sels):
            if sel.numel() == 0:                                        # render() cannot take an empty selection: nothing drawn
                assert out.images[q] is None and out.silhouettes[q] is None and not out.kept[q] and out.counts[q] == 0
                continue
            ref = render(cam, model, pipe, bg, 0, rescale=False, leaf_cluster_idx=leaf, selected_leaf_id=sel,
                         render_feat_map=False, render_cluster=False, pre_mask=pre, root_num=4, leaf_num=3, **kw)
            viewed = ref["radii"] > 0
            if len(ref["leaf_clusters_imgs"]) == 0:
                assert out.images[q] is None and out.silhouettes[q] is None and not out.kept[q], q
                continue
            assert out.kept[q] and len(ref["leaf_clusters_imgs"]) == 1
            want = ref["leaf_clusters_imgs"][0][:3] if kw["seg_rgb"] else ref["leaf_clusters_imgs"][0]
            assert torch.equal(out.images[q], want), (q, float((out.images[q] - want).abs().max()))
            assert torch.equal(out.silhouettes[q], ref["leaf_cluster_silhouettes"][0:1]), q
    want_sets = _expected_sets(s, cpu_model, viewed.cpu().numpy(), s["pre_mask"] if masked else None, kw["better_vis"],
                               kw["post_process"])
    assert [r is not None for r, _ in want_sets] == out.kept and [n for _, n in want_sets] == out.counts
    # the pair form of select_leaves_by_text gives the same
    selected = torch.full((6, 3), 5, dtype=torch.int32, device=gpu_device)
    for q, sel in enumerate(qc.SCENE_SELECTIONS):
        selected[q, :len(sel)] = torch.tensor(sel, dtype=torch.int32)
    count = torch.tensor([len(sel) for sel in qc.SCENE_SELECTIONS], dtype=torch.int32, device=gpu_device)
    with torch.no_grad():
        again = query.render_queries(cam, model, pipe, bg, 0, leaf, (selected, count), pre_mask=pre, root_num=4, leaf_num=3, **kw)
    assert again.kept == out.kept and again.counts == out.counts
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(again.images, out.images))
