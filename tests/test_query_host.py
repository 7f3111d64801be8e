"""CPU: the NumPy restatements of the open-vocabulary query step against goldens made by the reference's own code
(tests/golden/make_query_golden.py), the tie rules, the host glue of opengaussian_amd.query around a stand-in for the kernels,
and the margin conditions of the inputs tests/test_38_query_gpu.py compares exactly on the GPU."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import knn_restatement as kr
from tests import query_cases as qc
from tests import query_restatement as qr
from tests.test_knn_host import _FakeLib as _KnnFakeLib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def gold_case(gold, seed):
    k = f"s{seed}"
    return dict(text=qc.unpack_features(gold[f"{k}/text_q"]), leaf=qc.unpack_features(gold[f"{k}/leaf_q"]),
                occu=gold[f"{k}/occu"].astype(np.int64), centers=gold[f"{k}/centers"], leaf_num=np.float32(qc.GOLD_K / qc.GOLD_ROOTS),
                leaf_ind=gold[f"{k}/leaf_ind"].astype(np.int64), gt=gold[f"{k}/gt"].astype(np.int64), ignore=gold[f"{k}/ignore"],
                sim5=gold[f"{k}/sim5"], selected=gold[f"{k}/selected"], count=gold[f"{k}/count"],
                pred=gold[f"{k}/pred"].astype(np.int64))


def same_scalars(a, b):
    return all((math.isnan(x) and math.isnan(y)) or x == y for x, y in zip(a, b))


# ---- restatements against the reference's results ----------------------------------------------------------------------------
def test_stored_inputs_are_the_seeded_ones_and_have_their_margins(gold):
    top = int(gold["top"])
    for seed in gold["seeds"]:
        g, c = gold_case(gold, seed), qc.text_case(int(seed))
        assert np.array_equal(g["text"], c["text"]) and np.array_equal(g["leaf"], c["leaf"]) and np.array_equal(g["occu"], c["occu"])
        s5 = qr.similarity(g["text"], g["leaf"], g["occu"], 5)
        first, cut = qr.row_margins(s5, top)
        assert first.min() > qc.MARGIN and cut.min() > qc.MARGIN
        assert qr.rank_margin(s5, top) > qc.ORDER_MARGIN
        assert qr.merge_margin(s5, g["centers"], g["leaf_num"], top) > qc.MARGIN
        col = -np.sort(-qr.similarity(g["text"], g["leaf"], g["occu"], 2), axis=0)
        assert (col[0] - col[1])[g["occu"] >= 2].min() > qc.MARGIN
        assert (g["occu"] < 2).any() and (g["leaf_ind"] == qc.GOLD_K).any()             # zeroed leaves, ids clamped at K - 1


def test_restatement_selection_equals_the_reference_block(gold):
    for seed in gold["seeds"]:
        g = gold_case(gold, seed)
        sim, sel, cnt = qr.select_leaves(g["text"], g["leaf"], g["occu"], g["centers"], g["leaf_num"], top=int(gold["top"]))
        assert np.array_equal(sel, g["selected"]) and np.array_equal(cnt, g["count"]), seed
        assert np.abs(sim - g["sim5"]).max() < 1e-6              # the reference's fp32 matmul against fp64


def test_restatement_classes_and_metrics_equal_the_reference(gold):
    for seed in gold["seeds"]:
        g = gold_case(gold, seed)
        pred, _, _ = qr.classify(g["text"], g["leaf"], g["occu"], g["leaf_ind"])
        assert np.array_equal(pred, g["pred"]), seed
        C = qc.GOLD_Q + 1
        for tag, ign in (("plain", None), ("ignore", g["ignore"])):
            conf = qr.confusion(g["gt"], pred, C, ign)
            assert conf.sum() == len(pred)
            want_ious, want = gold[f"s{seed}/{tag}/ious"], gold[f"s{seed}/{tag}/scalars"]
            ious, *scalars = qr.metrics(conf)
            assert ious.dtype == np.float32 and np.array_equal(ious, want_ious), (seed, tag)
            assert same_scalars(scalars, want), (seed, tag, scalars, want)
            gt = g["gt"].copy()
            if ign is not None:
                gt[ign] = 0
            loop_ious, *loop_scalars = qr.reference_loop_metrics(gt, pred, C)               # the loop and the table agree
            assert np.array_equal(loop_ious, want_ious) and same_scalars(loop_scalars, want)
            from opengaussian_amd import query
            t_ious, *t_scalars = query.metrics_from_confusion(torch.from_numpy(conf))        # the product's own half
            assert t_ious.dtype == torch.float32 and np.array_equal(t_ious.numpy(), want_ious)
            assert same_scalars(t_scalars, want)


def test_metrics_of_an_unlabelled_scene_are_nan(gold):
    from opengaussian_amd import query
    pred = np.random.default_rng(0).integers(1, 20, 300)
    conf = qr.confusion(np.zeros(300, np.int64), pred, 20)
    assert conf[0, 0] == 300 and conf.sum() == 300
    for ious, *scalars in (qr.metrics(conf), query.metrics_from_confusion(torch.from_numpy(conf))):
        assert np.array_equal(np.asarray(ious), gold["allzero/ious"]) and same_scalars(scalars, gold["allzero/scalars"])
        assert all(math.isnan(s) for s in scalars)


# ---- the tie rules ----------------------------------------------------------------------------------------------------------
def test_tie_rules():
    assert list(qr.rank_desc([0.5, 0.7, 0.7, 0.1, 0.7], 3)) == [1, 2, 4]
    c = qc.text_case(6)
    far = np.zeros_like(c["centers"])
    sim, sel, cnt = qr.select_leaves(c["text"], c["leaf"], np.zeros(qc.GOLD_K), far, np.float32(60))    # every leaf zeroed
    assert not sim.any() and (cnt == 10).all() and (sel == np.arange(10)).all()       # best 0, candidates 1 .. top - 1
    _, sel, cnt = qr.select_leaves(c["text"], c["leaf"], np.zeros(qc.GOLD_K), far, c["leaf_num"])
    assert (cnt == 5).all() and (sel[:, :5] == np.arange(5)).all()                    # ... of which `c - 0 < 5` admits four
    _, sel, cnt = qr.select_leaves(c["text"], c["leaf"], np.zeros(qc.GOLD_K), far + np.arange(61)[:, None], c["leaf_num"])
    assert (cnt == 1).all() and (sel[:, 0] == 0).all() and (sel[:, 1:] == -1).all()   # ... none of which is near
    small = qc.text_case(6, K=7, roots=1)
    _, sel, cnt = qr.select_leaves(small["text"], small["leaf"], None, np.zeros((8, 6), np.float32), np.float32(7.0))
    assert (cnt == 7).all() and all(sorted(r[:7]) == list(range(7)) for r in sel) and (sel[:, 7:] == -1).all()   # K < top
    # the signed rule: a candidate far ABOVE the best is refused, any candidate below it passes
    sim = np.array([0.1, 0.9, 0.2, 0.3, 0.8])
    ids, _ = qr.select_row(sim, np.zeros((5, 6), np.float32), leaf_num=2.0, top=5)
    assert ids == [1, 2, 0]                                  # 4 - 1 = 3 is not below 2; 3 - 1 = 2 neither; 2 - 1 and 0 - 1 are


def test_planted_cases_have_their_margins():
    for K, D in ((640, 512), (8192, 513)):
        c = qc.planted_case(K, D, 21)
        s = qr.similarity(c["text"], c["leaf"], c["occu"], 5)
        first, cut = qr.row_margins(s[1:], 10)                   # row 0 is the zero text: exact ties, exact zeros
        assert first.min() > 0.04 and cut.min() > 0.1 and qr.rank_margin(s[1:], 10) > 0.04
        assert qr.merge_margin(s, c["centers"], c["leaf_num"]) > 0.3
        assert not s[0].any() and not s[:, [3, 5]].any()
        _, sel, cnt = qr.select_leaves(c["text"], c["leaf"], c["occu"], c["centers"], c["leaf_num"])
        assert (cnt[1:] == 6).all() and (sel[1:, :6] == c["slots"][1:, [0, 1, 3, 5, 7, 9]]).all() and cnt[0] == 1


@pytest.mark.parametrize("K", qc.SHAPE_KS)
def test_shape_cases_leave_rows_to_compare_exactly(K):
    """What tests/test_38_query_gpu.py::test_similarity_and_selection_shapes compares exactly is not an empty set: per (K, D)
    the rows whose decisions are clear (margins, or ties at an exact zero)."""
    zeroed = 0
    for D in qc.SHAPE_DS:
        rows = 0
        for Q in qc.SHAPE_QS:
            c = qc.shape_case(K, D, Q)
            zeroed += int((c["occu"] < 5).sum())
            s =qr.similarity(c["text"], c["leaf"], c["occu"], 5)
            ok = qc.shape_decided(c, s)
            assert Q == 1 or (ok[2] and not s[2].any())                                 # the zero text row is one of them
            rows += int(ok.sum())
        assert rows >= (qc.SHAPE_MIN_EXACT if D > 1 else 1), (K, D, rows)
    assert K == 1 or zeroed > 0                                                         # zeroed leaves among the inputs


def test_decided_rows_rules():
    z, cen = np.zeros(4, bool), np.zeros((5, 6), np.float32)
    rule = lambda sim, zeroed: bool(qr.decided_rows(np.array([sim]), zeroed, cen, 4.0, 2, qc.MARGIN, qc.ORDER_MARGIN)[0])
    assert rule([0.9, 0.5, 0.2, 0.1], z)
    assert not rule([0.9, 0.5, 0.5, 0.1], z)                                            # a tie at the cut between live leaves
    assert not rule([0.9, 0.9 - 5e-4, 0.2, 0.1], z)                                     # the best by less than the margin
    assert rule([0.9, 0.0, 0.0, -0.1], np.array([0, 1, 1, 0], bool))                    # a tie of two zeroed leaves: exact
    assert not rule([0.9, 0.0, 0.0, -0.1], np.array([0, 1, 0, 0], bool))                # ... of which one is live: not
    assert not rule([0.9, 1e-5, 0.0, -0.1], np.array([0, 0, 1, 0], bool))               # a live leaf too near a zeroed one
    assert rule([0.0, 0.0, 0.0, 0.0], z)                                                # a zero text row
    far = np.zeros((5, 6), np.float32)
    far[1, 0] = 0.9004                                                                  # a merge decided within the margin
    assert not qr.decided_rows(np.array([[0.9, 0.5, 0.2, 0.1]]), z, far, 4.0, 2, qc.MARGIN, qc.ORDER_MARGIN)[0]


def test_small_case_has_its_rank_margins():
    c = qc.small_case()
    s = qr.similarity(c["text"], c["leaf"], c["occu"], 5)
    assert qc.shape_decided(c, s).all() and (qr.select_leaves(c["text"], c["leaf"], c["occu"], c["centers"], c["leaf_num"])[2] == 7).all()


def test_split_restatement_and_cases():
    for Q in (1, 2, 33, 64):
        c = qc.split_case(3 * 1024 + 17, Q, holes=Q > 2)
        member = qr.membership(c["leaf_ind"], c["words"], Q)
        assert not member[(c["leaf_ind"] == -1) | (c["leaf_ind"] == c["K"]) | (c["leaf_ind"] == 0)].any()
        assert (c["leaf_ind"] == -1).any() and (c["leaf_ind"] == c["K"]).any()
        if Q > 2:
            assert not member[:, [0, Q // 2, Q - 1]].any() and member[c["leaf_ind"] == 1].sum(1).min() == Q - 3
        else:
            assert member[c["leaf_ind"] == 1].all()          # rows in all Q groups
        begin, rows, counts = qr.multi_split(c["leaf_ind"], c["words"], Q, c["row_ok"], c["group_keep"])
        assert begin[-1] == len(rows) and (counts >= np.diff(begin)).all()
        for q in range(Q):
            seg = rows[begin[q]:begin[q + 1]]
            assert (np.diff(seg) > 0).all() and (len(seg) == 0 or c["group_keep"][q])


# ---- the host glue of opengaussian_amd.query around a CPU stand-in for the kernels -----------------------------------------
def _arr(p, ct, m):
    return np.ctypeslib.as_array((ct * max(int(m), 1)).from_address(p))[:int(m)]


class _FakeLib(_KnnFakeLib):
    """The ogs_query_* entry points on host memory through the same pointers, computed by the restatement."""
    BLOCK = 1024

    def __init__(self):
        super().__init__()
        self.splits, self.scatter_capacity = 0, []

    ogs_query_max_leaves = staticmethod(lambda: 8192)
    ogs_query_max_top = staticmethod(lambda: 64)
    ogs_query_max_classes = staticmethod(lambda: 64)
    ogs_query_split_block = staticmethod(lambda: 1024)
    ogs_check_async_status = staticmethod(lambda: 0)

    def ogs_query_split_tmp_bytes(self, n, Q):
        return 8 * Q * 2 + 256                                # [counts before keep | begin]: the stand-in's own layout

    def ogs_query_select(self, Q, K, D, text, leaf, valid, centers, cd, leaf_num, max_dist, top, sim, selected, count, stream):
        t, l = _arr(text, ctypes.c_float, Q * D).reshape(Q, D), _arr(leaf, ctypes.c_float, K * D).reshape(K, D)
        occu = _arr(valid, ctypes.c_uint8, K) if valid else np.ones(K)
        s = qr.similarity(t, l, occu, 1)
        _arr(sim, ctypes.c_float, Q * K).reshape(Q, K)[:] = s
        if top > 0:
            c = _arr(centers, ctypes.c_float, K * cd).reshape(K, cd)
            _, sel, cnt = qr.select_leaves(t, l, occu, c, leaf_num, 1, top, max_dist)
            _arr(selected, ctypes.c_int32, Q * top).reshape(Q, top)[:] = sel
            _arr(count, ctypes.c_int32, Q)[:] = cnt
        return 0

    def ogs_query_classify(self, n, leaf_ind, K, T, sim, cls, pred, stream):
        s = _arr(sim, ctypes.c_float, T * K).reshape(T, K)
        c = np.argmax(s, axis=0)
        _arr(cls, ctypes.c_int32, K)[:] = c
        if n:
            _arr(pred, ctypes.c_int64, n)[:] = c[np.clip(_arr(leaf_ind, ctypes.c_int64, n), 0, K - 1)] + 1
        return 0

    def ogs_query_confusion(self, n, gt, pred, ignore, C, conf, stream):
        g, r = _arr(gt, ctypes.c_int64, n), _arr(pred, ctypes.c_int64, n)
        _arr(conf, ctypes.c_int64, C * C)[:] = qr.confusion(g, r, C, _arr(ignore, ctypes.c_uint8, n) if ignore else None).ravel()
        return 0

    def _member(self, n, leaf_ind, K, words, row_ok, Q, keep):
        return qr.membership(_arr(leaf_ind, ctypes.c_int64, n), _arr(words, ctypes.c_uint64, K), Q,
                             _arr(row_ok, ctypes.c_uint8, n) if row_ok else None, _arr(keep, ctypes.c_uint8, Q) if keep else None)

    def ogs_query_split_count(self, n, leaf_ind, K, words, row_ok, Q, tmp, stream):
        assert Q <= 64
        self.splits += 1
        _arr(tmp, ctypes.c_int64, 2 * Q)[:Q] = self._member(n, leaf_ind, K, words, row_ok, Q, None).sum(0)
        return 0

    def ogs_query_split_scan(self, n, Q, keep, tmp, begin, counts, stream):
        raw = _arr(tmp, ctypes.c_int64, 2 * Q)[:Q]
        kept = raw * (_arr(keep, ctypes.c_uint8, Q) != 0) if keep else raw
        _arr(begin, ctypes.c_int32, Q + 1)[:] = np.concatenate([[0], np.cumsum(kept)])
        _arr(counts, ctypes.c_int32, Q)[:] = raw
        return 0

    def ogs_query_split_scatter(self, n, leaf_ind, K, words, row_ok, Q, keep, tmp, rows, capacity, stream):
        member = self._member(n, leaf_ind, K, words, row_ok, Q, keep)
        out = np.concatenate([np.nonzero(member[:, q])[0] for q in range(Q)])
        assert len(out) == capacity                           # the wrapper sizes the rows by the counts it read
        self.scatter_capacity.append(int(capacity))
        _arr(rows, ctypes.c_int64, capacity)[:] = out
        return 0


@pytest.fixture
def cpu_query(monkeypatch):
    from opengaussian_amd import knn, query
    fake = _FakeLib()
    for mod in (query, knn):
        monkeypatch.setattr(mod, "_need_gpu", lambda t, name: None)
        monkeypatch.setattr(mod, "_stream", lambda: 0)
    monkeypatch.setattr(query._lib, "lib", lambda: fake)
    return query, fake


def test_glue_select_classify_metrics_equal_the_goldens(cpu_query, gold):
    query, _ = cpu_query
    g = gold_case(gold, gold["seeds"][0])
    T = torch.from_numpy
    sim, sel, cnt = query.select_leaves_by_text(T(g["text"]), T(g["leaf"]), T(g["occu"]), T(g["centers"]), float(g["leaf_num"]))
    assert sel.dtype == torch.int32 and np.array_equal(sel.numpy(), g["selected"]) and np.array_equal(cnt.numpy(), g["count"])
    assert np.abs(sim.numpy() - g["sim5"]).max() < 1e-6
    pred = query.classify_points(T(g["text"]), T(g["leaf"]), T(g["occu"]), T(g["leaf_ind"]))
    assert pred.dtype == torch.int64 and np.array_equal(pred.numpy(), g["pred"])
    ious, *scalars = query.segmentation_metrics(T(g["gt"]), pred, qc.GOLD_Q + 1, ignore=T(g["ignore"]))
    seed = gold["seeds"][0]
    assert np.array_equal(ious.numpy(), gold[f"s{seed}/ignore/ious"]) and same_scalars(scalars, gold[f"s{seed}/ignore/scalars"])


def test_glue_value_errors(cpu_query):
    query, _ = cpu_query
    f = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError, match=r"\[Q, D\]"):
        query.select_leaves_by_text(f(3, 8), f(5, 9), f(5), f(6, 6), 1.0)
    with pytest.raises(ValueError, match="occu_count"):
        query.select_leaves_by_text(f(3, 8), f(5, 8), f(4), f(6, 6), 1.0)
    with pytest.raises(ValueError, match="leaf_centers"):
        query.select_leaves_by_text(f(3, 8), f(5, 8), f(5), f(4, 6), 1.0)
    with pytest.raises(ValueError, match="8192"):
        query.select_leaves_by_text(f(1, 2), f(8193, 2), f(8193), f(8194, 6), 1.0)
    with pytest.raises(ValueError, match="top"):
        query.select_leaves_by_text(f(1, 2), f(5, 2), f(5), f(6, 6), 1.0, top=65)
    gt = torch.tensor([0, 1, 2, 3])
    for bad_gt, bad_pred in ((gt, gt + 1), (gt - 1, gt), (gt + 1, gt)):
        with pytest.raises(ValueError, match="outside"):
            query.segmentation_metrics(bad_gt, bad_pred, 4)
    with pytest.raises(ValueError, match="alike"):
        query.segmentation_metrics(gt, gt[:3], 4)
    # what the reference overwrites is not range-checked: a prediction at an unlabelled point, a label under `ignore`
    held = query.confusion_table(torch.tensor([0, 1, 99, 1]), torch.tensor([-1, 1, 4, 0]), 4, torch.tensor([False, False, True, False]))
    assert np.array_equal(held.numpy(), qr.confusion([0, 1, 0, 1], [0, 1, 0, 0], 4))
    with pytest.raises(ValueError, match="outside"):
        query.confusion_table(torch.tensor([0, 1, 99, 1]), torch.tensor([-1, 1, 4, 0]), 4)
    with pytest.raises(ValueError, match="classes"):
        query.segmentation_metrics(gt, gt, 65)
    with pytest.raises(ValueError, match="leaf_groups"):
        query.multi_split(gt, torch.zeros(5, 1, dtype=torch.int64), 65)
    with pytest.raises(ValueError, match="row_ok"):
        query.multi_split(gt, torch.zeros(5, dtype=torch.int64), 3, row_ok=torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError, match="1-D"):
        query.leaf_group_table([torch.zeros(2, 2)], 5, "cpu")


def _words_i64(words):
    return torch.from_numpy(np.asarray(words, np.uint64).view(np.int64).copy())


def test_glue_multi_split_chunks_above_64_groups(cpu_query):
    query, fake = cpu_query
    rng = np.random.default_rng(1)
    sels = [rng.choice(30, size=int(rng.integers(0, 4)), replace=False) for _ in range(150)]
    table, Q = query.leaf_group_table([torch.from_numpy(s) for s in sels], 30, "cpu")
    assert Q == 150 and table.shape == (30, 3) and table.dtype == torch.int64
    want = np.zeros((30, 150), bool)
    for q, s in enumerate(sels):
        want[s, q] = True
    bits = (table.numpy().view(np.uint64)[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    assert np.array_equal(bits.reshape(30, 192)[:, :150].astype(bool), want) and not bits.reshape(30, 192)[:, 150:].any()
    leaf_ind = rng.integers(-1, 31, 2500)
    row_ok, keep = rng.random(2500) < 0.8, rng.random(150) < 0.7
    begin, rows, counts = query.multi_split(torch.from_numpy(leaf_ind), table, 150, torch.from_numpy(row_ok), torch.from_numpy(keep))
    assert fake.splits == 3 and begin.shape == (151,)
    inside = (leaf_ind >= 0) & (leaf_ind < 30)
    for q in range(150):
        m = inside & np.isin(leaf_ind, sels[q]) & row_ok
        assert counts[q] == m.sum()
        assert np.array_equal(rows[begin[q]:begin[q + 1]].numpy(), np.nonzero(m)[0] if keep[q] else []), q


# ---- render_queries around stand-ins for the kernels and the rasterizer passes ----------------------------------------------
def _scene_model():
    from tests.golden import render_cases as rc
    s = qc.query_scene()
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    return s, rc.TinyModel(s["params"], "cpu", requires_grad=False), pipe


def _oracle_viewed(s, model):
    from oracle import raster_oracle as ro
    cam = s["cam"]
    g = ro.preprocess(model.get_xyz.numpy(), model.get_opacity.numpy(), cam.world_view_transform.numpy(),
                      cam.full_proj_transform.numpy(), cam.camera_center.numpy(), cam.image_width, cam.image_height,
                      math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), scales=model.get_scaling.numpy(),
                      rotations=model.get_rotation.numpy(), colors_precomp=np.zeros((len(model.get_xyz), 3), np.float32))
    return g.radii > 0


def _expected_sets(s, model, viewed, pre_mask, better_vis, post_process):
    """rows render(selected_leaf_id=...) draws for every selection of the scene (None: nothing drawn), and the row counts
    at the last rule -- the sequence of renderer.py:313-349 in NumPy"""
    leaf, xyz = s["leaf"].numpy(), model.get_xyz.numpy()
    small = (model.get_scaling.numpy() < 0.1).all(1)
    out = []
    for sel in qc.SCENE_SELECTIONS:
        m = np.isin(leaf, sel) & viewed
        if pre_mask is not None:
            m &= pre_mask.numpy()
        if better_vis:
            m &= small
            if m.sum() < 100:
                m[:] = False
        rows = np.nonzero(m)[0]
        if post_process and len(rows):
            rows = rows[kr.outlier_stats(xyz[rows])["mask"]]
        out.append((rows if len(rows) >= 10 else None, len(rows)))
    return out


@pytest.fixture(scope="module")
def scene():
    s, model, pipe = _scene_model()
    return s, model, pipe, _oracle_viewed(s, model)


def test_render_scene_has_what_its_queries_need_and_the_knn_margins(scene):
    s, model, pipe, viewed = scene
    leaf, xyz = s["leaf"].numpy(), model.get_xyz.numpy()
    small = (model.get_scaling.numpy() < 0.1).all(1)
    for pre in (None, s["pre_mask"]):
        ok = viewed & small & (True if pre is None else pre.numpy())
        n10, n11 = (ok & (leaf == 10)).sum(), (ok & (leaf == 11)).sum()
        assert 10 <= n10 < 100 and n10 == ((leaf == 10) & viewed).sum()              # only the `< 100` rule drops leaf 10
        assert n11 == 11 == (leaf == 11).sum()
        assert all((ok & np.isin(leaf, sel)).sum() >= 200 for sel in ([4, 7], [4, 5], [12, 9]))
        for better_vis in (True, False):
            sets = _expected_sets(s, model, viewed, pre, better_vis, True)
            assert [r is not None for r, _ in sets] == [True, True, not better_vis, False, False, True]
            assert better_vis or 0 < sets[4][1] < 10                                # leaf 11: under 10 only after the kNN filter
            for sel in qc.SCENE_SELECTIONS:                                          # no row near its threshold
                m = np.isin(leaf, sel) & viewed & (small if better_vis else True) & (True if pre is None else pre.numpy())
                if m.sum() > 1:
                    assert kr.outlier_stats(xyz[m])["margin"].min() > 1e-6, (sel, better_vis)
    assert (leaf == 12).sum() > 50 and (~viewed).sum() > 20


@pytest.fixture
def cpu_render(cpu_query, monkeypatch, scene):
    query, fake = cpu_query
    s, model, pipe, viewed = scene
    monkeypatch.setattr(query, "_visible", lambda *a, **k: torch.from_numpy(viewed))

    def fake_groups(local, num, settings, means3D, opacity, scales, rotations, cov3D, shs, colors):
        # an "image" that identifies the drawn rows IN ORDER: the first coordinate of each, padded
        imgs = []
        for g in range(num):
            x = means3D[local == g][:, 0]
            imgs.append(torch.cat((x, torch.full((3000 - len(x),), float("nan")))))
        return imgs, [torch.tensor([float((local == g).sum())]) for g in range(num)]
    monkeypatch.setattr(query, "_render_groups", fake_groups)
    return query, fake, s, model, pipe, viewed


@pytest.mark.parametrize("better_vis", [True, False])
@pytest.mark.parametrize("post_process", [True, False])
@pytest.mark.parametrize("masked", [True, False])
def test_glue_render_queries_rules_and_forms(cpu_render, better_vis, post_process, masked):
    query, fake, s, model, pipe, viewed = cpu_render
    pre = s["pre_mask"] if masked else None
    want = _expected_sets(s, model, viewed, pre, better_vis, post_process)
    as_list = [torch.tensor(sel, dtype=torch.int64) for sel in qc.SCENE_SELECTIONS]
    selected = torch.full((6, 4), 7, dtype=torch.int32)                                # the pair form: junk past count
    count = torch.tensor([len(sel) for sel in qc.SCENE_SELECTIONS], dtype=torch.int32)
    for q, sel in enumerate(qc.SCENE_SELECTIONS):
        selected[q, :len(sel)] = torch.tensor(sel, dtype=torch.int32)
    xyz = model.get_xyz.numpy()
    for form in (as_list, (selected, count)):
        out = query.render_queries(s["cam"], model, pipe, s["bg"], 0, s["leaf"], form, pre_mask=pre, better_vis=better_vis,
                                   post_process=post_process, root_num=4, leaf_num=3)
        for q, (rows, n) in enumerate(want):
            assert out.kept[q] == (rows is not None) and (out.images[q] is None) == (rows is None), q
            assert out.counts[q] == n, (q, out.counts[q], n)
            if rows is not None:
                got = out.images[q].numpy()
                assert np.array_equal(got[:len(rows)], xyz[rows, 0]) and np.isnan(got[len(rows):]).all()
                assert float(out.silhouettes[q]) == len(rows)
    assert fake.calls == (2 if post_process else 0)                                    # ONE kNN launch per call


def test_glue_render_queries_chunks_above_64_queries(cpu_render, monkeypatch):
    query, fake, s, model, pipe, viewed = cpu_render
    from opengaussian_amd import renderer
    monkeypatch.setattr(renderer, "GROUPS_PER_PASS", 5)                                # several passes per split as well
    sels = [torch.tensor(qc.SCENE_SELECTIONS[q % 6], dtype=torch.int64) for q in range(70)]
    out = query.render_queries(s["cam"], model, pipe, s["bg"], 0, s["leaf"], sels, pre_mask=s["pre_mask"], root_num=4, leaf_num=3)
    want = _expected_sets(s, model, viewed, s["pre_mask"], True, True)
    assert fake.splits == 2 and fake.calls == 2 and len(out.images) == 70
    for q in range(70):
        rows, n = want[q % 6]
        assert out.kept[q] == (rows is not None) and out.counts[q] == n
        if rows is not None:
            assert np.array_equal(out.images[q].numpy()[:len(rows)], model.get_xyz.numpy()[rows, 0])
    empty = query.render_queries(s["cam"], model, pipe, s["bg"], 0, s["leaf"], [], root_num=4, leaf_num=3)
    assert empty.images == [] and empty.kept == []


def test_cpu_tensors_are_refused():
    from opengaussian_amd import query
    f = torch.zeros
    calls = (lambda: query.select_leaves_by_text(f(2, 4), f(3, 4), f(3), f(4, 6), 1.0),
             lambda: query.classify_points(f(2, 4), f(3, 4), f(3), f(5, dtype=torch.int64)),
             lambda: query.segmentation_metrics(f(5, dtype=torch.int64), f(5, dtype=torch.int64), 3),
             lambda: query.multi_split(f(5, dtype=torch.int64), f(3, dtype=torch.int64), 2))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    s, model, pipe = _scene_model()
    with pytest.raises(RuntimeError, match="no CPU path"):
        query.render_queries(s["cam"], model, pipe, s["bg"], 0, s["leaf"], [torch.tensor([1])])
