"""CPU: the label-votes restatement against a direct loop, the conditions the cases must meet (from the oracle alone) before the
GPU test may rely on them, the table helpers of opengaussian_amd/query.py on hand-made integer tables, argument validation."""
import numpy as np
import pytest
import torch

from tests import label_votes_cases as vc
from tests import label_votes_restatement as vr

Q = 1 << 32        # units per unit of blend weight


def _hooks():
    from opengaussian_amd import _lib
    return int(_lib.lib().ogs_label_votes_fold_columns()), int(_lib.lib().ogs_label_votes_quadrant_capacity())


def test_hooks_describe_a_quadrant():
    fold, cap = _hooks()
    assert 1 <= fold <= cap <= 64
    assert vc.many_counts(fold, cap)[-1] == 64


def test_restatement_equals_a_direct_loop():
    """the autograd route is the table of the definition: a per-pixel, per-entry loop over w = alpha * T on a tiny case"""
    from tests import label_map_cases as lmc
    c = lmc.scene_case(300, 5)
    sc = type(c["sc"])(*[getattr(c["sc"], f)[:60].contiguous() for f in ("means3D", "scales", "rotations", "opacities", "shs", "ins_feat")])
    img, L = vc.label_image("noise", 5)
    a = vr.vote_table(sc, c["cam"], img.numpy(), L)
    b = vr.vote_table_by_loops(sc, c["cam"], img.numpy(), L)
    assert a.shape == (60, L + 1) and a.max() > 0.5
    assert np.abs(a - b).max() <= 1e-12 * a.max()
    # rows: index_add, out-of-range rows dropped
    rows = np.array([i % 4 - 1 for i in range(60)])
    rt = vr.rows_table(a, rows, 2)
    assert np.allclose(rt[0], a[rows == 0].sum(0)) and np.allclose(rt[1], a[rows == 1].sum(0))


@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_case_conditions(name):
    fold, cap = _hooks()
    c = vc.case(name, fold, cap)
    t = vc.oracle(name, fold, cap)
    P, L = c["sc"].means3D.shape[0], c["L"]
    assert t.shape == (P, L + 1) and (t >= 0).all() and t.max() > 0.5
    lab = vc.clamp_labels(c["image"].numpy(), L)
    kind = name.split("_", 1)[1]
    if kind == "null" or kind == "L0":
        assert not t[:, :L].any() and t[:, L].any()
    if kind == "blocks8":
        assert all(len(np.unique(lab[y:y + 8, x:x + 8])) == 1 for y in range(0, vc.H, 8) for x in range(0, vc.W, 8))
    if kind == "blocks4":
        assert all(len(np.unique(lab[y:y + 8, x:x + 8])) == 4 for y in range(0, vc.H, 8) for x in range(0, vc.W, 8))
    if kind.startswith("noise"):
        img = c["image"].numpy()
        assert 0.25 < (img == -1).mean() < 0.42 and (img >= L).sum() >= 2 and (img < -1).sum() == 2
    if c["many"]:
        quad = lab[vc.QUAD_Y0:vc.QUAD_Y0 + 8, vc.QUAD_X0:vc.QUAD_X0 + 8]
        assert len(np.unique(quad)) == c["many"]
        # every label of the quadrant, found nowhere else in the image, receives weight: a column block that is skipped shows
        outside = lab.copy()
        outside[vc.QUAD_Y0:vc.QUAD_Y0 + 8, vc.QUAD_X0:vc.QUAD_X0 + 8] = -1
        only_here = [l for l in np.unique(quad) if not (outside == l).any()]
        assert len(only_here) >= c["many"] - 2
        assert (t[:, only_here].sum(0) > 1e-3).all()
    if name.startswith("wide"):
        small = t[:300].max()
        assert t.max() > 5 * small, (t.max(), small)        # the wide Gaussians own the table's maximum


@pytest.mark.parametrize("name", vc.LABEL_CHECK)
def test_decided_rows(name):
    """at least 90 % of the voted rows are decided, so the GPU label check never sets more than 10 % aside"""
    fold, cap = _hooks()
    t = vc.oracle(name, fold, cap)
    label, weight, second, total = vr.labels_from_votes(t)
    voted = label >= 0
    decided = voted & (weight - second > vc.DECIDED * t.max())
    share = decided.sum() / max(int(voted.sum()), 1)
    print(name, "voted", int(voted.sum()), "decided", int(decided.sum()), "share", round(float(share), 3))
    assert voted.sum() > 0 and share >= 0.9, share


def test_fp32_graph_is_close_to_float64():
    fold, cap = _hooks()
    a, b = vc.oracle("P300_noise5", fold, cap), vc.oracle_fp32("P300_noise5", fold, cap)
    assert np.abs(a - b).max() <= 1e-5 * a.max()


# ---- the fixed-point helpers and the table helpers ---------------------------------------------------------------------------------
def test_votes_as_float():
    from opengaussian_amd import query
    t = torch.tensor([[0, 1, Q], [3 * Q // 2, -Q, 1 << 52]], dtype=torch.int64)
    f = query.votes_as_float(t)
    assert f.dtype == torch.float64 and f.tolist() == [[0.0, 2.0 ** -32, 1.0], [1.5, -1.0, 2.0 ** 20]]
    assert query.VOTE_QUANTUM == 2.0 ** -32
    with pytest.raises(ValueError):
        query.votes_as_float(t.to(torch.int32))


def test_labels_from_votes_rules():
    from opengaussian_amd import query
    t = torch.tensor([[5 * Q, 2 * Q, 0, 1 * Q],            # label 0
                      [2 * Q, 7 * Q, 7 * Q, 0],            # an exact tie: the lowest label, second = the other
                      [0, 0, 0, 9 * Q],                    # unlabelled weight only
                      [0, 0, 0, 0],                        # empty
                      [Q + 1, Q, Q - 1, 0],                # the tie is decided on the integers: one unit apart
                      [0, 0, Q // 2, 3 * Q // 2],          # weight 0.5, share 0.25
                      [(1 << 60) + 1, 1 << 60, 0, 0]],     # one unit apart where float64 no longer tells them apart
                     dtype=torch.int64)
    label, weight, second, total = query.labels_from_votes(t)
    assert label.dtype == torch.int64 and label.tolist() == [0, 1, -1, -1, 0, 2, 0]
    assert weight.tolist()[:6] == [5.0, 7.0, 0.0, 0.0, 1.0 + 2.0 ** -32, 0.5]
    assert second.tolist()[:6] == [2.0, 7.0, 0.0, 0.0, 1.0, 0.0]
    assert total.tolist()[:6] == [8.0, 16.0, 9.0, 0.0, 3.0, 2.0]
    assert query.labels_from_votes(t, min_weight=1.0)[0].tolist() == [0, 1, -1, -1, 0, -1, 0]
    assert query.labels_from_votes(t, min_weight=0.5)[0].tolist() == [0, 1, -1, -1, 0, 2, 0]
    assert query.labels_from_votes(t, min_share=0.5)[0].tolist() == [0, -1, -1, -1, -1, -1, 0]
    assert query.labels_from_votes(t, min_share=0.25)[0].tolist() == [0, 1, -1, -1, 0, 2, 0]
    for kw in (dict(), dict(min_weight=1.0), dict(min_share=0.3), dict(min_weight=0.75, min_share=0.4)):
        got = query.labels_from_votes(t[:6], **kw)
        want = vr.labels_from_votes(t[:6].numpy().astype(np.float64) / Q, **kw)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a.numpy(), b)
    # L = 0: one column, nothing to win
    label, weight, second, total = query.labels_from_votes(torch.tensor([[3 * Q], [0]], dtype=torch.int64))
    assert label.tolist() == [-1, -1] and weight.tolist() == [0.0, 0.0] and total.tolist() == [3.0, 0.0]
    with pytest.raises(ValueError):
        query.labels_from_votes(t.to(torch.float64))
    with pytest.raises(ValueError):
        query.labels_from_votes(t[0])


def test_labels_from_votes_on_a_random_table():
    from opengaussian_amd import query
    g = torch.Generator().manual_seed(8)
    t = torch.randint(0, 6, (200, 9), generator=g, dtype=torch.int64) * (Q // 4)          # many exact ties and zeros
    got = query.labels_from_votes(t, min_weight=0.5, min_share=0.125)
    want = vr.labels_from_votes(t.numpy().astype(np.float64) / Q, min_weight=0.5, min_share=0.125)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.numpy(), b)


def test_leaves_from_votes_rules():
    """the selection rule of select_leaves_by_masks: inside weight and inside share of the leaf's whole visible weight"""
    from opengaussian_amd import query
    #                     prompt 0  prompt 1  outside
    t = torch.tensor([[6 * Q, 0, 2 * Q],                   # leaf 0: 0.75 inside prompt 0
                      [Q, Q, 2 * Q],                       # leaf 1: a quarter in each
                      [0, Q // 2, 0],                      # leaf 2: all of it in prompt 1, but only 0.5 of weight
                      [0, 0, 5 * Q],                       # leaf 3: outside
                      [4 * Q, 4 * Q, 0],                   # leaf 4: half in each
                      [0, 0, 0]], dtype=torch.int64)       # leaf 5: never seen
    sel = query.leaves_from_votes(t, min_share=0.5, min_weight=1.0)
    assert [s.dtype for s in sel] == [torch.int64] * 2 and [s.tolist() for s in sel] == [[0, 4], [4]]
    assert [s.tolist() for s in query.leaves_from_votes(t, min_share=0.5, min_weight=0.5)] == [[0, 4], [2, 4]]
    assert [s.tolist() for s in query.leaves_from_votes(t, min_share=0.25, min_weight=1.0)] == [[0, 1, 4], [1, 4]]
    assert [s.tolist() for s in query.leaves_from_votes(t, min_share=0.0, min_weight=0.0)] == [[0, 1, 4], [1, 2, 4]]
    assert [s.tolist() for s in query.leaves_from_votes(t, min_share=0.8, min_weight=0.0)] == [[], [2]]
    assert query.leaves_from_votes(t[:, 2:]) == []


# ---- validation --------------------------------------------------------------------------------------------------------------------
def test_label_votes_arguments_are_validated():
    from opengaussian_amd import rasterizer as R
    kept = dict(P=10, W=16, H=12, Cn=3, image=torch.zeros(8, dtype=torch.uint8), sorted_rec=torch.zeros(8, dtype=torch.uint8),
                quad_list=torch.zeros(8, dtype=torch.uint8))
    img = torch.zeros(12, 16, dtype=torch.int64)
    rows = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="integer"):
        R.label_votes(kept, img.float(), 3)
    with pytest.raises(RuntimeError, match="integer"):
        R.label_votes(kept, img.bool(), 3)
    with pytest.raises(RuntimeError, match="12 x 16"):
        R.label_votes(kept, img[:, :15], 3)
    with pytest.raises(RuntimeError, match="12 x 16"):
        R.label_votes(kept, img.reshape(-1), 3)
    with pytest.raises(RuntimeError, match="num_labels"):
        R.label_votes(kept, img, -1)
    with pytest.raises(RuntimeError, match="10 Gaussians"):
        R.label_votes(kept, img, 3, rows=rows[:9], num_rows=4)
    with pytest.raises(RuntimeError, match="integer"):
        R.label_votes(kept, img, 3, rows=rows.float(), num_rows=4)
    with pytest.raises(RuntimeError, match="num_rows"):
        R.label_votes(kept, img, 3, rows=rows)
    with pytest.raises(RuntimeError, match="num_rows"):
        R.label_votes(kept, img, 3, rows=rows, num_rows=0)
    with pytest.raises(RuntimeError, match="out must be"):
        R.label_votes(kept, img, 3, out=torch.zeros(10, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="out must be"):
        R.label_votes(kept, img, 3, out=torch.zeros(10, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.label_votes(kept, img, 3)
    # a grouped or tiny pass leaves no such state
    with pytest.raises(RuntimeError, match="ungrouped streaming pass"):
        R.label_votes(None, img, 3)
    with pytest.raises(RuntimeError, match="ungrouped streaming pass"):
        R.label_votes(dict(P=10, W=16, H=12), img, 3)


def test_c_abi_rejects_bad_arguments_on_the_host():
    """every argument error is a code from the host side: nothing is launched (no GPU is needed to see them)"""
    import ctypes as C
    from opengaussian_amd import _lib
    lib = _lib.lib()
    a = _lib.OgsRasterFwdArgs()
    a.P, a.W, a.H, a.C = 10, 16, 12, 3
    lv = _lib.OgsLabelVotesArgs()
    lv.num_labels, lv.num_rows = 3, 10
    fake = C.c_void_p(4096)          # never dereferenced: the calls below fail before any launch
    call = lambda: lib.ogs_raster_label_votes(C.byref(a), C.byref(lv), None)
    assert lib.ogs_raster_label_votes(None, C.byref(lv), None) < 0 and lib.ogs_raster_label_votes(C.byref(a), None, None) < 0
    assert call() < 0                                        # NULL pointers
    a.image_buffer = a.sorted_rec = a.quad_list = fake
    lv.pixel_labels = fake
    assert call() < 0                                        # votes == NULL
    lv.votes = fake
    lv.pixel_labels = None
    assert call() < 0                                        # pixel_labels == NULL
    lv.pixel_labels = fake
    for field, bad in (("num_rows", 0), ("num_rows", -4), ("num_labels", -1)):
        saved = getattr(lv, field)
        setattr(lv, field, bad)
        assert call() < 0, (field, bad)
        setattr(lv, field, saved)
    for field, bad in (("P", 0), ("W", 0), ("H", -1), ("C", 4), ("num_groups", 2)):
        saved = getattr(a, field)
        setattr(a, field, bad)
        assert call() < 0, (field, bad)
        setattr(a, field, saved)
