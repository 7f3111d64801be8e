"""CPU: the feature-votes restatement against a direct loop, the conditions the cases must meet (from the oracle alone) before
the GPU test may rely on them, query.features_from_votes and the algebra of query.lift_mask_features on hand-made integer
tables, argument validation through the facade and the C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import feature_votes_cases as fc
from tests import feature_votes_restatement as fr
from tests import label_votes_cases as vc
from tests import label_votes_restatement as vr

Q = 1 << 32        # units per unit of blend weight


def _hooks():
    from opengaussian_amd import _lib
    return int(_lib.lib().ogs_feature_votes_fold_columns()), int(_lib.lib().ogs_feature_votes_block_columns())


def test_hooks_describe_the_fold():
    from opengaussian_amd import _lib
    fold, block = _hooks()
    assert fold == 16 == int(_lib.lib().ogs_label_votes_fold_columns())
    assert block in (16, 32, 64) and block % fold == 0
    counts = [fc.channels_of(s, fold, block) for s in fc.CHANNELS]
    assert counts == [1, 3, fold - 1, fold, fold + 1, block - 1, block, block + 1, 2 * block + 1]


def _tiny_scene():
    from tests import label_map_cases as lmc
    c = lmc.scene_case(300, 5)
    sc = type(c["sc"])(*[getattr(c["sc"], f)[:60].contiguous() for f in ("means3D", "scales", "rotations", "opacities", "shs", "ins_feat")])
    return sc, c["cam"]


def test_restatement_equals_a_direct_loop():
    """the autograd route is the table of the definition: a per-pixel, per-entry loop over w = alpha * T on a tiny case, with and
    without the mask"""
    sc, cam = _tiny_scene()
    F = fc.features(3).numpy()
    for valid in (None, fc.valid_mask().numpy()):
        a = fr.feature_table(sc, cam, F, valid)
        b = fr.feature_table_by_loops(sc, cam, F, valid)
        assert a.shape == (60, 4) and a[:, 3].max() > 0.5 and (a[:, :3] < 0).any()
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    # the mask gates contributions, not occlusion: the masked weight column is the unmasked walk restricted to the valid pixels,
    # which the label restatement gives as column 0 of the image (valid ? 0 : -1)
    lab = np.where(fc.valid_mask().numpy(), 0, -1)
    assert np.abs(a[:, 3] - vr.vote_table(sc, cam, lab, 1)[:, 0]).max() <= 1e-12 * a[:, 3].max()


def test_one_hot_features_restate_the_label_votes():
    sc, cam = _tiny_scene()
    img, L = vc.label_image("noise", 5)
    lab = vc.clamp_labels(img.numpy(), L)
    F = (lab[None] == np.arange(L)[:, None, None]).astype(np.float32)
    a = fr.feature_table(sc, cam, F)
    b = vr.vote_table(sc, cam, img.numpy(), L)
    assert np.abs(a[:, :L] - b[:, :L]).max() <= 1e-12 * b.max()
    assert np.abs(a[:, L] - b.sum(axis=1)).max() <= 1e-12 * b.max()


@pytest.mark.parametrize("name", ["P300_3", "P300_3_masked", "wide_3_masked", "P1500_f+1_masked"])
def test_case_conditions(name):
    fold, block = _hooks()
    c = fc.case(name, fold, block)
    t = fc.oracle(name, fold, block)
    P, D = c["sc"].means3D.shape[0], c["D"]
    assert t.shape == (P, D + 1) and (t[:, D] >= 0).all() and t[:, D].max() > 0.5
    assert (t[:, :D] < 0).any() and (t[:, :D] > 0).any()                       # negative partials are exercised
    if c["valid"] is not None:
        v = c["valid"].numpy()
        assert 0.4 < v.mean() < 0.5
        assert not v[vc.QUAD_Y0:vc.QUAD_Y0 + 8, vc.QUAD_X0:vc.QUAD_X0 + 8].any()
        # every other quadrant is half valid
        quads = [v[y:y + 8, x:x + 8].mean() for y in range(0, fc.H, 8) for x in range(0, fc.W, 8)]
        assert sorted(set(quads)) == [0.0, 0.5]
        full = fc.oracle(name.replace("_masked", ""), fold, block)
        assert (t[:, D] <= full[:, D] + 1e-12).all() and t[:, D].sum() < 0.6 * full[:, D].sum()
    if name.startswith("wide"):
        assert t[:, D].max() > 5 * t[:300, D].max()                            # the wide Gaussians own the weight column's maximum


def test_fp32_graph_is_close_to_float64():
    fold, block = _hooks()
    a, b = fc.oracle("P300_3", fold, block), fc.oracle_fp32("P300_3", fold, block)
    assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max()


# ---- the table helpers ---------------------------------------------------------------------------------------------------------------
def test_features_from_votes_rules():
    from opengaussian_amd import query
    t = torch.tensor([[3 * Q, -Q, 2 * Q],                  # weight 2: mean (1.5, -0.5)
                      [Q, Q, Q // 2],                      # weight 0.5: mean (2, 2)
                      [5 * Q, 7 * Q, 0],                   # no weight (cannot happen from the kernel): zeros
                      [0, 0, 0],                           # never seen
                      [-3, 1, 4]],                         # a few units
                     dtype=torch.int64)
    feat, weight = query.features_from_votes(t)
    assert feat.dtype == torch.float64 and weight.dtype == torch.float64
    assert feat.tolist() == [[1.5, -0.5], [2.0, 2.0], [0.0, 0.0], [0.0, 0.0], [-0.75, 0.25]]
    assert weight.tolist() == [2.0, 0.5, 0.0, 0.0, 4 * 2.0 ** -32]
    feat, weight = query.features_from_votes(t, min_weight=0.5)             # weight <= min_weight: zeros
    assert feat.tolist() == [[1.5, -0.5], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]
    assert weight.tolist() == [2.0, 0.5, 0.0, 0.0, 4 * 2.0 ** -32]
    for kw in (dict(), dict(min_weight=0.5), dict(min_weight=1e-9)):
        got = query.features_from_votes(t, **kw)
        want = fr.features_from_table(t.numpy().astype(np.float64) / Q, **kw)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a.numpy(), b)
    with pytest.raises(ValueError):
        query.features_from_votes(t.to(torch.float64))
    with pytest.raises(ValueError):
        query.features_from_votes(t[0])
    with pytest.raises(ValueError):
        query.features_from_votes(t[:, :1])


def test_features_from_votes_on_a_random_table():
    from opengaussian_amd import query
    g = torch.Generator().manual_seed(3)
    t = torch.randint(-5 * Q, 5 * Q, (200, 9), generator=g, dtype=torch.int64)
    t[:, -1] = torch.randint(0, 4, (200,), generator=g, dtype=torch.int64) * (Q // 2)        # many zero weights
    got = query.features_from_votes(t, min_weight=0.25)
    want = fr.features_from_table(t.numpy().astype(np.float64) / Q, min_weight=0.25)
    assert (want[1] == 0).sum() > 20
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.numpy(), b)


def test_mask_votes_times_feats_algebra():
    """one view of lift_mask_features on a stand-in label-vote table: votes of the L mask columns times the mask features, the
    no-mask column dropped, accumulated over views"""
    from opengaussian_amd import query
    g = torch.Generator().manual_seed(11)
    R, L, D = 6, 4, 3
    table = torch.randint(0, 9, (R, L + 1), generator=g, dtype=torch.int64) * (Q // 4)
    M = torch.randn(L, D, generator=g)
    zero_f, zero_w = torch.zeros(R, D, dtype=torch.float64), torch.zeros(R, dtype=torch.float64)
    feat, weight = query._mask_votes_times_feats(table, M, zero_f, zero_w)
    assert feat.dtype == torch.float64 and weight.dtype == torch.float64
    want = np.zeros((R, D))
    for r in range(R):
        for l in range(L):
            want[r] += (table[r, l].item() / Q) * M[l].double().numpy()
    np.testing.assert_allclose(feat.numpy(), want, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(weight.numpy(), table[:, :L].sum(1).numpy() / Q)
    # a second view with another number of masks accumulates
    table2 = torch.randint(0, 9, (R, 3), generator=g, dtype=torch.int64) * (Q // 4)
    M2 = torch.randn(2, D, generator=g)
    feat2, weight2 = query._mask_votes_times_feats(table2, M2, feat, weight)
    np.testing.assert_allclose(feat2.numpy(), want + (table2[:, :2].double() / Q).numpy() @ M2.double().numpy(), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(weight2.numpy(), weight.numpy() + table2[:, :2].sum(1).numpy() / Q)
    # one-hot mask features give back the votes: the mean feature of a row is its share per mask
    feat, weight = query._mask_votes_times_feats(table, torch.eye(L), zero_f[:, :1].expand(R, L), zero_w)
    np.testing.assert_array_equal(feat.numpy(), table[:, :L].numpy() / Q)


# ---- validation --------------------------------------------------------------------------------------------------------------------
def test_feature_votes_arguments_are_validated():
    from opengaussian_amd import rasterizer as R
    kept = dict(P=10, W=16, H=12, Cn=3, image=torch.zeros(8, dtype=torch.uint8), sorted_rec=torch.zeros(8, dtype=torch.uint8),
                quad_list=torch.zeros(8, dtype=torch.uint8))
    F = torch.zeros(3, 12, 16)
    rows = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="floating"):
        R.feature_votes(kept, F.to(torch.int32))
    with pytest.raises(RuntimeError, match="tensor"):
        R.feature_votes(kept, F.numpy())
    with pytest.raises(RuntimeError, match="12 x 16"):
        R.feature_votes(kept, F[:, :, :15])
    with pytest.raises(RuntimeError, match="12 x 16"):
        R.feature_votes(kept, F[0])
    with pytest.raises(RuntimeError, match="12 x 16"):
        R.feature_votes(kept, F[:0])
    with pytest.raises(RuntimeError, match="valid"):
        R.feature_votes(kept, F, valid=torch.ones(12, 16))
    with pytest.raises(RuntimeError, match="12 x 16"):
        R.feature_votes(kept, F, valid=torch.ones(12, 15, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="10 Gaussians"):
        R.feature_votes(kept, F, rows=rows[:9], num_rows=4)
    with pytest.raises(RuntimeError, match="integer"):
        R.feature_votes(kept, F, rows=rows.float(), num_rows=4)
    with pytest.raises(RuntimeError, match="num_rows"):
        R.feature_votes(kept, F, rows=rows)
    with pytest.raises(RuntimeError, match="num_rows"):
        R.feature_votes(kept, F, rows=rows, num_rows=0)
    with pytest.raises(RuntimeError, match="out must be"):
        R.feature_votes(kept, F, out=torch.zeros(10, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="out must be"):
        R.feature_votes(kept, F, out=torch.zeros(10, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.feature_votes(kept, F)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.feature_votes(kept, F, valid=torch.ones(12, 16, dtype=torch.bool))
    # a grouped or tiny pass leaves no such state
    with pytest.raises(RuntimeError, match="ungrouped streaming pass"):
        R.feature_votes(None, F)
    with pytest.raises(RuntimeError, match="ungrouped streaming pass"):
        R.feature_votes(dict(P=10, W=16, H=12), F)


def test_c_abi_rejects_bad_arguments_on_the_host():
    """every argument error is a code from the host side: nothing is launched (no GPU is needed to see them)"""
    from opengaussian_amd import _lib
    lib = _lib.lib()
    a = _lib.OgsRasterFwdArgs()
    a.P, a.W, a.H, a.C = 10, 16, 12, 3
    fv = _lib.OgsFeatureVotesArgs()
    fv.num_channels, fv.num_rows = 3, 10
    fake = C.c_void_p(4096)          # never dereferenced: the calls below fail before any launch
    call = lambda: lib.ogs_raster_feature_votes(C.byref(a), C.byref(fv), None)
    assert lib.ogs_raster_feature_votes(None, C.byref(fv), None) < 0 and lib.ogs_raster_feature_votes(C.byref(a), None, None) < 0
    assert call() < 0                                        # NULL pointers
    a.image_buffer = a.sorted_rec = a.quad_list = fake
    fv.features = fake
    assert call() < 0                                        # votes == NULL
    fv.votes = fake
    fv.features = None
    assert call() < 0                                        # features == NULL
    fv.features = fake
    block = int(lib.ogs_feature_votes_block_columns())
    for field, bad in (("num_rows", 0), ("num_rows", -4), ("num_channels", 0), ("num_channels", -1),
                       ("num_channels", 65535 * block)):     # D + 1 columns: one walk more than the grid's second dimension holds
        saved = getattr(fv, field)
        setattr(fv, field, bad)
        assert call() < 0, (field, bad)
        setattr(fv, field, saved)
    for field, bad in (("P", 0), ("W", 0), ("H", -1), ("C", 4), ("num_groups", 2)):
        saved = getattr(a, field)
        setattr(a, field, bad)
        assert call() < 0, (field, bad)
        setattr(a, field, saved)
