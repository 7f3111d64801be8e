"""CPU: the feature-map restatement against a direct loop, the conditions the cases must meet (from the oracle alone) before the
GPU test may rely on them, query.relevancy_maps against a per-pixel loop, argument validation through the facade and the C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import feature_map_cases as mc
from tests import feature_map_restatement as mr
from tests import feature_votes_restatement as fr
from tests import label_votes_cases as vc


def _hooks():
    from opengaussian_amd import _lib
    return int(_lib.lib().ogs_feature_map_fold_columns()), int(_lib.lib().ogs_feature_map_block_columns())


def test_hooks_describe_the_fold():
    fold, block = _hooks()
    assert fold == 16 and block in (32, 64, 128) and block % fold == 0
    counts = [mc.channels_of(s, fold, block) for s in mc.CHANNELS]
    assert counts == [1, 3, fold - 1, fold, fold + 1, 2 * fold, 2 * fold + 1, block - 1, block, block + 1, 2 * block + 1]
    assert len(set(mc.CASE_NAMES)) == len(mc.CASE_NAMES) == 34


def _tiny_scene():
    from tests import label_map_cases as lmc
    c = lmc.scene_case(300, 5)
    sc = type(c["sc"])(*[getattr(c["sc"], f)[:60].contiguous() for f in ("means3D", "scales", "rotations", "opacities", "shs", "ins_feat")])
    return sc, c["cam"]


def test_restatement_equals_a_direct_loop():
    sc, cam = _tiny_scene()
    X = mc.features(60, 3).numpy()
    rows = vc.leaf_rows(60).numpy()
    for feats, r in ((X, None), (mc.features(vc.LEAF_ROWS, 3).numpy(), rows)):
        a, alpha_a = mr.feature_image(sc, cam, feats, r)
        b, alpha_b = mr.feature_image_by_loops(sc, cam, feats, r)
        assert a.shape == (3, mc.H, mc.W) and alpha_a.max() > 0.5 and (a < 0).any() and (a > 0).any()
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max() and np.abs(alpha_a - alpha_b).max() <= 1e-12
    # rows outside [0, R) occlude and add nothing: they changed the map, not the alpha
    assert ((rows < 0) | (rows >= vc.LEAF_ROWS)).any()
    full = mr.feature_image(sc, cam, mc.features(vc.LEAF_ROWS, 3).numpy(), np.clip(rows, 0, vc.LEAF_ROWS - 1))
    assert np.abs(full[0] - a).max() > 1e-3 and np.abs(full[1] - alpha_a).max() <= 1e-12
    # the tile weights restate the same blend: their sum over the entries is the alpha
    tw = mr.tile_weights(sc, cam)
    for t, (ids, w) in enumerate(tw):
        ty, tx = divmod(t, 3)
        want = alpha_a[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]
        assert np.abs(w.sum(0)[:want.shape[0], :want.shape[1]] - want).max() <= 1e-12


def test_map_is_the_transpose_of_the_votes_restatement():
    """sum(map(X) * F) = sum(X * table(F)[:, :D]): the two restatements are adjoint, which the GPU test then asks of the kernels"""
    sc, cam = _tiny_scene()
    X, F = mc.features(60, 3).double().numpy(), mc.upstream(3).double().numpy()
    lhs = (mr.feature_image(sc, cam, X)[0] * F).sum()
    rhs = (X * fr.feature_table(sc, cam, F)[:, :3]).sum()
    assert abs(lhs - rhs) <= 1e-10 * np.abs(X).sum()


def _quadrant_facts(scene):
    """per quadrant of every tile of a scene, from the fp32 restatement's weights: how many entries put weight on it (what the
    kernel stages when every row is counted), and whether a pixel stopped while a neighbour of the quadrant went on"""
    sc, cam = mc.scene(scene)
    H, W = cam.image_height, cam.image_width
    facts = []
    for t, (ids, w) in enumerate(mr.tile_weights(sc, cam, dtype=torch.float32)):
        ty, tx = divmod(t, 3)
        for q in range(4):
            y0, x0 = 8 * (q >> 1), 8 * (q & 1)
            hh, ww = min(8, H - ty * 16 - y0), min(8, W - tx * 16 - x0)
            if hh <= 0 or ww <= 0 or len(ids) == 0:
                continue
            wq = w[:, y0:y0 + hh, x0:x0 + ww].reshape(len(ids), -1)
            staged = np.nonzero((wq > 0).any(axis=1))[0]
            last = np.where((wq > 0).any(axis=0), len(ids) - 1 - np.argmax((wq > 0)[::-1], axis=0), -1)      # per pixel: its last entry
            alpha = wq.sum(axis=0)
            # a saturated pixel (alpha > 0.999: it met the stop rule) whose last entry precedes another pixel's
            early = bool(((alpha > 0.999) & (last < last.max())).any())
            facts.append(dict(tile=t, quadrant=q, staged=len(staged), early=early, partial=hh < 8 or ww < 8))
    return facts


def test_case_conditions():
    """across the scenes: a lone partial batch, an accumulator carried over several batches, a list beyond one 64-entry sub-chunk,
    a pixel that stops early while its neighbours go on, partial quadrants with entries"""
    facts = {s: _quadrant_facts(s) for s in mc.SCENES}
    every = [f for fs in facts.values() for f in fs]
    print({s: sorted(f["staged"] for f in fs) for s, fs in facts.items()})
    assert any(1 <= f["staged"] <= 15 for f in every)
    assert any(f["staged"] > 32 for f in every)
    assert any(f["staged"] > 64 for f in every)                      # more entries with weight than a sub-chunk holds
    assert any(f["staged"] % 16 not in (0,) and f["staged"] > 16 for f in every)      # a partial batch after whole ones
    assert any(f["early"] for f in every)
    assert any(f["partial"] and f["staged"] > 0 for f in facts["odd"]) and not any(f["partial"] for s in ("P300", "P1500", "wide") for f in facts[s])
    assert mc.ODD_W % 4 and (mc.ODD_W * mc.ODD_H) % 4 and mc.ODD_W % 8 and mc.ODD_H % 8      # 4-byte planar stores, cut quadrants
    # with the leaf rows some staged entries drop out (a tenth of the rows is -1): the counts differ from rows = None
    assert (vc.leaf_rows(1500) < 0).sum() > 100


@pytest.mark.parametrize("name", ["P300_3", "P1500_f+1_rows", "wide_3_rows", "odd_3"])
def test_oracle_shapes_and_fp32_graph(name):
    fold, block = _hooks()
    c = mc.case(name, fold, block)
    m, a = mc.oracle(name, fold, block)
    m32, a32 = mc.oracle_fp32(name, fold, block)
    assert m.shape == (c["D"], c["H"], c["W"]) and a.shape == (c["H"], c["W"]) and a.max() > 0.9 and (m < 0).any() and (m > 0).any()
    assert np.abs(a - a32).max() <= 1e-2 and np.mean(np.abs(m - m32).max(axis=0) > mc.MAP_BAR * np.abs(m).max()) <= 2e-3


# ---- relevancy -------------------------------------------------------------------------------------------------------------------------
def test_relevancy_maps_against_a_pixel_loop():
    from opengaussian_amd import query
    g = torch.Generator().manual_seed(8)
    D, H, W, Q, K = 5, 6, 7, 3, 4
    fmap = torch.randn(D, H, W, generator=g)
    fmap[:, 2, 3] = 0.0                                              # a pixel without a feature
    text, canon = torch.randn(Q, D, generator=g), torch.randn(K, D, generator=g)
    for kw in (dict(), dict(chunk=5), dict(chunk=1)):
        sim = query.relevancy_maps(fmap, text, **kw)
        assert sim.shape == (Q, H, W) and sim.dtype == torch.float32
        np.testing.assert_allclose(sim.numpy(), mr.relevancy_by_loops(fmap.numpy(), text.numpy()), rtol=0, atol=2e-6)
        assert bool((sim[:, 2, 3] == 0).all()) and float(sim.abs().max()) <= 1 + 1e-6
        rel = query.relevancy_maps(fmap, text, canon, **kw)
        np.testing.assert_allclose(rel.numpy(), mr.relevancy_by_loops(fmap.numpy(), text.numpy(), canon.numpy()), rtol=0, atol=2e-6)
        assert bool((rel[:, 2, 3] == 0.5).all())
        last = fmap.permute(1, 2, 0).contiguous()
        np.testing.assert_allclose(query.relevancy_maps(last, text, canon, channels_last=True, **kw).numpy(), rel.numpy(), rtol=0, atol=2e-6)
        np.testing.assert_allclose(query.relevancy_maps(last, text, channels_last=True, **kw).numpy(), sim.numpy(), rtol=0, atol=2e-6)
    # scale invariance and the text's own direction
    np.testing.assert_allclose(query.relevancy_maps(3 * fmap, 0.5 * text).numpy(), sim.numpy(), rtol=0, atol=2e-6)
    own = query.relevancy_maps(text.t().reshape(D, 1, Q).contiguous(), text)
    np.testing.assert_allclose(torch.diagonal(own[:, 0, :]).numpy(), np.ones(Q), rtol=0, atol=2e-6)
    # differentiable in the map
    f = fmap.clone().requires_grad_(True)
    query.relevancy_maps(f, text, canon).sum().backward()
    assert f.grad is not None and bool(torch.isfinite(f.grad).all()) and float(f.grad.abs().max()) > 0
    with pytest.raises(ValueError):
        query.relevancy_maps(fmap, text[:, :-1])
    with pytest.raises(ValueError):
        query.relevancy_maps(fmap, text, canon[:, :-1])
    with pytest.raises(ValueError):
        query.relevancy_maps(fmap[0], text)


# ---- validation ------------------------------------------------------------------------------------------------------------------------
def test_feature_map_arguments_are_validated():
    from opengaussian_amd import rasterizer as R
    kept = dict(P=10, W=16, H=12, Cn=3, image=torch.zeros(8, dtype=torch.uint8), sorted_rec=torch.zeros(8, dtype=torch.uint8),
                quad_list=torch.zeros(8, dtype=torch.uint8))
    X = torch.zeros(10, 3)
    rows = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="floating"):
        R.feature_map(kept, X.to(torch.int32))
    with pytest.raises(RuntimeError, match="tensor"):
        R.feature_map(kept, X.numpy())
    with pytest.raises(RuntimeError, match=r"\[R >= 1, D >= 1\]"):
        R.feature_map(kept, X[0])
    with pytest.raises(RuntimeError, match=r"\[R >= 1, D >= 1\]"):
        R.feature_map(kept, X[:, :0])
    with pytest.raises(RuntimeError, match=r"\[R >= 1, D >= 1\]"):
        R.feature_map(kept, X[:0], rows=rows)
    with pytest.raises(RuntimeError, match="10 Gaussians"):
        R.feature_map(kept, X[:9])                                   # R must be P without rows
    with pytest.raises(RuntimeError, match="10 Gaussians"):
        R.feature_map(kept, X, rows=rows[:9])
    with pytest.raises(RuntimeError, match="integer"):
        R.feature_map(kept, X, rows=rows.float())
    with pytest.raises(RuntimeError, match="integer"):
        R.feature_map(kept, X, rows=rows.bool())
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.feature_map(kept, X)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.feature_map(kept, X[:4], rows=rows)
    with pytest.raises(RuntimeError, match="ungrouped streaming pass"):
        R.feature_map(None, X)
    with pytest.raises(RuntimeError, match="ungrouped streaming pass"):
        R.feature_map(dict(P=10, W=16, H=12), X)


def test_c_abi_rejects_bad_arguments_on_the_host():
    """every argument error is a code from the host side: nothing is launched (no GPU is needed to see them)"""
    from opengaussian_amd import _lib
    lib = _lib.lib()
    a = _lib.OgsRasterFwdArgs()
    a.P, a.W, a.H, a.C = 10, 16, 12, 3
    fm = _lib.OgsFeatureMapArgs()
    fm.num_channels, fm.num_rows = 3, 10
    fake = C.c_void_p(4096)          # never dereferenced: the calls below fail before any launch
    call = lambda: lib.ogs_raster_feature_map(C.byref(a), C.byref(fm), None)
    assert lib.ogs_raster_feature_map(None, C.byref(fm), None) < 0 and lib.ogs_raster_feature_map(C.byref(a), None, None) < 0
    assert call() < 0                                        # NULL pointers
    a.image_buffer = a.sorted_rec = a.quad_list = fake
    fm.features = fake
    assert call() < 0                                        # out_map == NULL
    fm.out_map = fake
    fm.features = None
    assert call() < 0                                        # features == NULL
    fm.features = fake
    block = int(lib.ogs_feature_map_block_columns())
    for field, bad in (("num_rows", 0), ("num_rows", -4), ("num_channels", 0), ("num_channels", -1),
                       ("num_channels", 65535 * block + 1)):     # one walk more than the grid's second dimension holds
        saved = getattr(fm, field)
        setattr(fm, field, bad)
        assert call() < 0, (field, bad)
        setattr(fm, field, saved)
    for field, bad in (("P", 0), ("W", 0), ("H", -1), ("C", 4), ("num_groups", 2)):
        saved = getattr(a, field)
        setattr(a, field, bad)
        assert call() < 0, (field, bad)
        setattr(a, field, saved)
