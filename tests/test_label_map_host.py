"""CPU: the plain-torch click helpers against their restatements, argument validation, and the conditions the label-map
cases must meet (computed from the oracle alone) before the GPU test may rely on them."""
import numpy as np
import pytest
import torch

from tests import label_map_cases as lc
from tests import label_map_restatement as lr


def _cap():
    from opengaussian_amd import _lib
    return int(_lib.lib().ogs_label_map_tile_capacity())


def _case_names():
    # the names do not depend on the capacity's value (64 here only shapes the ids); the cases themselves are built with the
    # library's own figure
    return [f"P{P}_L{L}" for P in lc.SCENE_PS for L in lc.SCENE_LS] + ["null", "wide"] + [f"cap_{k}" for k in range(4)]


def case_by_id(name, cap):
    if name.startswith("cap_"):
        n, _ = lc.capacity_counts(cap)[int(name[4:])]
        name = f"cap_{n}"
    return name, lc.all_cases(cap)[name]


# ---- labels_at_pixels ----------------------------------------------------------------------------------------------------------
def _random_map(seed, Hh=13, Ww=17, L=6):
    g = torch.Generator().manual_seed(seed)
    label = torch.randint(-1, L, (Hh, Ww), generator=g, dtype=torch.int32)
    weight = torch.rand(Hh, Ww, generator=g)
    weight[label < 0] = 0.0
    return label, weight


@pytest.mark.parametrize("radius", [0, 1, 3, 9])
def test_labels_at_pixels_equals_the_restatement(radius):
    from opengaussian_amd import query
    label, weight = _random_map(3 + radius)
    Hh, Ww = label.shape
    xy = torch.tensor([[0, 0], [Ww - 1, Hh - 1], [Ww - 1, 0], [0, Hh - 1], [5, 6], [16, 3], [8, 12], [1, 1]])
    got = query.labels_at_pixels(query.LabelMap(label, weight, weight, weight), xy, radius)
    assert got.dtype == torch.int64 and got.shape == (8,)
    np.testing.assert_array_equal(got.numpy(), lr.labels_at_pixels(label.numpy(), weight.numpy(), xy.numpy(), radius))


def test_labels_at_pixels_ties_and_empty_windows():
    from opengaussian_amd import query
    label = torch.tensor([[4, 2, -1, -1], [2, 4, -1, -1], [-1, -1, -1, 9]], dtype=torch.int32)
    weight = torch.tensor([[0.5, 0.25, 0.0, 0.0], [0.25, 0.5, 0.0, 0.0], [0.0, 0.0, 0.0, 0.125]])
    xy = torch.tensor([[0, 0], [1, 1], [2, 0], [3, 2], [3, 0]])
    # radius 0: the pixel's own label; an unlabelled pixel gives -1
    np.testing.assert_array_equal(query.labels_at_pixels((label, weight), xy, 0).numpy(), [4, 4, -1, 9, -1])
    # radius 1 around (0, 0): labels 4 and 2 ... 4 holds 1.0, 2 holds 0.5
    assert int(query.labels_at_pixels((label, weight), xy[:1], 1)) == 4
    # an exact tie goes to the lowest label
    weight[0, 0], weight[1, 1] = 0.25, 0.25
    assert int(query.labels_at_pixels((label, weight), xy[:1], 1)) == 2
    np.testing.assert_array_equal(query.labels_at_pixels((label, weight), xy, 1).numpy(),
                                  lr.labels_at_pixels(label.numpy(), weight.numpy(), xy.numpy(), 1))
    with pytest.raises(ValueError):
        query.labels_at_pixels((label, weight), torch.tensor([[0.5, 1.0]]), 0)
    with pytest.raises(ValueError):
        query.labels_at_pixels((label, weight[:2]), xy, 0)
    with pytest.raises(ValueError):
        query.labels_at_pixels((label, weight), xy, -1)


# ---- click_features ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantize", [True, False])
@pytest.mark.parametrize("radius", [0, 5, 10])
def test_click_features_equals_the_restatement(radius, quantize):
    from opengaussian_amd import query
    g = torch.Generator().manual_seed(11)
    fmap = torch.rand(6, 19, 23, generator=g) * 1.2 - 0.1               # a few values outside [0, 1]: the clamp of the 8-bit image
    xy = torch.tensor([[0, 0], [22, 18], [3, 15], [11, 9], [22, 0]])
    got = query.click_features(fmap, xy, radius=radius, quantize=quantize)
    assert got.dtype == torch.float32 and got.shape == (5, 6)
    want = lr.click_features(fmap.numpy(), xy.numpy(), radius=radius, quantize=quantize)
    assert np.abs(got.numpy() - want).max() <= 1e-6


# ---- select_leaves_by_click ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roots,leaves", [(4, 12), (3, 10), (64, 640)])
def test_select_leaves_by_click_equals_the_restatement(roots, leaves):
    from opengaussian_amd import query
    g = torch.Generator().manual_seed(roots)
    root_book = torch.randn(roots, 9, generator=g)
    leaf_book = torch.randn(leaves + 1, 6, generator=g)
    leaf_book[torch.randperm(leaves, generator=g)[: leaves // 4]] = 0.0         # unassigned leaves
    K = 40
    root_click = root_book[torch.randint(0, roots, (K,), generator=g), :6] + 0.3 * torch.randn(K, 6, generator=g)
    leaf_click = leaf_book[torch.randint(0, leaves, (K,), generator=g)] + 0.3 * torch.randn(K, 6, generator=g)
    got = query.select_leaves_by_click(root_click, leaf_click, root_book, leaf_book)
    assert got.dtype == torch.int64
    np.testing.assert_array_equal(got.numpy(), lr.select_leaves_by_click(root_click, leaf_click, root_book, leaf_book))
    with pytest.raises(ValueError):
        query.select_leaves_by_click(root_click[:, :5], leaf_click, root_book, leaf_book)


# ---- validation ----------------------------------------------------------------------------------------------------------------
def test_label_map_arguments_are_validated():
    from opengaussian_amd import rasterizer as R
    kept = dict(P=10, W=16, H=16, Cn=3, image=torch.zeros(8, dtype=torch.uint8), sorted_rec=torch.zeros(8, dtype=torch.uint8),
                quad_list=torch.zeros(8, dtype=torch.uint8))
    labels = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="integer"):
        R.label_map(kept, labels.float(), 3)
    with pytest.raises(RuntimeError, match="integer"):
        R.label_map(kept, labels.bool(), 3)
    with pytest.raises(RuntimeError, match="10 Gaussians"):
        R.label_map(kept, labels[:9], 3)
    with pytest.raises(RuntimeError, match="num_labels"):
        R.label_map(kept, labels, -1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.label_map(kept, labels, 3)
    # a grouped or tiny pass leaves no such state
    with pytest.raises(RuntimeError, match="ungrouped streaming pass"):
        R.label_map(None, labels, 3)
    with pytest.raises(RuntimeError, match="ungrouped streaming pass"):
        R.label_map(dict(P=10, W=16, H=16), labels, 3)


# ---- the cases' own conditions, from the oracle alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", _case_names())
def test_case_conditions(name):
    cap = _cap()
    name, c = case_by_id(name, cap)
    o = lc.oracle(name, cap)
    labels, L = c["labels"].numpy(), c["L"]
    valid = (labels >= 0) & (labels < L)
    labelled = o["label"] >= 0
    # decided pixels: at least 90 % of the labelled ones, so the GPU test never sets more than 10 % aside
    assert int(o["decided"].sum()) >= 0.9 * int(labelled.sum()), (int(o["decided"].sum()), int(labelled.sum()))
    assert not (o["decided"] & ~labelled).any()
    gx = (lc.W + 15) // 16
    per_tile = o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0].astype(np.int64)
    if name.startswith("cap_"):
        n = len(labels)
        assert len(np.unique(labels)) == n and valid.all()
        assert per_tile[1] == n, "all n Gaussians reach tile (1, 0)"
        # the pixels of that one tile show many labels between them: the capacity is exercised by what wins, not only by what is listed
        assert len(np.unique(o["label"][:16, 16:32][labelled[:16, 16:32]])) >= min(n, cap) // 2
        # labels of every sub-pass (rank // cap) win a decided pixel somewhere
        ranks = np.searchsorted(o["used"], np.unique(o["label"][o["decided"]])) // cap
        assert set(ranks.tolist()) == set(range((n + cap - 1) // cap)), sorted(set(ranks.tolist()))
    elif name == "null":
        assert not valid.any() and not labelled.any() and (o["alpha"] > 0).any()
    else:
        assert per_tile[0] == 0 and (per_tile[1:] > 0).all(), "tile (0, 0) sees nothing, every other tile does"
        assert gx == 3 and len(per_tile) == 6
        assert 0.25 < (labels == -1).mean() < 0.42 and (labels >= L).sum() >= 2 and (labels < -1).sum() == 2
        assert labelled.any() and (o["alpha"][~labelled] > 0).any(), "some pixels show unlabelled Gaussians only"
        # an unlabelled Gaussian in front: somewhere the labels' weights do not add up to alpha
        assert (o["alpha"] - o["W"].sum(0) > 1e-2).any()
        if name == "wide":
            assert o["used"].max() == 2 ** 31 - 2 and len(o["used"]) > 100
