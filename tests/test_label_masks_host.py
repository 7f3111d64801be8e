"""CPU: mask_ops.get_SAM_mask_and_feat / LabelMasks against tests/golden/sam_labels_golden.npz (the reference's own
get_SAM_mask_and_feat run on the CPU, tests/golden/make_sam_labels_golden.py), everything exact; the label path of the
loss functions refuses CPU tensors like the stack path; the five label entry points are part of the C ABI."""
import os

import numpy as np
import pytest
import torch

from tests.golden.make_sam_labels_golden import CASES, LEVELS, case_id, case_inputs

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "sam_labels_golden.npz"))
LABEL_SYMBOLS = ("ogs_label_feature_sums", "ogs_label_feature_sums_backward", "ogs_label_cohesion",
                 "ogs_label_cohesion_backward", "ogs_label_feature_sqdev")


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_drop_in_matches_reference_golden(case, level):
    from opengaussian_amd import mask_ops as mk
    gt, feats = case_inputs(*case)
    k = f"{case_id(case)}_L{level}"
    gt_before = gt.clone()
    four = mk.get_SAM_mask_and_feat(gt, level=level, original_mask_feat=feats)
    three = mk.get_SAM_mask_and_feat(gt, level=level)
    assert len(four) == 4 and len(three) == 3
    assert torch.equal(gt, gt_before)                                    # the input is not written
    mask_id, masks, mask_feat, invalid = four
    assert mask_id.dtype == torch.int64 and invalid.dtype == torch.bool
    np.testing.assert_array_equal(mask_id.numpy(), GOLD[k + "_mask_id"])
    np.testing.assert_array_equal(invalid.numpy(), GOLD[k + "_invalid_pix"])
    np.testing.assert_array_equal(mask_feat.numpy(), GOLD[k + "_mask_feat"])
    want = GOLD[k + "_mask_bool"]
    assert isinstance(masks, mk.LabelMasks) and not isinstance(masks, torch.Tensor)
    assert masks.labels.dtype == torch.int32 and masks.labels.is_contiguous()
    assert masks.labels.shape == mask_id.shape
    assert masks.num_mask == int(mask_id.max()) == want.shape[0] == len(masks)
    assert masks.shape == want.shape
    dense = masks.dense()
    assert dense.dtype == torch.bool and tuple(dense.shape) == want.shape
    np.testing.assert_array_equal(dense.numpy().astype(np.uint8), want)
    assert masks.to("cpu").shape == masks.shape
    # the three-value form returns the same things
    assert torch.equal(three[0], mask_id) and torch.equal(three[2], invalid)
    assert torch.equal(three[1].labels, masks.labels) and three[1].num_mask == masks.num_mask


def test_goldens_hold_an_empty_row_and_an_empty_level():
    """what the fixture is for: each stack has a level without any mask and a level with an id that has no pixel"""
    for case in CASES:
        n = [GOLD[f"{case_id(case)}_L{lvl}_mask_bool"] for lvl in LEVELS]
        assert sorted(m.shape[0] == 0 for m in n) == [False, True]
        full = [m for m in n if m.shape[0]][0]
        assert (full.reshape(full.shape[0], -1).sum(1) == 0).sum() == 1


def test_label_masks_on_cpu_are_refused():
    from opengaussian_amd import mask_ops as mk
    masks = mk.LabelMasks(torch.randint(0, 4, (8, 12)), 3)
    feat = torch.rand(6, 8, 12)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mk.mask_feature_mean(feat, masks)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mk.cohesion_loss(feat, masks, torch.rand(3, 6))


def test_label_entry_points_declared_exported_and_bound():
    import ctypes
    from opengaussian_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ogs_mask.h")).read()
    _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in LABEL_SYMBOLS:
        assert f"int {name}(" in hdr, name
        assert hasattr(raw, name), name
        dense = name.replace("ogs_label_", "ogs_mask_")
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[dense]           # the dense twin's argument list
