"""CPU: the mask-reduction oracle (oracle/mask_oracle.py) against the goldens produced by the reference's own
functions (tests/golden/make_mask_golden.py), plus the torch-only host functions of the product module."""
import os

import numpy as np
import pytest
import torch

from tests.golden.make_mask_golden import CASES, case_inputs
from tests.golden import make_separation_golden as sg

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "mask_golden.npz"))
SEP_GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "separation_golden.npz"))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"s{c[0]}")
def test_oracle_matches_reference_goldens(case):
    from oracle import mask_oracle as mo
    seed, C, H, W, N, overlap = case
    feat, masks, sil, masks2 = case_inputs(*case)
    k = f"s{seed}"
    np.testing.assert_allclose(mo.mask_feature_mean(feat, masks, image_mask=sil).numpy(), GOLD[k + "_mean_w"], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(mo.mask_feature_mean(feat, masks).numpy(), GOLD[k + "_mean"], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(mo.mask_feature_mean(feat, masks.long(), image_mask=sil).numpy(), GOLD[k + "_mean_int64"], rtol=2e-5, atol=1e-6)
    mean, var, cnt = mo.mask_feature_mean(feat, masks, return_var=True)
    np.testing.assert_allclose(var.numpy(), GOLD[k + "_var"], rtol=1e-4, atol=1e-6)
    np.testing.assert_array_equal(cnt.numpy(), GOLD[k + "_cnt"])
    mean_w = torch.from_numpy(GOLD[k + "_mean_w"])
    np.testing.assert_allclose(float(mo.cohesion_loss(feat, masks, mean_w)), float(GOLD[k + "_cohesion"]), rtol=2e-5)
    for base in (None, "former", "later"):
        np.testing.assert_allclose(mo.calculate_iou(masks, masks2, base=base).numpy(), GOLD[k + f"_iou_{base}"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"s{c[0]}")
def test_oracle_gradient_of_stage1_loss_matches_reference(case):
    """d(separation + 0.1 * cohesion)/d feat_map through autograd of the oracle == the reference's (train.py:450-456)."""
    from oracle import mask_oracle as mo
    from opengaussian_amd.mask_ops import separation_loss
    seed, C, H, W, N, overlap = case
    feat, masks, sil, _ = case_inputs(*case)
    fm = feat.clone().requires_grad_(True)
    sw = sil.clone().requires_grad_(True)
    mean_w = mo.mask_feature_mean(fm, masks, image_mask=sw)
    loss = separation_loss(mean_w, 1000) + 0.1 * mo.cohesion_loss(fm, masks, mean_w)
    loss.backward()
    want = GOLD[f"s{seed}_dfeat"]
    assert np.abs(fm.grad.numpy() - want).max() <= 2e-5 * np.abs(want).max() + 1e-9
    want = GOLD[f"s{seed}_dsil"]
    assert np.abs(sw.grad.numpy() - want).max() <= 2e-5 * np.abs(want).max() + 1e-9


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"s{c[0]}")
def test_host_side_torch_functions_match_reference(case):
    from opengaussian_amd.mask_ops import pair_mask_feature_mean, separation_loss
    seed, C, H, W, N, overlap = case
    feat, masks, sil, _ = case_inputs(*case)
    k = f"s{seed}"
    mean_w = torch.from_numpy(GOLD[k + "_mean_w"])
    np.testing.assert_allclose(float(separation_loss(mean_w, 1000)), float(GOLD[k + "_separation"]), rtol=1e-5)
    np.testing.assert_allclose(float(separation_loss(mean_w, 40000)), float(GOLD[k + "_sep_late"]), rtol=1e-5)
    pm = torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(seed))
    np.testing.assert_allclose(pair_mask_feature_mean(pm, masks).numpy(), GOLD[k + "_pair"], rtol=1e-5, atol=1e-7)


def test_mask_ops_refuse_cpu_tensors():
    from opengaussian_amd import mask_ops
    feat, masks, sil, _ = case_inputs(*CASES[0])
    with pytest.raises(RuntimeError):
        mask_ops.mask_feature_mean(feat, masks)
    with pytest.raises(RuntimeError):
        mask_ops.cohesion_loss(feat, masks, torch.zeros(masks.shape[0], feat.shape[0]))
    with pytest.raises(RuntimeError):
        mask_ops.calculate_iou(masks, masks)


@pytest.mark.parametrize("mode", list(sg.ITERATIONS))
@pytest.mark.parametrize("N,C", sg.CASES, ids=lambda v: str(v))
def test_separation_oracle_and_torch_formulation_match_reference(N, C, mode):
    """separation_golden.npz (the reference's separation_loss in float64, early and late weights; N - 1 divisible by 9
    puts a rank exactly on the late threshold) against the float64 oracle restatement -- to float64 rounding, value and
    gradient -- and against the product's torch formulation, in float64 likewise and in float32 at the bars of the GPU
    test: value 2e-6 relative, gradient max(1e-5, 4 * e32) of the largest entry, e32 = the deviation of the reference's
    own float32 gradient, read from the file."""
    from oracle import mask_oracle as mo
    from opengaussian_amd.mask_ops import _separation_loss_torch
    it = sg.ITERATIONS[mode]
    base = sg.case_means(N, C)
    assert float(sg.rank_gap(base).min()) >= sg.GAP               # input condition: no rank hangs on a float32 rounding
    k = f"n{N}_c{C}_{mode}"
    value, grad, e32 = float(SEP_GOLD[k + "_value"]), SEP_GOLD[k + "_grad"], float(SEP_GOLD[k + "_e32"])
    assert grad.shape == (N, C) and grad.dtype == np.float64 and 0.0 < e32 < 1e-6
    for f, dtype, vtol, gtol in ((lambda m: mo.separation_loss(m, it), torch.float64, 1e-13, 1e-12),
                                 (lambda m: _separation_loss_torch(m, it), torch.float64, 1e-13, 1e-12),
                                 (lambda m: _separation_loss_torch(m, it), torch.float32, 2e-6, max(1e-5, 4 * e32))):
        m = base.clone().to(dtype).requires_grad_(True)
        loss = f(m)
        loss.backward()
        assert loss.dtype == dtype
        assert abs(float(loss.detach()) - value) <= vtol * abs(value)
        assert np.abs(m.grad.double().numpy() - grad).max() <= gtol * np.abs(grad).max()


def test_separation_late_threshold_is_kept_on_the_boundary():
    """(8/9) * 0.9 + 0.1 rounds to 0.90000004 in float32: rank 8 (N-1) / 9 keeps its weight under the late rule"""
    from oracle import mask_oracle as mo
    for N in (10, 19, 37, 1000):
        r = torch.arange(N)
        early, late = mo.separation_weights(r, 1000), mo.separation_weights(r, 40000)
        b = 8 * (N - 1) // 9
        assert float(early[b]) == float(np.float32(0.90000004)) and float(late[b]) == float(early[b])
        assert float(late[b - 1]) == float(np.float32(0.1)) and bool((late[b:] == early[b:]).all())
        assert bool((early[1:] > early[:-1]).all())


def test_separation_no_rank_weight_equals_the_late_threshold():
    """for no N the kernel serves (2 .. 1024) is a rank weight float32(0.9) itself, so `< 0.9` and `<= 0.9` decide alike and
    the only exact decision of the late rule is the one above, on the kept side"""
    from oracle import mask_oracle as mo
    for N in range(2, 1025):
        assert not bool((mo.separation_weights(torch.arange(N), 1000) == torch.tensor(0.9)).any()), N
