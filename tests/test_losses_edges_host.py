"""CPU: pins for the edge fixture of tests/test_36_losses_edges_gpu.py (tests/golden/loss_edges_golden*.npz, produced by the
reference's own functions through tests/golden/make_loss_edges_golden.py).

The GPU file compares with the fixture where an array is stored and with tests/loss_restatement.py in fp64 elsewhere, and it
builds the expected photometric gradient as a sign(img - gt) / N + b grad_ssim.  Here: the restatement in fp64 reproduces
every stored value and array to 1e-10; that formula reproduces the restatement's autograd gradient for every upstream row;
the stored fp32 deviations (v32, e32) are what an fp32 run gives.
"""
import numpy as np
import pytest
import torch

from tests import loss_restatement as lr
from tests.golden import make_loss_edges_golden as me

GOLD = me.load_golden()
RESTATED = {"l1_loss": lr.l1_loss, "l2_loss": lr.l2_loss, "ssim": lr.ssim}
NOISE = lambda k: "_v32_" in k or "_e32" in k


@pytest.fixture(scope="module")
def restated():
    """the generator's records, from the restatement instead of the reference's functions"""
    return me.all_records(RESTATED)


def test_fixture_holds_every_case_and_nothing_over_the_size_limit(restated):
    import glob
    import os
    paths = glob.glob(os.path.join(me.HERE, me.PATTERN))
    assert paths and all(os.path.getsize(p) < 1024 * 1024 for p in paths)
    assert set(GOLD) == set(restated)
    assert len(me.PHOTO_CASES) == 16 and sum(H * W for H, W, _ in me.PHOTO_CASES) < 28000
    assert len(me.MASKED_CASES) == 11 * 2 * 5
    for i, (hw, C, kind) in enumerate(me.MASKED_CASES):
        assert (f"{me.masked_key(i)}_l1_dx" in GOLD) == (hw in me.DX_STORED)
        H, W = me.MASKED_HW[hw]
        assert H * W == hw


def test_restatement_fp64_reproduces_every_stored_value_and_array(restated):
    """weight_chw and the negative weights of `negw` included: their dx are stored"""
    checked = 0
    for k in sorted(GOLD):
        if NOISE(k):
            continue
        want, got = np.asarray(GOLD[k], np.float64), np.asarray(restated[k], np.float64)
        assert want.shape == got.shape and GOLD[k].dtype == np.float64, k
        top = float(np.abs(want).max())
        # a zero weight gives exactly 0; the `delta` gradient is rounding noise away from the five pixels, measured against its top
        assert float(np.abs(got - want).max()) <= 1e-10 * top, k
        checked += 1
    assert checked == 3 * 16 + 2 * 110 + 2 * 10 + 2 * (2 * 2 * 5) + 2 * 2
    for name in ("l1", "l2"):
        assert "e5_c3_weight_chw_%s_dx" % name in GOLD and "x0_negw_%s_dx" % name in GOLD
    x, t, mask, w = me.extreme_inputs(me.EXTREME_CASES.index(((6, 33, 47), "negw")))
    assert float(w.min()) < -1 and float(GOLD["x0_negw_l2"]) != 0.0
    inside = mask.expand_as(x).numpy() & (w.expand_as(x).numpy() < 0)
    d = (x - t).numpy()[inside]
    assert (np.sign(GOLD["x0_negw_l1_dx"][inside]) == np.sign(d)).all()            # sign(d) |w|, not sign(d) w
    assert (np.sign(GOLD["x0_negw_l2_dx"][inside]) == -np.sign(d)).all()


@pytest.mark.parametrize("index", [me.PHOTO_CASES.index((33, 33, "near")), me.PHOTO_CASES.index((70, 75, "delta"))],
                         ids=["33x33-near", "70x75-delta"])
def test_sign_plus_ssim_gradient_is_the_autograd_gradient_for_every_upstream_row(index):
    img, gt = (v.double() for v in me.photo_inputs(index))
    sign_over_n = me.l1_gradient(img, gt)
    for lam, u, v in me.UPSTREAM:
        x = img.clone().requires_grad_(True)
        loss, l1 = lr.photometric_loss(x, gt, lam)
        (u * loss + v * l1).backward()
        a, b = u * (1.0 - lam) + v, -u * lam
        want = a * sign_over_n + b * GOLD[f"p{index}_grad_ssim"]
        assert float(np.abs(x.grad.numpy() - want).max()) <= 1e-10 * float(np.abs(want).max()), (lam, u, v)


def test_bands():
    b = me.bands(70, 75)
    assert set(b) == set(me.BANDS) and all(v.shape == (70, 75) and v.dtype == bool for v in b.values())
    assert b["border"].sum() == 70 * 75 - 60 * 65 and b["corners"].sum() == 100 and not (b["corners"] & ~b["border"]).any()
    rows = [y for y in range(70) if b["seam"][y, 16]]
    assert rows == [0, 1, 2, 3, 4, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 59, 60, 61, 62, 63, 64, 65, 66, 67, 68]
    assert all(v.all() for v in me.bands(5, 5).values()) and not me.bands(11, 11)["border"][5, 5]
    for c, y, x in me.delta_pixels(70, 75):
        assert b["seam"][y, x] or b["corners"][y, x]


def test_stored_fp32_deviations_are_what_an_fp32_run_gives(restated):
    """v32 / e32 are rounding noise of an fp32 run of the same torch operations; the restatement's fp32 run on this machine
    gives the same figures up to the order of a few operations: within a factor of 2, or under one fp32 ulp (1.2e-7)"""
    keys = [k for k in sorted(GOLD) if NOISE(k)]
    assert len(keys) == 16 * (4 + 2 * 4) + 2 * (2 * 2 * 5) + 2 * 2
    for k in keys:
        stored, here = float(GOLD[k]), float(restated[k])
        assert 0.0 <= stored < 1e-3, k
        assert abs(stored - here) <= max(0.5 * max(stored, here), 1.2e-7), (k, stored, here)
