"""CPU: the torch restatement of the reference's image losses (tests/loss_restatement.py) against goldens produced by the
reference's own functions, and the host side of opengaussian_amd.losses: symbols, refusal of CPU tensors, and the cases
that are documented to go through plain torch (checked with the C library made unreachable)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import loss_restatement as lr
from tests.golden import make_loss_golden as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = mg.load_golden()
LOSS_SYMBOLS = ["ogs_loss_photometric_tmp_bytes", "ogs_loss_photometric_forward", "ogs_loss_photometric_backward",
                "ogs_loss_masked_tmp_bytes", "ogs_loss_masked_forward", "ogs_loss_masked_backward"]


def _rel(got, want, floor=0.0):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(float(np.abs(want).max()), floor))


@pytest.mark.parametrize("index", range(len(mg.PHOTO_CASES)), ids=lambda i: "%dx%d-%s" % mg.PHOTO_CASES[i])
def test_restatement_fp64_reproduces_photometric_goldens(index):
    img, gt = (t.double() for t in mg.photo_inputs(index))
    x = img.clone().requires_grad_(True)
    loss, l1 = lr.photometric_loss(x, gt, mg.LAMBDA)
    loss.backward()
    k = f"p{index}_"
    # "same": the golden loss is 0 and its gradient rounding noise (1e-18); the floors are the unit of one pixel's share
    n = img.numel()
    assert _rel(l1.item(), GOLD[k + "l1"], 1.0 / n) <= 1e-10
    assert _rel(lr.ssim(img, gt).item(), GOLD[k + "ssim"]) <= 1e-10
    assert _rel(loss.item(), GOLD[k + "loss"], 1.0 / n) <= 1e-10
    assert _rel(x.grad.numpy(), GOLD[k + "grad"], 1.0 / n) <= 1e-10


@pytest.mark.parametrize("index", range(len(mg.MASKED_CASES)), ids=mg.masked_key)
def test_restatement_fp64_reproduces_masked_goldens(index):
    x, t, mask, weight = mg.masked_inputs(index)
    x, t = x.double(), t.double()
    weight = None if weight is None else weight.double()
    for name, fn in (("l1", lr.l1_loss), ("l2", lr.l2_loss)):
        xx = x.clone().requires_grad_(True)
        v = fn(xx, t, mask, weight)
        v.backward()
        k = f"{mg.masked_key(index)}_{name}"
        assert _rel(v.item(), GOLD[k], 1.0 / x.numel()) <= 1e-10
        assert _rel(xx.grad.numpy(), GOLD[k + "_dx"], 1.0 / x.numel()) <= 1e-10


def test_golden_e32_is_the_fp32_runs_own_deviation():
    for i, (H, W, kind) in enumerate(mg.PHOTO_CASES):
        g64, g32 = GOLD[f"p{i}_grad"], GOLD[f"p{i}_f32_grad"]
        assert g64.dtype == np.float64 and g32.dtype == np.float32 and g64.shape == (3, H, W)
        assert float(GOLD[f"p{i}_e32"]) == float(np.abs(g32.astype(np.float64) - g64).max() / np.abs(g64).max())


def test_loss_symbols_are_declared_bound_and_exported():
    import ctypes
    from opengaussian_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "ogs_loss.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(ogs_loss_[a-z0-9_]+)\s*\(", hdr, re.M))
    assert declared == set(LOSS_SYMBOLS)
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in LOSS_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    lib = _lib.lib()
    assert lib.ogs_loss_photometric_tmp_bytes(3, 1080, 1920) == 16 * 3 * 34 * 60       # one fp64 pair per 32x32 tile
    assert lib.ogs_loss_masked_tmp_bytes() > 0


def test_cpu_tensors_are_refused():
    from opengaussian_amd import losses
    img, gt = mg.photo_inputs(0)
    x, t, mask, weight = mg.masked_inputs(0)
    for call in (lambda: losses.ssim(img, gt), lambda: losses.photometric_loss(img, gt, 0.2),
                 lambda: losses.ssim(img[None], gt[None]), lambda: losses.l1_loss(img, gt), lambda: losses.l2_loss(img, gt),
                 lambda: losses.l1_loss(x, t, mask), lambda: losses.l2_loss(x, t, mask.float(), torch.rand(1, 33, 47))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_documented_fallbacks_never_reach_the_library(monkeypatch):
    """Every case the docstring lists as plain torch, on CPU tensors, with the C library unreachable."""
    from opengaussian_amd import _lib, losses

    def unreachable():
        raise AssertionError("a fallback case called into libogs_hip")

    monkeypatch.setattr(_lib, "lib", unreachable)
    for phrase in ("window_size != 11", "size_average=False", "channel count other than 3", "requires grad",
                   "anything but 0 and 1", "another shape"):
        assert phrase in losses.__doc__, phrase
    img, gt = mg.photo_inputs(2)
    x, t, mask, weight = mg.masked_inputs(0)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)

    assert torch.isfinite(losses.ssim(img, gt, window_size=7))
    per_image = losses.ssim(img[None], gt[None], size_average=False)
    assert per_image.shape == (1,)
    close(per_image[0], lr.ssim(img, gt))
    close(losses.ssim(img[:1], gt[:1]), lr.ssim(img[:1], gt[:1]))                           # C = 1
    close(losses.ssim(torch.stack([img, gt]), torch.stack([gt, gt])),                     # a batch of two
          lr.ssim_map(img, gt).mean() * 0.5 + 0.5)
    # gt / mask / weight inside the graph
    g = gt.clone().requires_grad_(True)
    close(losses.ssim(img, g), lr.ssim(img, gt))
    loss, l1 = losses.photometric_loss(img, g, 0.2)
    want, want_l1 = lr.photometric_loss(img, gt, 0.2)
    close(loss, want); close(l1, want_l1)
    loss.backward()
    assert g.grad is not None and float(g.grad.abs().max()) > 0
    tg = t.clone().requires_grad_(True)
    close(losses.l1_loss(x, tg), lr.l1_loss(x, t))
    close(losses.l2_loss(x, tg, mask), lr.l2_loss(x, t, mask))
    soft = torch.rand(1, 33, 47).requires_grad_(True)
    close(losses.l1_loss(x, t, soft), lr.l1_loss(x, t, soft))
    wg = torch.rand(1, 33, 47).requires_grad_(True)
    m = mg.masked_inputs(4)[2]
    close(losses.l2_loss(x, t, m, wg), lr.l2_loss(x, t, m, wg))
    # a float mask that is not 0 / 1 multiplies, as in the reference
    two = torch.full((1, 33, 47), 2.0)
    close(losses.l1_loss(x, t, two), lr.l1_loss(x, t, two))
    close(losses.l2_loss(x, t, two.to(torch.int64)), lr.l2_loss(x, t, two.to(torch.int64)))
    # other shapes: a mask that broadcasts along W, 4 channels with a mask, gt of another shape
    col = torch.rand(33, 1) < 0.5
    close(losses.l1_loss(x, t, col), lr.l1_loss(x, t, col))
    x4, t4 = torch.rand(4, 33, 47), torch.rand(4, 33, 47)
    close(losses.l2_loss(x4, t4, mask), lr.l2_loss(x4, t4, mask))
    close(losses.l1_loss(x, t[:1]), lr.l1_loss(x, t[:1]))
