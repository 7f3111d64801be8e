"""GPU: the fused image losses (opengaussian_amd/losses.py -> include/ogs_loss.h) against goldens produced by the
reference's own functions in fp64 (tests/golden/make_loss_golden.py).

Bounds.  Values: 2e-5 relative (the convention of test_30_mask_gpu.py; the reference's own fp32 run is within 3.5e-6 of its
fp64 run).  Gradients: max(1e-4, 4 * e32) of the largest golden entry, where e32 is the deviation of the reference's own
fp32 gradient from its fp64 gradient, READ FROM THE GOLDEN FILE; 1e-4 is the project's gradient floor and the factor 4
allows for a different summation order, nothing more.
"""
import types

import numpy as np
import pytest
import torch

from tests import helpers
from tests import loss_restatement as lr
from tests.golden import make_loss_golden as mg

pytestmark = pytest.mark.gpu
GOLD = mg.load_golden()
PHOTO_IDS = ["%dx%d-%s" % c for c in mg.PHOTO_CASES]
SAME = [i for i, c in enumerate(mg.PHOTO_CASES) if c[2] == "same"]
REGULAR = [i for i in range(len(mg.PHOTO_CASES)) if i not in SAME]


def _value_ok(got, want, what):
    got = float(got.detach()) if torch.is_tensor(got) else float(got)
    want = float(want.detach()) if torch.is_tensor(want) else float(want)
    print(f"{what}: got {got:.9g} want {want:.9g} rel {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) <= 2e-5 * abs(want), what


def _grad_ok(got, want, e32, what):
    want = np.asarray(want, np.float64)
    bound = max(1e-4, 4.0 * float(e32))
    err = float(np.abs(got.detach().cpu().double().numpy() - want).max() / np.abs(want).max())
    print(f"{what}: grad err {err:.2e} of max, bound {bound:.2e}")
    assert err <= bound, what


@pytest.mark.parametrize("index", REGULAR, ids=[PHOTO_IDS[i] for i in REGULAR])
def test_photometric_values_and_gradient_match_fp64_goldens(gpu_device, index):
    from opengaussian_amd import losses
    img, gt = (t.to(gpu_device) for t in mg.photo_inputs(index))
    k = f"p{index}_"
    x = img.clone().requires_grad_(True)
    loss, l1 = losses.photometric_loss(x, gt, mg.LAMBDA)
    loss.backward()
    ss, l1_alone = losses.ssim(img, gt), losses.l1_loss(img, gt)
    _value_ok(ss, GOLD[k + "ssim"], "ssim")
    _value_ok(l1_alone, GOLD[k + "l1"], "l1_loss")
    _value_ok(l1, GOLD[k + "l1"], "Ll1")
    _value_ok(loss, GOLD[k + "loss"], "photometric_loss")
    assert x.grad.shape == img.shape and torch.isfinite(x.grad).all()
    _grad_ok(x.grad, GOLD[k + "grad"], GOLD[k + "e32"], "d loss / d image")
    # the fused form is the composition of the separate drop-ins
    composed = (1.0 - mg.LAMBDA) * float(l1_alone) + mg.LAMBDA * (1.0 - float(ss))
    assert abs(float(loss.detach()) - composed) <= 1e-6


@pytest.mark.parametrize("index", SAME, ids=[PHOTO_IDS[i] for i in SAME])
def test_identical_images_give_zero_loss_and_a_negligible_gradient(gpu_device, index):
    """1e-6 is under 1 % of the (1 - lambda) / (CHW) L1 step of one differing pixel at 3 x 40 x 40."""
    from opengaussian_amd import losses
    img, gt = (t.to(gpu_device) for t in mg.photo_inputs(index))
    assert torch.equal(img, gt)
    x = img.clone().requires_grad_(True)
    loss, l1 = losses.photometric_loss(x, gt, mg.LAMBDA)
    loss.backward()
    print("same: loss %.3e l1 %.3e largest gradient entry %.3e" % (float(loss.detach()), float(l1.detach()), float(x.grad.abs().max())))
    assert abs(float(loss.detach())) <= 1e-6 and float(l1.detach()) == 0.0
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) <= 1e-6


@pytest.mark.parametrize("index", [2, 4, 8], ids=[PHOTO_IDS[i] for i in (2, 4, 8)])
def test_upstream_scalars_reach_both_terms(gpu_device, index):
    """(3 ssim + 2 l1).backward() against the restatement on the GPU in fp64"""
    from opengaussian_amd import losses
    img, gt = (t.to(gpu_device) for t in mg.photo_inputs(index))
    x = img.clone().requires_grad_(True)
    (3.0 * losses.ssim(x, gt) + 2.0 * losses.l1_loss(x, gt)).backward()
    x64 = img.double().requires_grad_(True)
    (3.0 * lr.ssim(x64, gt.double()) + 2.0 * lr.l1_loss(x64, gt.double())).backward()
    _grad_ok(x.grad, x64.grad.cpu().numpy(), GOLD[f"p{index}_e32"], "3 ssim + 2 l1")


@pytest.mark.parametrize("index", range(len(mg.MASKED_CASES)), ids=mg.masked_key)
def test_masked_losses_match_fp64_goldens(gpu_device, index):
    from opengaussian_amd import losses
    x, t, mask, weight = (None if v is None else v.to(gpu_device) for v in mg.masked_inputs(index))
    for name, fn in (("l1", losses.l1_loss), ("l2", losses.l2_loss)):
        k = f"{mg.masked_key(index)}_{name}"
        xx = x.clone().requires_grad_(True)
        v = fn(xx, t, mask, weight)
        v.backward()
        want, want_dx = float(GOLD[k]), GOLD[k + "_dx"]
        assert xx.grad.shape == x.shape
        if mask is not None:
            outside = ~mask.expand_as(x) if mask.dim() == 3 else ~mask[None].expand_as(x)
            assert bool(outside.any()) and float(xx.grad[outside].abs().max()) == 0.0       # exactly 0 outside the mask
        if want == 0.0:                                   # the all-false mask: the clamp bites, nothing flows
            assert float(v.detach()) == 0.0 and float(xx.grad.abs().max()) == 0.0
            continue
        _value_ok(v, want, k)
        _grad_ok(xx.grad, want_dx, GOLD[k + "_e32"], k)


def test_mask_dtypes_layouts_and_batched_inputs(gpu_device):
    from opengaussian_amd import losses
    index = mg.MASKED_CASES.index(((6, 33, 47), "one_hw"))
    x, t, mask, _ = (v if v is None else v.to(gpu_device) for v in mg.masked_inputs(index))
    want, want_dx, e32 = float(GOLD["m0_one_hw_l1"]), GOLD["m0_one_hw_l1_dx"], GOLD["m0_one_hw_l1_e32"]
    for m in (mask, mask.to(torch.uint8), mask.float(), mask[0], mask[0].to(torch.int64)):
        _value_ok(losses.l1_loss(x, t, m), want, f"mask {m.dtype} {tuple(m.shape)}")
    # a non-contiguous x (a permuted [H,W,C] buffer) and the [1,C,H,W] form, values and gradients
    hwc = x.permute(1, 2, 0).contiguous().requires_grad_(True)
    xv = hwc.permute(2, 0, 1)
    assert not xv.is_contiguous()
    v = losses.l1_loss(xv, t, mask)
    v.backward()
    _value_ok(v, want, "non-contiguous x")
    _grad_ok(hwc.grad.permute(2, 0, 1), want_dx, e32, "non-contiguous x")
    xb = x[None].clone().requires_grad_(True)
    v = losses.l1_loss(xb, t[None], mask)
    v.backward()
    _value_ok(v, want, "[1,C,H,W]")
    assert xb.grad.shape == xb.shape
    _grad_ok(xb.grad[0], want_dx, e32, "[1,C,H,W]")
    # photometric: [1,3,H,W] and a non-contiguous fp64 image
    img, gt = (u.to(gpu_device) for u in mg.photo_inputs(2))
    xb = img[None].clone().requires_grad_(True)
    loss, _ = losses.photometric_loss(xb, gt[None], mg.LAMBDA)
    loss.backward()
    _value_ok(loss, GOLD["p2_loss"], "[1,3,H,W]")
    assert xb.grad.shape == xb.shape
    _grad_ok(xb.grad[0], GOLD["p2_grad"], GOLD["p2_e32"], "[1,3,H,W]")
    hwc = img.double().permute(1, 2, 0).contiguous().requires_grad_(True)
    loss, _ = losses.photometric_loss(hwc.permute(2, 0, 1), gt, mg.LAMBDA)
    loss.backward()
    _value_ok(loss, GOLD["p2_loss"], "non-contiguous fp64 image")
    assert hwc.grad.dtype == torch.float64
    _grad_ok(hwc.grad.permute(2, 0, 1), GOLD["p2_grad"], GOLD["p2_e32"], "non-contiguous fp64 image")


def test_two_calls_give_the_same_bits(gpu_device):
    from opengaussian_amd import losses
    img, gt = (t.to(gpu_device) for t in mg.photo_inputs(4))
    x, t, mask, weight = (v if v is None else v.to(gpu_device) for v in mg.masked_inputs(4))

    def once():
        a = img.clone().requires_grad_(True)
        loss, l1 = losses.photometric_loss(a, gt, mg.LAMBDA)
        loss.backward()
        b = x.clone().requires_grad_(True)
        v = losses.l2_loss(b, t, mask, weight)
        v.backward()
        return [loss.detach(), l1.detach(), a.grad, v.detach(), b.grad]

    for u, w in zip(once(), once()):
        assert torch.equal(u, w)


def test_stage0_step_through_the_rasterizer(gpu_device):
    """One stage-0 step in the shape of test_60_integration_gpu.py: render() -> photometric_loss -> backward through the
    rasterizer, against the same step with the fp32 torch restatement.  2e-4 of the largest entry: the gradient tolerance of
    that file's comparisons (helpers.assert_grad_family_close's default)."""
    from opengaussian_amd import losses
    from opengaussian_amd.renderer import render
    from tests.test_60_integration_gpu import _Model
    dev = gpu_device
    W, H, f, P = 160, 112, 120.0, 5000
    sc, cam = helpers.tiny_scene(P, W, H, f, seed=5, log_scale_mean=-3.0)
    cam = cam.to(dev)
    target_sc, _ = helpers.tiny_scene(P, W, H, f, seed=6, log_scale_mean=-3.0)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        target = render(cam, _Model(target_sc, dev), pipe, bg, iteration=0, rescale=False, render_feat_map=False)["render"]

    def step(loss_fn):
        m = _Model(sc, dev)
        out = render(cam, m, pipe, bg, iteration=1, rescale=False, render_feat_map=False)
        loss, l1 = loss_fn(out["render"], target, 0.2)
        loss.backward()
        return float(loss), m._xyz.grad.clone(), m._features_dc.grad.clone()

    got, want = step(losses.photometric_loss), step(lr.photometric_loss)
    assert abs(got[0] - want[0]) <= 2e-5 * abs(want[0])
    for a, b, what in ((got[1], want[1], "_xyz.grad"), (got[2], want[2], "_features_dc.grad")):
        err = float((a - b).abs().max() / b.abs().max())
        print(f"{what}: {err:.2e} of max")
        assert torch.isfinite(a).all() and err <= 2e-4, what


def test_full_hd_against_fp64_restatement(gpu_device):
    """1080 x 1920: indexing past 2^20 pixels, 6120 partial pairs in the second-stage reduce."""
    from opengaussian_amd import losses
    H, W = 1080, 1920
    g = torch.Generator().manual_seed(77)
    coarse = torch.rand(1, 3, H // 8 + 2, W // 8 + 2, generator=g)
    gt = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[0]
    gt = (gt + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1).to(gpu_device)
    img = (gt + 0.03 * torch.randn(3, H, W, generator=g).to(gpu_device)).clamp(0, 1)
    x = img.clone().requires_grad_(True)
    loss, l1 = losses.photometric_loss(x, gt, mg.LAMBDA)
    loss.backward()
    x64 = img.double().requires_grad_(True)
    want, want_l1 = lr.photometric_loss(x64, gt.double(), mg.LAMBDA)
    want.backward()
    _value_ok(loss, want, "loss 1080p")
    _value_ok(l1, want_l1, "Ll1 1080p")
    _grad_ok(x.grad, x64.grad.cpu().numpy(), 0.0, "d loss / d image 1080p")
    # the masked pair at the same size, [1,H,W] mask over 6 channels
    xm, tm = torch.rand(6, H, W, generator=g).to(gpu_device), torch.rand(6, H, W, generator=g).to(gpu_device)
    mask = (torch.rand(1, H, W, generator=g) < 0.5).to(gpu_device)
    xx = xm.clone().requires_grad_(True)
    v = losses.l1_loss(xx, tm, mask)
    v.backward()
    x64 = xm.double().requires_grad_(True)
    want = lr.l1_loss(x64, tm.double(), mask)
    want.backward()
    _value_ok(v, want, "masked l1 1080p")
    _grad_ok(xx.grad, x64.grad.cpu().numpy(), 0.0, "masked l1 dx 1080p")
