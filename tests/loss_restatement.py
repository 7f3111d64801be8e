"""The reference's image losses (utils/loss_utils.py:17-73: l1_loss, l2_loss, ssim) restated in plain torch, in whatever
dtype and on whatever device the inputs have.  The CPU-side check of opengaussian_amd.losses (tests/test_losses_host.py pins
it to goldens produced by the reference's own functions, in fp64 to 1e-10) and the torch baseline of
scripts/photometric_loss_bench.py.

The 2-D window is the OUTER PRODUCT OF THE fp32 1-D WEIGHTS, ROUNDED TO fp32, and only then cast to the image's dtype -- that is
what the reference convolves with, also in an fp64 run.
"""
from math import exp

import torch
import torch.nn.functional as F

WINDOW, SIGMA, C1, C2 = 11, 1.5, 0.01 ** 2, 0.03 ** 2


def window_1d():
    g = torch.tensor([exp(-(i - WINDOW // 2) ** 2 / (2.0 * SIGMA ** 2)) for i in range(WINDOW)], dtype=torch.float32)
    return g / g.sum()


def ssim_map(img, gt):
    """[.., C, H, W] -> the per-pixel SSIM map [1, C, H, W]; zero padding of 5, weights not renormalised at the border."""
    C, H, W = img.shape[-3:]
    x, y = img.reshape(1, C, H, W), gt.reshape(1, C, H, W)
    g = window_1d()
    w = torch.outer(g, g).to(device=x.device, dtype=x.dtype).expand(C, 1, WINDOW, WINDOW).contiguous()
    blur = lambda t: F.conv2d(t, w, padding=WINDOW // 2, groups=C)
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))


def ssim(img, gt):
    return ssim_map(img, gt).mean()


def l1_loss(x, gt, mask=None, weight=None):
    d = x - gt
    if mask is None:
        return d.abs().mean()
    w = mask if weight is None else mask * weight
    return (d * w).abs().sum() / mask.sum().clamp(min=1)


def l2_loss(x, gt, mask=None, weight=None):
    d2 = (x - gt) ** 2
    if mask is None:
        return d2.mean()
    w = mask if weight is None else mask * weight
    return (d2 * w).sum() / mask.sum().clamp(min=1)


def photometric_loss(img, gt, lambda_dssim):
    """train.py:385-386 -> (loss, Ll1)"""
    l1 = l1_loss(img, gt)
    return (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ssim(img, gt)), l1
