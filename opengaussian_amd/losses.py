"""Full-frame image losses of OpenGaussian's stage 0 and stage 2 as fused HIP kernels (include/ogs_loss.h).

Same names, arguments and results as the reference's
  utils/loss_utils.py:17-23    l1_loss(network_output, gt, mask=None, weight=None)
  utils/loss_utils.py:25-31    l2_loss(network_output, gt, mask=None, weight=None)
  utils/loss_utils.py:43-73    ssim(img1, img2, window_size=11, size_average=True)
plus ``photometric_loss(image, gt, lambda_dssim) -> (loss, Ll1)``, the one-forward, one-backward form of
train.py:385-386.  Window (11 taps, sigma 1.5, fp32 weights), zero padding of 5 and C1 / C2 are the reference's.
Each is differentiable with respect to its FIRST argument only.

HIP path: fp32 results; [3,H,W] and [1,3,H,W] images for ssim / photometric_loss; [C,H,W] / [1,C,H,W] with C = 3 or 6 for
the masked losses (any shape without a mask); masks of dtype bool (or integer / float holding only 0 and 1) and shape [H,W],
[1,H,W] or [C,H,W]; a weight of the mask's shape.  Inputs that are not contiguous fp32 are made so.  CPU tensors raise:
there is no CPU path.

Plain-torch fallbacks (no train.py call site uses them; they run wherever their tensors live):
  * ssim with window_size != 11, size_average=False, a channel count other than 3, or a batch of more than one image;
  * a gt, mask or weight that requires grad;
  * a non-bool mask holding anything but 0 and 1 (the reference multiplies by the mask's values; finding this out costs a
    non-bool mask one device-to-host read per call);
  * a mask or weight of another shape (general broadcasting), C other than 3 or 6 with a mask, gt of another shape.
"""
from __future__ import annotations

from math import exp

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, ptr


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); the MI355X image losses have no CPU path")


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _scalar_ptr(g):
    """Device pointer of an upstream 0-dim gradient (None stays NULL = 0); the tensor is returned to keep it alive."""
    if g is None:
        return None, None
    g = g.to(torch.float32).contiguous()
    return g, g.data_ptr()


# ---- plain-torch compositions (fallbacks) -----------------------------------------------------------------------------
def _l1_torch(x, gt, mask=None, weight=None):
    if mask is None:
        return (x - gt).abs().mean()
    w = torch.ones_like(mask) if weight is None else weight
    return ((x - gt) * mask * w).abs().sum() / mask.sum().clamp(min=1)


def _l2_torch(x, gt, mask=None, weight=None):
    if mask is None:
        return ((x - gt) ** 2).mean()
    w = torch.ones_like(mask) if weight is None else weight
    return ((x - gt) ** 2 * mask * w).sum() / mask.sum().clamp(min=1)


def _window_torch(window_size, channel, like):
    g = torch.tensor([exp(-(i - window_size // 2) ** 2 / (2.0 * 1.5 ** 2)) for i in range(window_size)], dtype=torch.float32)
    g = (g / g.sum())[:, None]
    return (g @ g.t()).expand(channel, 1, window_size, window_size).contiguous().to(device=like.device, dtype=like.dtype)


def _ssim_torch(img1, img2, window_size=11, size_average=True):
    ch, pad = img1.size(-3), window_size // 2
    win = _window_torch(window_size, ch, img1)
    blur = lambda t: F.conv2d(t, win, padding=pad, groups=ch)
    mu1, mu2 = blur(img1), blur(img2)
    s11, s22, s12 = blur(img1 * img1) - mu1 * mu1, blur(img2 * img2) - mu2 * mu2, blur(img1 * img2) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    smap = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))
    return smap.mean() if size_average else smap.mean(1).mean(1).mean(1)


# ---- photometric pair ------------------------------------------------------------------------------------------------
class _Photometric(torch.autograd.Function):
    """(loss, l1, ssim) of one [3,H,W] pair from ogs_loss_photometric_forward; backward recomputes the SSIM partials."""

    @staticmethod
    def forward(ctx, img, gt, lambda_dssim):
        lib = _lib.lib()
        a, b = _f32(img).reshape(img.shape[-3:]), _f32(gt).reshape(gt.shape[-3:])
        C, H, W = (int(v) for v in a.shape)
        out = torch.empty(5, dtype=torch.float32, device=a.device)
        tmp = torch.empty(lib.ogs_loss_photometric_tmp_bytes(C, H, W), dtype=torch.uint8, device=a.device)
        check(lib.ogs_loss_photometric_forward(ptr(a), ptr(b), C, H, W, float(lambda_dssim), ptr(out), ptr(tmp), _stream()),
              "ogs_loss_photometric_forward")
        ctx.save_for_backward(a, b)
        ctx.lam = float(lambda_dssim)
        ctx.in_shape, ctx.in_dtype = tuple(img.shape), img.dtype
        ctx.set_materialize_grads(False)
        parts = out.unbind(0)
        return parts[4], parts[2], parts[3]

    @staticmethod
    def backward(ctx, g_loss, g_l1, g_ssim):
        if not ctx.needs_input_grad[0] or (g_loss is None and g_l1 is None and g_ssim is None):
            return None, None, None
        a, b = ctx.saved_tensors
        C, H, W = (int(v) for v in a.shape)
        (k0, p_loss), (k1, p_l1), (k2, p_ssim) = _scalar_ptr(g_loss), _scalar_ptr(g_l1), _scalar_ptr(g_ssim)
        dimg = torch.empty_like(a)
        check(_lib.lib().ogs_loss_photometric_backward(ptr(a), ptr(b), p_l1, p_ssim, p_loss, ctx.lam, C, H, W, ptr(dimg),
                                                       _stream()), "ogs_loss_photometric_backward")
        del k0, k1, k2
        return dimg.reshape(ctx.in_shape).to(ctx.in_dtype), None, None


def _photometric_served(img, gt) -> bool:
    """[3,H,W] or [1,3,H,W], gt of the same shape and outside the graph."""
    if img.dim() not in (3, 4) or img.shape != gt.shape or gt.requires_grad:
        return False
    if img.dim() == 4 and img.shape[0] != 1:
        return False
    return img.shape[-3] == 3 and img.shape[-1] >= 1 and img.shape[-2] >= 1


def photometric_loss(image, gt, lambda_dssim):
    """(loss, Ll1) with Ll1 = l1_loss(image, gt) and loss = (1 - lambda) Ll1 + lambda (1 - ssim(image, gt)), train.py:385-386,
    from one forward and one backward launch pair.  Ll1 comes back because training_report logs it."""
    if not _photometric_served(image, gt):
        l1 = _l1_torch(image, gt)
        return (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - _ssim_torch(image, gt)), l1
    _need_gpu(image, "image")
    loss, l1, _ = _Photometric.apply(image, gt.to(image.device), float(lambda_dssim))
    return loss, l1


def ssim(img1, img2, window_size=11, size_average=True):
    """Mean SSIM (utils/loss_utils.py:43-73).  Fallbacks: see the module docstring."""
    if window_size != 11 or not size_average or not _photometric_served(img1, img2):
        return _ssim_torch(img1, img2, window_size, size_average)
    _need_gpu(img1, "img1")
    return _Photometric.apply(img1, img2.to(img1.device), 0.0)[2]


# ---- masked pair -----------------------------------------------------------------------------------------------------
class _Masked(torch.autograd.Function):
    """out[2] of ogs_loss_masked_forward: num / clamp(sum mask, 1), or the plain mean without a mask."""

    @staticmethod
    def forward(ctx, x, t, mask_u8, weight, mask_channels, p):
        lib = _lib.lib()
        a, b = _f32(x), _f32(t)
        if mask_u8 is None:
            C, HW = 1, a.numel()
        else:
            C, HW = int(a.shape[-3]), int(a.shape[-2]) * int(a.shape[-1])
        w = None if weight is None else _f32(weight)
        out = torch.empty(3, dtype=torch.float32, device=a.device)
        tmp = torch.empty(lib.ogs_loss_masked_tmp_bytes(), dtype=torch.uint8, device=a.device)
        check(lib.ogs_loss_masked_forward(ptr(a), ptr(b), ptr(mask_u8), ptr(w), int(mask_channels), int(p), C, HW, ptr(out),
                                          ptr(tmp), _stream()), "ogs_loss_masked_forward")
        ctx.save_for_backward(a, b, mask_u8, w, out)
        ctx.args = (int(mask_channels), int(p), C, HW)
        ctx.in_shape, ctx.in_dtype = tuple(x.shape), x.dtype
        ctx.set_materialize_grads(False)
        return out[2]

    @staticmethod
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        a, b, mask_u8, w, out = ctx.saved_tensors
        mask_channels, p, C, HW = ctx.args
        keep, gp = _scalar_ptr(g)
        dx = torch.empty_like(a)
        check(_lib.lib().ogs_loss_masked_backward(ptr(a), ptr(b), ptr(mask_u8), ptr(w), mask_channels, p, C, HW, ptr(out), gp,
                                                  ptr(dx), _stream()), "ogs_loss_masked_backward")
        del keep
        return dx.reshape(ctx.in_shape).to(ctx.in_dtype), None, None, None, None, None


def _strip(shape):
    s = tuple(int(v) for v in shape)
    while len(s) > 2 and s[0] == 1:
        s = s[1:]
    return s


def _mask_channels(x, gt, mask, weight):
    """1 or C when the HIP path serves this (x, gt, mask, weight) layout, None otherwise.  Looks at no tensor contents."""
    if x.dim() not in (3, 4) or x.shape != gt.shape or gt.requires_grad or mask.requires_grad:
        return None
    xs = _strip(x.shape)
    if len(xs) != 3 or xs[0] not in (3, 6):
        return None
    ms = _strip(mask.shape)
    if ms != xs[1:] and ms != xs:
        return None
    if weight is not None and (weight.requires_grad or _strip(weight.shape) != ms):
        return None
    return 1 if ms == xs[1:] else xs[0]


def _mask_bytes(mask):
    """Contiguous uint8 0/1, or None for a non-bool mask holding other values (the reference multiplies by them)."""
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)
    if not bool(((mask == 0) | (mask == 1)).all()):
        return None
    return (mask != 0).to(torch.uint8).contiguous()


def _masked_loss(p, fallback, network_output, gt, mask, weight):
    if mask is None:
        if network_output.shape != gt.shape or gt.requires_grad:
            return fallback(network_output, gt)
        _need_gpu(network_output, "network_output")
        return _Masked.apply(network_output, gt.to(network_output.device), None, None, 0, p)
    channels = _mask_channels(network_output, gt, mask, weight)
    if channels is None:
        return fallback(network_output, gt, mask, weight)
    m = _mask_bytes(mask)
    if m is None:
        return fallback(network_output, gt, mask, weight)
    _need_gpu(network_output, "network_output")
    dev = network_output.device
    return _Masked.apply(network_output, gt.to(dev), m.to(dev), None if weight is None else weight.to(dev), channels, p)


def l1_loss(network_output, gt, mask=None, weight=None):
    """utils/loss_utils.py:17-23: mean |x - gt|, or sum |(x - gt) mask weight| / clamp(sum mask, 1) with the sum of the
    mask taken over the mask's own elements.  Fallbacks: see the module docstring."""
    return _masked_loss(1, _l1_torch, network_output, gt, mask, weight)


def l2_loss(network_output, gt, mask=None, weight=None):
    """utils/loss_utils.py:25-31: mean (x - gt)^2, or sum (x - gt)^2 mask weight / clamp(sum mask, 1)."""
    return _masked_loss(2, _l2_torch, network_output, gt, mask, weight)
