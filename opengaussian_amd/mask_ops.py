"""Image-space mask reductions of OpenGaussian's stage-1 / association losses.

Same names, arguments and results as the reference's
  utils/opengs_utlis.py:90-123    calculate_iou
  utils/opengs_utlis.py:181-197   pair_mask_feature_mean
  utils/opengs_utlis.py:240-283   mask_feature_mean
  train.py:102-122                cohesion_loss
  train.py:124-155                separation_loss
  utils/opengs_utlis.py:125-182   get_SAM_mask_and_feat   (returns a LabelMasks in place of the one-hot stack)
but without the [num_mask, C, H, W] expansions: the two hot ones (mask_feature_mean, cohesion_loss, called every
stage-1 step, train.py:450-452) are segmented reductions in HIP (include/ogs_mask.h) with hand-written
backward passes; the others are small and stay plain torch on the GPU.  No CPU path: CPU tensors raise.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import check, ptr


TABLE_STRIDE = 16      # OGS_MASK_TABLE_STRIDE


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); the MI355X mask reductions have no CPU path")


def _mask_bytes(masks: torch.Tensor) -> torch.Tensor:
    """[N,H,W] masks of any dtype / layout (bool stacks, the permuted int64 one-hot of get_SAM_mask_and_feat,
    opengs_utlis.py:147-149) -> contiguous uint8 0/1."""
    if masks.dtype == torch.bool and masks.is_contiguous():
        return masks.view(torch.uint8)
    if masks.dtype == torch.uint8 and masks.is_contiguous():
        return masks
    return (masks != 0).to(torch.uint8).contiguous()


class LabelMasks:
    """A disjoint [N, H, W] mask stack held as ONE int32 label image: pixel (y, x) lies in mask labels[y, x] - 1 when
    1 <= labels[y, x] <= num_mask and in no mask otherwise (0 = invalid pixel).  mask_feature_mean and cohesion_loss
    take it in place of the stack and then read 4 bytes per pixel of masks whatever N is; `dense()` gives the rows to
    any other consumer.  Not a tensor."""

    def __init__(self, labels: torch.Tensor, num_mask: int):
        if labels.dim() != 2:
            raise RuntimeError(f"LabelMasks: labels must be [H, W], got {tuple(labels.shape)}")
        self.labels = labels.to(torch.int32).contiguous()
        self.num_mask = int(num_mask)

    @property
    def shape(self):
        return (self.num_mask, int(self.labels.shape[0]), int(self.labels.shape[1]))

    def __len__(self):
        return self.num_mask

    def to(self, device):
        return LabelMasks(self.labels.to(device), self.num_mask)

    def dense(self) -> torch.Tensor:
        """The bool stack [N, H, W]."""
        ids = torch.arange(1, self.num_mask + 1, dtype=torch.int32, device=self.labels.device)
        return self.labels[None] == ids[:, None, None]


def get_SAM_mask_and_feat(gt_sam_mask, level=3, filter_th=50, original_mask_feat=None, sample_mask=False):
    """The reference's per-iteration mask preparation (utils/opengs_utlis.py:125-182; train.py:441) without its
    [H, W, num_mask + 1] int64 one-hot (1.6 GB written and read back per step at 1080p with 96 masks).
    gt_sam_mask [4, H, W]: mask ids, each level's ids continuing after the previous level's maximum, -1 = no mask.
    Returns (mask_id [H, W] int64 with 0 = invalid, masks, invalid_pix [H, W] bool), or with `original_mask_feat`
    (mask_id, masks, mask_feat, invalid_pix), values as the reference's -- except that `masks` is a LabelMasks with
    num_mask = mask_id.max() where the reference returns mask_bool [num_mask, H, W]: mask_feature_mean and
    cohesion_loss take it as it is, `masks.dense()` is the stack.  Nothing of size num_mask * H * W is allocated; the
    two maxima it needs come back in ONE device-to-host read.  Runs on the device of its input (CPU included).
    filter_th / sample_mask are accepted and unused, as in the reference."""
    cur = gt_sam_mask[level]
    if level > 0:
        prev_max, cur_max = torch.stack([gt_sam_mask[level - 1].max(), cur.max()]).tolist()
    else:
        prev_max, cur_max = None, cur.max().item()
    # ids of this level: -1, 0 .. num_mask-1  ->  0 (invalid), 1 .. num_mask
    offset = 0 if prev_max is None else prev_max + 1
    mask_id = ((cur - offset).clamp_min(-1) + 1).to(torch.int64)
    num_mask = max(int(cur_max - offset), -1) + 1
    invalid_pix = mask_id == 0
    masks = LabelMasks(mask_id, num_mask)
    if original_mask_feat is not None:
        min_ind = 0 if prev_max is None else int(prev_max) + 1
        mask_feat = original_mask_feat[min_ind:int(cur_max) + 1, :].clone()
        return mask_id, masks, mask_feat, invalid_pix
    return mask_id, masks, invalid_pix


def _membership(masks, device):
    """(membership tensor, N, form) of a mask argument, as the ogs_{form}_* entry points take it: the int32 label image
    of a LabelMasks ("label"), or the contiguous uint8 stack of anything else ("mask")"""
    if isinstance(masks, LabelMasks):
        m = masks.to(device)
        return m.labels, m.num_mask, "label"
    m = _mask_bytes(masks.to(device))
    return m, int(m.shape[0]), "mask"


class _Sums(torch.autograd.Function):
    """table [N, C+1] of weighted per-mask feature sums | weighted counts (ogs_{form}_feature_sums).  `for_var`: the call
    belongs to mask_feature_mean(return_var=True), which is not differentiable."""

    @staticmethod
    def forward(ctx, feat_map, member, N, form, weight, for_var):
        f = feat_map.detach().to(torch.float32).contiguous()
        C, H, W = (int(x) for x in f.shape)
        w = None if weight is None else weight.detach().to(torch.float32).reshape(H, W).contiguous()
        table = torch.empty(N, TABLE_STRIDE, dtype=torch.float32, device=f.device)   # 64-byte rows (ogs_mask.h)
        name = f"ogs_{form}_feature_sums"
        check(getattr(_lib.lib(), name)(ptr(f), ptr(member), ptr(w), C, N, H * W, 0, ptr(table), _stream()), name)
        ctx.save_for_backward(member, w, f)
        ctx.shape = (C, H, W, N)
        ctx.form = form
        ctx.weight_shape = None if weight is None else tuple(weight.shape)
        ctx.for_var = bool(for_var)
        return table[:, :C + 1]

    @staticmethod
    def backward(ctx, g_table):
        if ctx.for_var:
            raise RuntimeError("mask_feature_mean(return_var=True) is not differentiable here (the reference only "
                               "uses it under no_grad, train.py:689)")
        member, w, f = ctx.saved_tensors
        C, H, W, N = ctx.shape
        # d table[n, c] / d feat[c, pix] = mask * w ;  d table[n, c] / d w[pix] = mask * feat[c, pix] ;
        # d table[n, C] / d w[pix] = mask
        coef = g_table[:, :C].to(torch.float32).contiguous()
        need_w = w is not None and ctx.needs_input_grad[4]
        coef_cnt = g_table[:, C].to(torch.float32).contiguous() if need_w else None
        dfeat = torch.empty(C, H, W, dtype=torch.float32, device=g_table.device)
        dweight = torch.empty(H, W, dtype=torch.float32, device=g_table.device) if need_w else None
        name = f"ogs_{ctx.form}_feature_sums_backward"
        check(getattr(_lib.lib(), name)(ptr(member), ptr(w), ptr(coef), ptr(f), ptr(coef_cnt), C, N, H * W, ptr(dfeat),
                                        ptr(dweight), _stream()), name)
        return (dfeat if ctx.needs_input_grad[0] else None, None, None, None,
                dweight.reshape(ctx.weight_shape) if need_w else None, None)


def mask_feature_mean(feat_map, gt_masks, image_mask=None, return_var=False):
    """Average instance feature inside each mask (utils/opengs_utlis.py:240-283).
    feat_map [C=3|6, H, W]; gt_masks [num_mask, H, W] (0/1 of any dtype) or a LabelMasks; image_mask [1,H,W] / [H,W] weights
    (the rendered silhouette, train.py:450) or None.  Returns [num_mask, C]; with return_var=True
    (mean [N,C], variance [N], pixel count [N]) as the reference."""
    _need_gpu(feat_map, "feat_map")
    C, H, W = (int(x) for x in feat_map.shape)
    if tuple(gt_masks.shape[1:]) != (H, W):
        raise RuntimeError(f"gt_masks must be [num_mask, {H}, {W}], got {tuple(gt_masks.shape)}")
    member, N, form = _membership(gt_masks, feat_map.device)
    if image_mask is not None:
        if image_mask.numel() != H * W:
            raise RuntimeError(f"image_mask must have H*W = {H * W} elements, got {tuple(image_mask.shape)}")
        image_mask = image_mask.to(feat_map.device)
    table = _Sums.apply(feat_map, member, N, form, image_mask, bool(return_var))
    counts = table[:, C].clamp(min=1)
    mean = table[:, :C] / counts[:, None]
    if not return_var:
        return mean
    # sum mask*(f - mean)^2 in a second pass over the map, now that the means are known (masked_for_variance, :272-276).
    # Expanded into sum f^2 - 2 mean sum f + count mean^2 it needs one pass only, but cancels: the fp32 atomic sums of a
    # 196 k pixel mask at 0.9 +- 0.05 left the variance anywhere between 8e-6 and 1.4e-4 off from call to call (DESIGN.md
    # section 6b); the deviations from a known mean keep it at 3e-7.
    f = feat_map.detach().to(torch.float32).contiguous()
    w = None if image_mask is None else image_mask.detach().to(torch.float32).reshape(H, W).contiguous()
    mu = mean.detach().contiguous()
    sq = torch.empty(N, TABLE_STRIDE, dtype=torch.float32, device=f.device)
    name = f"ogs_{form}_feature_sqdev"
    check(getattr(_lib.lib(), name)(ptr(f), ptr(member), ptr(w), ptr(mu), C, N, H * W, ptr(sq), _stream()), name)
    return mean, (sq[:, :C] / counts[:, None]).mean(dim=1), counts


class _Cohesion(torch.autograd.Function):
    """mean over the masks of the mean distance to the mask's mean (ogs_{form}_cohesion)"""

    @staticmethod
    def forward(ctx, feat_map, member, N, form, mean):
        f = feat_map.detach().to(torch.float32).contiguous()
        mu = mean.detach().to(torch.float32).contiguous()
        C, H, W = (int(x) for x in f.shape)
        table = torch.empty(N, TABLE_STRIDE, dtype=torch.float32, device=f.device)
        name = f"ogs_{form}_cohesion"
        check(getattr(_lib.lib(), name)(ptr(f), ptr(member), ptr(mu), C, N, H * W, ptr(table), _stream()), name)
        cnt = table[:, 1].clamp(min=1)
        ctx.save_for_backward(f, member, mu, cnt)
        ctx.num_mask, ctx.form = N, form
        return (table[:, 0] / cnt).mean() if N > 0 else table.sum()

    @staticmethod
    def backward(ctx, g):
        f, member, mu, cnt = ctx.saved_tensors
        C, H, W = (int(x) for x in f.shape)
        N = ctx.num_mask
        gl = (g.to(torch.float32) / (max(N, 1) * cnt)).contiguous()
        dfeat = torch.empty(C, H, W, dtype=torch.float32, device=f.device)
        dmean = torch.empty(N, TABLE_STRIDE, dtype=torch.float32, device=f.device)
        name = f"ogs_{ctx.form}_cohesion_backward"
        check(getattr(_lib.lib(), name)(ptr(f), ptr(member), ptr(mu), ptr(gl), C, N, H * W, ptr(dfeat), ptr(dmean),
                                        _stream()), name)
        return dfeat, None, None, None, dmean[:, :C]


def cohesion_loss(feat_map, gt_mask, feat_mean_stack):
    """Intra-mask smoothing loss, Eq. (1) of the paper (train.py:102-122): mean over masks of the mean L2 distance
    between the pixels of a mask and that mask's mean feature."""
    _need_gpu(feat_map, "feat_map")
    return _Cohesion.apply(feat_map, *_membership(gt_mask, feat_map.device), feat_mean_stack)


class _Separation(torch.autograd.Function):
    """loss and dloss/dmeans from ogs_separation_loss (two launches); backward scales the stored gradient."""

    @staticmethod
    def forward(ctx, means, late: bool):
        N, Cc = means.shape
        m = means.detach().contiguous()
        dev = m.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        want_grad = means.requires_grad
        grad = torch.empty(N, Cc, dtype=torch.float32, device=dev) if want_grad else None
        tmp = torch.empty(N * N + N, dtype=torch.float32, device=dev)
        check(_lib.lib().ogs_separation_loss(ptr(m), N, Cc, int(bool(late)), ptr(loss), ptr(grad), ptr(tmp), _stream()),
              "ogs_separation_loss")
        ctx.grad = grad
        return loss

    @staticmethod
    def backward(ctx, g):
        return (None if ctx.grad is None else ctx.grad * g), None


def _separation_loss_torch(feat_mean_stack, iteration):
    N, _ = feat_mean_stack.shape
    diff_squared = (feat_mean_stack.unsqueeze(1) - feat_mean_stack.unsqueeze(0)).pow(2).sum(2)
    inverse_distance = 1.0 / (diff_squared + 1)
    eye = torch.eye(N, device=feat_mean_stack.device).bool()
    inverse_distance = inverse_distance.masked_fill(eye, 0)
    sorted_indices = inverse_distance.argsort().argsort()
    loss_weight = (sorted_indices.float() / (N - 1)) * (1.0 - 0.1) + 0.1
    if iteration > 35_000:
        loss_weight[loss_weight < 0.9] = 0.1
    return (inverse_distance * loss_weight).sum() / (N * (N - 1))


def separation_loss(feat_mean_stack, iteration):
    """Inter-mask contrastive loss, Eq. (2) (train.py:124-155).  On the GPU (fp32, 2 <= N <= 1024 masks, C <= 16): the
    whole [N, N] computation -- pairwise inverse distances, the rank of every element inside its row
    (argsort().argsort()), the rank weights, the sum AND the gradient -- in two small launches instead of ~30
    launch-bound torch kernels and two segmented sorts (0.3-0.45 ms -> 0.03 ms forward + backward).  Anything else (CPU
    tensors of the host-logic tests, other dtypes, N = 1) takes the literal torch formulation."""
    N, Cc = feat_mean_stack.shape
    if feat_mean_stack.is_cuda and feat_mean_stack.dtype is torch.float32 and 2 <= N <= 1024 and 1 <= Cc <= 16:
        return _Separation.apply(feat_mean_stack, iteration > 35_000)
    return _separation_loss_torch(feat_mean_stack, iteration)


def pair_mask_feature_mean(feat_map, masks):
    """Mean feature of N (map, mask) pairs (utils/opengs_utlis.py:181-197): feat_map [N,C,H,W], masks [N,H,W].
    One pass over data that already has the N*C*H*W shape -- nothing to fuse; torch on the GPU."""
    m = masks.unsqueeze(1).float()
    return (feat_map * m).sum(dim=[2, 3]) / (m.expand(-1, feat_map.shape[1], -1, -1).sum(dim=[2, 3]) + 1e-6)


def calculate_iou(masks1, masks2, base=None):
    """IoU matrix [m, n] of masks2 [m,H,W] against masks1 [n,H,W] (utils/opengs_utlis.py:90-123).  The
    intersection counts are one {0,1} GEMM over the pixels (fp32: sums of 0/1 products are exact below 2^24
    pixels) instead of an [m, n, H, W] boolean expansion."""
    _need_gpu(masks1, "masks1")
    a = (masks1 != 0).flatten(1)
    b = (masks2 != 0).flatten(1)
    if a.shape[1] >= (1 << 24):
        raise RuntimeError("calculate_iou: more than 2^24 pixels per mask")
    inter = b.float() @ a.float().t()                                            # [m, n]
    ca = a.sum(dim=1).float()[None, :]
    cb = b.sum(dim=1).float()[:, None]
    if base == "former":
        union = ca + 1e-6
    elif base == "later":
        union = cb + 1e-6
    else:
        union = ca + cb - inter + 1e-6
    return inter / union
