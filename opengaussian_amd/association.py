"""2D-3D association (train.py ``construct_pseudo_ins_feat``) on grouped label statistics instead of images.

Drop-in for the reference's ``construct_pseudo_ins_feat(scene, renderFunc, renderArgs, filter, cluster_indices, mode,
root_num, leaf_num, sam_level, save_memory, enable_multiview_refinement)``: same signature, same side effects --

  * every mode: ``view.pesudo_ins_feat`` [6, H, W] and ``view.pesudo_mask_bool`` [M+1, H, W] (bit for bit the reference's);
  * ``mode="leaf"`` (stage 2.2): ``view.cluster_masks`` / ``view.bClusterOccur`` (set when still None) and
    ``scene.gaussians.iClusterSubNum``;
  * ``mode="lang"`` (stage 3): ``<model_path>/cluster_lang.npz`` with leaf_feat, leaf_score, occu_count, leaf_ind; the
    ``match_info`` [k1*k2, V, 3] table (matched mask id, score, matched) is also returned (the reference returns None);
  * ``save_memory``: views are moved back with ``to_cpu()`` after use, as the reference does.

What changes is how the decisions are reached.  Each of them depends only on, per (rendered subset g, pseudo mask l), the pixels
where alpha_g > thr inside mask l, the sum of g's blended feature over them, and g's maximum alpha.  The pseudo masks of one SAM
level are disjoint, so they are one int32 label image and those numbers are one grouped statistics pass per view
(rasterizer.rasterize_group_stats): stage 2.2 runs ONE pass over the coarse clusters of a view instead of a render() with an
image per cluster plus a Python loop; stage 3 runs ONE pass over all root_num * leaf_num leaves of a view instead of root_num
render() calls with up to leaf_num images each.  The table -> decision logic (``coarse_decisions``, ``leaf_decisions``) is
plain torch and is fed by image-derived tables just as well (``tables_from_images``): the CPU tests drive it with hand-made
images, and the fall-back below uses it.

Kept from the reference: IoU against the mask's pixel count + 1e-6 in stage 2.2 (``base="former"``), the ``topk(l1, 10)``
over ALL intersecting masks, the skip of a cluster whose selection is empty, ``cluster_occur`` as a CPU bool tensor, the
``match_info`` layout.  The CPU RNG advances by one ``torch.rand(1)`` per replaced render() call (V in stage 2.2, root_num * V
in stage 3), so a training run continues on the reference's random sequence.

Not reproduced: the debug PNG dumps (``debug_pseudo_label``, ``stage3``): they need torchvision and full images.
Fall-back: if a view's ``pesudo_mask_bool`` has overlapping rows (a caller that set it itself), a label image cannot carry it;
that view's stage 2.2 / 3 work runs through ``renderFunc`` images and ``mask_ops`` instead (same decisions logic).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import mask_ops
from .rasterizer import GaussianRasterizationSettings, rasterize_group_stats, visible_radii

COARSE_ALPHA = 0.9          # stage 2.2 silhouette threshold (train.py, rendered_cluster_silhouettes > 0.9)
COARSE_SEEN = 0.8           # a coarse cluster is rendered at all when max alpha > 0.8 (gaussian_renderer cluster branch)
LEAF_ALPHA = 0.8            # stage 3 silhouette threshold
MIN_COARSE_POINTS = 100     # better_vis: >= 100 small visible Gaussians per coarse cluster
MIN_LEAF_POINTS = 10        # >= 10 visible Gaussians per leaf


# ---- pseudo labels (stage 2.1 part of every mode) ----------------------------------------------------------------------
def sam_mask_ids(sam_mask: torch.Tensor, level: int) -> torch.Tensor:
    """Per-pixel mask number of one SAM level, 0 = invalid (get_SAM_mask_and_feat: ids relative to the previous level)."""
    mid = sam_mask[level].clone()
    if level > 0:
        mid = mid - (sam_mask[level - 1].max().detach().cpu() + 1)
    if mid.min() < 0:
        mid = mid.clamp_min(-1)
    return mid + 1


def pseudo_labels(view, rendered_ins_feat: torch.Tensor, sam_level: int, filter: bool = True):
    """Sets ``view.pesudo_ins_feat`` / ``view.pesudo_mask_bool`` from the rendered feature map and the view's SAM masks, and
    returns the label image (int32 [H, W]: row number of ``pesudo_mask_bool`` for the pixels of a kept mask, -1 elsewhere)
    and the row count L = M + 1.  Per-mask means and variances come from mask_ops.mask_feature_mean on the mask rows, as in
    the reference; no int64 one-hot is built."""
    mid = sam_mask_ids(view.original_sam_mask.cuda(), sam_level)
    M = int(mid.max().item())
    H, W = mid.shape
    rows = mid.unsqueeze(0) == torch.arange(1, M + 1, device=mid.device).view(-1, 1, 1)        # [M, H, W] bool
    mean_, var, pix = mask_ops.mask_feature_mean(rendered_ins_feat, rows, return_var=True)
    C = rendered_ins_feat.shape[0]
    mean = torch.cat((torch.zeros((1, C), device=mean_.device), mean_), dim=0)              # [M+1, C]
    drop = torch.cat((torch.tensor([False], device=var.device), var > 0.006), dim=0)        # high variance: filtered
    big = torch.nonzero(pix > pix.max() * 0.8).squeeze()                                   # large masks are kept
    drop[big + 1] = False
    filtered = mean.clone()
    filtered[drop] *= 0
    view.pesudo_ins_feat = (filtered if filter else mean)[mid].permute(2, 0, 1)
    pmb = torch.zeros((M + 1, H, W), dtype=torch.bool, device=mid.device)
    pmb[1:] = rows
    pmb[drop] = False
    view.pesudo_mask_bool = pmb
    keep = ~drop
    labels = torch.where(keep[mid] & (mid > 0), mid, torch.full_like(mid, -1)).to(torch.int32)
    return labels, M + 1


def labels_of_mask_rows(mask_bool: torch.Tensor):
    """int32 label image of disjoint boolean rows [L, H, W] (-1: no row), or None when rows overlap."""
    if mask_bool.shape[0] == 0:
        return torch.full(mask_bool.shape[1:], -1, dtype=torch.int32, device=mask_bool.device)
    per_pix = mask_bool.sum(dim=0)
    if bool((per_pix > 1).any()):
        return None
    return torch.where(per_pix > 0, mask_bool.to(torch.uint8).argmax(dim=0), torch.full_like(per_pix, -1)).to(torch.int32)


# ---- tables -> decisions (pure torch, any device) --------------------------------------------------------------------------
def tables_from_stats(count: torch.Tensor, feat_sum: torch.Tensor, L: int):
    """(inter [G, L] f32, feat_inter [G, L, C], sil_count [G] f32, feat_sil [G, C]) of a statistics pass: bucket L holds the
    silhouette pixels outside every mask."""
    inter = count[:, :L].to(torch.float32)
    return inter, feat_sum[:, :L], count.sum(dim=1).to(torch.float32), feat_sum.sum(dim=1)


def tables_from_images(imgs: torch.Tensor, sil: torch.Tensor, masks: torch.Tensor):
    """The same tables from images: imgs [G, C, H, W], sil [G, H, W] bool, masks [L, H, W] bool (may overlap)."""
    G, C = imgs.shape[:2]
    s = sil.flatten(1).to(torch.float32)
    m = masks.flatten(1).to(torch.float32)
    f = imgs.flatten(2) * s[:, None, :]                                   # [G, C, HW]
    inter = s @ m.t()
    feat_inter = torch.einsum("gcp,lp->glc", f, m)
    return inter, feat_inter, s.sum(dim=1), f.sum(dim=2)


def coarse_decisions(inter, feat_inter, mask_pix, pseudo_mean):
    """Stage 2.2 for the clusters of one view that were seen, in cluster order.  inter / feat_inter as tables_from_*; mask_pix
    [L] pixels per pesudo_mask_bool row; pseudo_mean [L, C] = mask_feature_mean(view.pesudo_ins_feat, view.pesudo_mask_bool).
    Returns per cluster the selected row numbers (a LongTensor, empty: the cluster is skipped)."""
    out = []
    for g in range(inter.shape[0]):
        iou = inter[g] / (mask_pix + 1e-6)                                 # base="former"
        rows = torch.nonzero(iou > 0.2).flatten()
        cluster_mean = feat_inter[g, rows] / inter[g, rows].clamp(min=1)[:, None]
        diff = pseudo_mean[rows] - cluster_mean
        l1 = diff.abs().sum(dim=1)
        l2 = diff.pow(2).sum(dim=1).sqrt()
        sel = rows[(l1 < 0.9) & (l2 < 0.5)]
        if sel.numel() > 10:
            sel = rows[torch.topk(l1, 10, largest=False)[1]]                # over every intersecting mask (the reference's)
        out.append(sel)
    return out


def leaf_decisions(inter, feat_sil, sil_count, mask_pix, pseudo_mean):
    """Stage 3 for the leaves of one view: (max_ind, max_score, b_matched, scores) as the reference stores them in
    match_info (non-matched: index and score 0)."""
    union = (mask_pix[None, :] + sil_count[:, None]) - inter + 1e-6
    ious = inter / union
    pred = feat_sil / (sil_count[:, None] + 1e-6)
    l1 = (pred[:, None, :] - pseudo_mean[None, :, :]).abs().sum(dim=2)
    scores = ious * (1 - l1)
    max_score, max_ind = torch.max(scores, dim=-1)
    b = max_score > 0.2
    max_score = max_score * b
    max_ind = max_ind * b
    return max_ind, max_score, b, scores


# ---- the driver --------------------------------------------------------------------------------------------------------
def _settings(view, pc, pipe, bg):
    import math
    return GaussianRasterizationSettings(
        image_height=int(view.image_height), image_width=int(view.image_width),
        tanfovx=math.tan(view.FoVx * 0.5), tanfovy=math.tan(view.FoVy * 0.5), bg=bg, scale_modifier=1.0,
        viewmatrix=view.world_view_transform, projmatrix=view.full_proj_transform, sh_degree=pc.active_sh_degree,
        campos=view.camera_center, prefiltered=False, debug=bool(getattr(pipe, "debug", False)))


def _geometry(pc, pipe):
    """(means3D, opacity, scales, rotations, cov3D) as render() hands them to the rasterizer, detached"""
    with torch.no_grad():
        if getattr(pipe, "compute_cov3D_python", False):
            return pc.get_xyz.detach(), pc.get_opacity.detach(), None, None, pc.get_covariance(1.0).detach()
        return pc.get_xyz.detach(), pc.get_opacity.detach(), pc.get_scaling.detach(), pc.get_rotation.detach(), None


def _stats_pass(view, pc, pipe, bg, gid, G, labels, L, feat, thr):
    m3, op, scl, rot, cov = _geometry(pc, pipe)
    rs = _settings(view, pc, pipe, bg)
    with torch.no_grad():
        return rasterize_group_stats(m3, op, gid, G, labels, L, rs, feat, scales=scl, rotations=rot, cov3D_precomp=cov,
                                     alpha_threshold=thr)


def _viewed(view, pc, pipe, bg, feat):
    m3, op, scl, rot, cov = _geometry(pc, pipe)
    with torch.no_grad():
        return visible_radii(m3, op, _settings(view, pc, pipe, bg), feat, scales=scl, rotations=rot, cov3D_precomp=cov) > 0


def _coarse_groups(view, pc, viewed, cluster_indices, num_cluster):
    """cluster number of every Gaussian the better_vis cluster pass renders (-1: none), and the kept clusters"""
    scales = pc.get_scaling.detach()
    gid = torch.where(viewed, cluster_indices.to(torch.int64), torch.full_like(cluster_indices, -1, dtype=torch.int64))
    gid = torch.where((scales < 0.5).all(dim=1), gid, torch.full_like(gid, -1))
    occ = getattr(view, "bClusterOccur", None)
    if occ is not None:
        occ = torch.as_tensor(occ).to(device=gid.device, dtype=torch.bool)
        gid = torch.where(occ[gid.clamp_min(0)], gid, torch.full_like(gid, -1))
    counts = torch.bincount(gid[gid >= 0], minlength=num_cluster)[:num_cluster]
    return gid, torch.nonzero(counts >= MIN_COARSE_POINTS).flatten()


def _leaf_groups(view, viewed, cluster_indices, root_num, leaf_num):
    """leaf number of every Gaussian some per-root stage-3 render draws (-1: none), and the kept leaves"""
    n_leaf = root_num * leaf_num
    lid = cluster_indices.to(torch.int64)
    gid = torch.where((lid >= 0) & (lid < n_leaf) & viewed, lid, torch.full_like(lid, -1))     # k1*k2: the dummy leaf
    occ = getattr(view, "bClusterOccur", None)
    if occ is not None:
        occ = torch.as_tensor(occ).to(device=gid.device, dtype=torch.bool)
        gid = torch.where(occ[(gid.clamp_min(0) // leaf_num)], gid, torch.full_like(gid, -1))
    counts = torch.bincount(gid[gid >= 0], minlength=n_leaf)[:n_leaf]
    return gid, torch.nonzero(counts >= MIN_LEAF_POINTS).flatten()


def _compact(gid, kept, n):
    remap = torch.full((n + 1,), -1, dtype=torch.int32, device=gid.device)
    remap[kept] = torch.arange(kept.numel(), dtype=torch.int32, device=gid.device)
    return remap[torch.where(gid >= 0, gid, torch.full_like(gid, n))]


def _to_gpu(view):
    if not getattr(view, "data_on_gpu", True):
        view.to_gpu()


def _release(view, save_memory):
    if getattr(view, "data_on_gpu", False) and save_memory:
        view.to_cpu()


def construct_pseudo_ins_feat(scene, renderFunc, renderArgs, filter=True, cluster_indices=None, mode="root", root_num=64,
                              leaf_num=10, sam_level=3, save_memory=False, enable_multiview_refinement=False):
    torch.cuda.empty_cache()
    pc = scene.gaussians
    pipe, bg = renderArgs[0], renderArgs[1]
    views = sorted(scene.getTrainCameras(), key=lambda cam: cam.image_name)

    for view in views:
        _to_gpu(view)
        pkg = renderFunc(view, pc, *renderArgs, rescale=False, origin_feat=True)
        pseudo_labels(view, pkg["ins_feat"], sam_level, filter)
        _release(view, save_memory)

    torch.cuda.empty_cache()
    if mode == "leaf":
        _stage_coarse(views, pc, pipe, bg, renderFunc, renderArgs, cluster_indices, root_num, leaf_num, save_memory)
        torch.cuda.empty_cache()
    if mode == "lang":
        return _stage_lang(scene, views, pc, pipe, bg, renderFunc, renderArgs, cluster_indices, root_num, leaf_num,
                           sam_level, save_memory)
    return None


def _view_labels(view):
    """the label image of the view's pesudo_mask_bool rows (None when rows overlap: the image path), L, the rows"""
    pmb = view.pesudo_mask_bool.cuda()
    return labels_of_mask_rows(pmb), pmb.shape[0], pmb


def _stage_coarse(views, pc, pipe, bg, renderFunc, renderArgs, cluster_indices, root_num, leaf_num, save_memory):
    num_cluster = int(cluster_indices.max()) + 1
    sub_num = torch.ones(num_cluster).to(torch.int32)
    for view in views:
        _to_gpu(view)
        labels, L, pmb = _view_labels(view)
        mask_pix = pmb.flatten(1).sum(dim=1).to(torch.float32)
        pseudo_ins = view.pesudo_ins_feat.cuda()
        pseudo_mean = mask_ops.mask_feature_mean(pseudo_ins, pmb)
        if labels is None:
            # overlapping rows: the image path (the reference's render() of the clusters)
            pkg = renderFunc(view, pc, *renderArgs, cluster_idx=cluster_indices, rescale=False, render_feat_map=False,
                             render_cluster=True, origin_feat=True, better_vis=True, root_num=root_num, leaf_num=leaf_num)
            occur = pkg["cluster_occur"]
            seen = torch.nonzero(occur).flatten().tolist()
            if seen:
                sil = pkg["cluster_silhouettes"] > COARSE_ALPHA
                inter, feat_inter, _, _ = tables_from_images(torch.stack(pkg["cluster_imgs"]), sil, pmb)
        else:
            torch.rand(1)                   # the RNG draw of the replaced render() call
            feat = (pc.get_ins_feat(origin=True).detach() + 1) / 2
            viewed = _viewed(view, pc, pipe, bg, feat)
            occur = torch.zeros(num_cluster).to(torch.bool)
            seen = []
            if bool(viewed.any()):
                gid, kept = _coarse_groups(view, pc, viewed, cluster_indices.to(viewed.device), num_cluster)
                if kept.numel():
                    max_alpha, count, feat_sum, _ = _stats_pass(view, pc, pipe, bg, _compact(gid, kept, num_cluster),
                                                                kept.numel(), labels, L, feat, COARSE_ALPHA)
                    ok = max_alpha > COARSE_SEEN
                    seen = kept[ok].tolist()
                    occur[seen] = True
                    inter, feat_inter, _, _ = tables_from_stats(count[ok], feat_sum[ok], L)
        masks = []
        if seen:
            # a few KB of tables: the per-cluster selection loop runs on the host, one copy instead of a sync per cluster
            sels = coarse_decisions(inter.cpu(), feat_inter.cpu(), mask_pix.cpu(), pseudo_mean.cpu())
            for c, sel in zip(seen, sels):
                if sel.numel() == 0:
                    occur[c] = False
                    continue
                sel = sel.to(pmb.device)
                masks.append(pmb[sel].any(dim=0) if labels is None else torch.isin(labels, sel.to(labels.dtype)))
                sub_num[c] = max(sub_num[c], sel.numel())
        if getattr(view, "cluster_masks", None) is None:
            view.cluster_masks = masks
            view.bClusterOccur = occur
        _release(view, save_memory)
    pc.iClusterSubNum = (sub_num + 1).clamp(max=leaf_num)


def _stage_lang(scene, views, pc, pipe, bg, renderFunc, renderArgs, cluster_indices, root_num, leaf_num, sam_level,
                save_memory):
    n_leaf = root_num * leaf_num
    match_info = torch.zeros(n_leaf, len(views), 3).cuda()
    for v_id, view in enumerate(views):
        _to_gpu(view)
        labels, L, pmb = _view_labels(view)
        mask_pix = pmb.flatten(1).sum(dim=1).to(torch.float32)
        pseudo_mean = mask_ops.mask_feature_mean(view.pesudo_ins_feat.cuda(), pmb)       # once per view, not per root
        if labels is None:
            for root_id in range(root_num):     # the image path: the reference's per-root render() calls
                pkg = renderFunc(view, pc, *renderArgs, leaf_cluster_idx=cluster_indices, rescale=False, render_feat_map=False,
                                 render_cluster=True, origin_feat=True, better_vis=False, selected_root_id=root_id,
                                 root_num=root_num, leaf_num=leaf_num)
                ids = pkg["occured_leaf_id"]
                if not ids:
                    continue
                sil = pkg["leaf_cluster_silhouettes"] > LEAF_ALPHA
                inter, _, sil_count, feat_sil = tables_from_images(torch.stack(pkg["leaf_clusters_imgs"]), sil, pmb)
                ind, score, b, _ = leaf_decisions(inter, feat_sil, sil_count, mask_pix, pseudo_mean)
                match_info[torch.tensor(ids).cuda(), v_id] = torch.stack((ind, score, b), dim=1).to(match_info.dtype)
        else:
            for _ in range(root_num):
                torch.rand(1)                   # the RNG draws of the root_num replaced render() calls
            feat = (pc.get_ins_feat(origin=True).detach() + 1) / 2
            viewed = _viewed(view, pc, pipe, bg, feat)
            gid, kept = _leaf_groups(view, viewed, cluster_indices.to(viewed.device), root_num, leaf_num)
            if kept.numel():
                _, count, feat_sum, _ = _stats_pass(view, pc, pipe, bg, _compact(gid, kept, n_leaf), kept.numel(), labels, L,
                                                    feat, LEAF_ALPHA)
                inter, _, sil_count, feat_sil = tables_from_stats(count, feat_sum, L)
                ind, score, b, _ = leaf_decisions(inter, feat_sil, sil_count, mask_pix, pseudo_mean)
                match_info[kept.to(match_info.device), v_id] = torch.stack((ind, score, b), dim=1).to(match_info.dtype)
        _release(view, save_memory)
    torch.cuda.empty_cache()
    write_cluster_lang(scene, views, match_info, cluster_indices, root_num, leaf_num, sam_level, save_memory)
    return match_info


def write_cluster_lang(scene, views, match_info, cluster_indices, root_num, leaf_num, sam_level, save_memory):
    """Per-leaf language feature from the matches of every view -> cluster_lang.npz (the tail of stage 3)."""
    n_leaf = root_num * leaf_num
    matched = match_info[:, :, 0].to(torch.int64)
    totals = match_info.sum(dim=1)
    leaf_score = totals[:, 1] / (totals[:, 2] + 1e-6)
    occu = totals[:, 2]
    feat_sum = None
    for v_id, view in enumerate(views):
        _to_gpu(view)
        sam = view.original_sam_mask
        hi = sam[sam_level].max().to(torch.int64) + 1
        lo = sam[sam_level - 1].max().to(torch.int64) + 1 if sam_level > 0 else 0
        lang = view.original_mask_feat[lo:hi, :]
        lang = torch.cat((torch.zeros_like(lang[0]).unsqueeze(0), lang)).cuda()     # row 0: "no mask"
        if feat_sum is None:
            feat_sum = torch.zeros(n_leaf, lang.shape[1]).cuda()
        feat_sum += lang[matched[:, v_id]]
        _release(view, save_memory)
    if feat_sum is None:
        feat_sum = torch.zeros(n_leaf, 512).cuda()
    leaf_feat = feat_sum / (occu + 1e-4).unsqueeze(1)
    np.savez(os.path.join(scene.model_path, "cluster_lang.npz"), leaf_feat=leaf_feat.cpu().numpy(),
             leaf_score=leaf_score.cpu().numpy(), occu_count=occu.cpu().numpy(), leaf_ind=cluster_indices.cpu().numpy())
