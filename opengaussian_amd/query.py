"""Open-vocabulary queries on the GPU (include/ogs_query.h): what the reference does after ``cluster_lang.npz`` is written.

``select_leaves_by_text``   every query text to its leaves in one launch (render_lerf_by_text.py:62,101-115)
``classify_points``         leaf -> class -> point prediction (scripts/eval_scannet.py:143-144,158-163)
``segmentation_metrics``    ``calculate_metrics`` (:55-93) from one confusion table instead of 4 x classes full-length
                            reductions on the CPU; ``confusion_table`` / ``metrics_from_confusion`` are its two halves
``multi_split``             rows of OVERLAPPING leaf selections, group by group, each group ascending
``render_queries``          the object image and silhouette of every query of a view from one grouped rasterizer pass and
                            one kNN launch, instead of one ``render(selected_leaf_id=...)`` call per query
``render_label_map``        pixel -> label: per pixel the leaf / instance / class with the largest blend weight, one launch over
                            the view's kept pass (``rasterizer.label_map``); ``labels_at_pixels`` reads clicks off it
``lift_labels``             pixel labels -> Gaussians: the blend weight every Gaussian (or leaf) puts on every label of the views'
                            label images, one launch per view (``rasterizer.label_votes``), an int64 fixed-point table;
                            ``votes_as_float`` / ``labels_from_votes`` read it, ``select_leaves_by_masks`` turns mask prompts into
                            the leaf selections ``render_queries`` takes (``leaves_from_votes`` is its rule)
``lift_features``           dense per-pixel vectors -> Gaussians: the blend-weighted sum of the views' feature images per Gaussian (or
                            leaf) with the weight beside it, one call per view (``rasterizer.feature_votes``) into one int64 table;
                            ``features_from_votes`` divides; ``lift_mask_features`` is the route for features kept per 2D mask
``render_feature_map``      Gaussians -> dense per-pixel vectors, the way back: a feature table per Gaussian (or leaf) rendered into a view
                            in one launch whatever D is (``rasterizer.feature_map``), differentiable in the features with
                            ``rasterizer.feature_votes`` as its backward; ``relevancy_maps`` reads cosine / LERF relevancy off it
``diffuse_features``        the 3D side of lifting: fill the Gaussians no view saw and smooth the rest over the kNN graph of the Gaussians
                            (``knn.neighbors`` + ``neighbor_weights``), one gather-sum launch per step (``knn.aggregate``)
``diffuse`` /               the same graph inside a training loss: the diffusion with a backward (``knn.gather_sum`` per step) and
``neighbor_smoothness``     the loss sum w |F_i - F_j|^2 fused forward and backward; gradients through the reverse-edge lists
                            (``knn.reverse_edges``), no float atomics
``transfer_labels`` /       per-point results across a CHANGE of the point set (densified, pruned, another checkpoint, a scan): labels by
``transfer_features``       nearest-neighbour vote, feature rows by weighted mean, over exact kNN between the two sets (``knn.Index``)
``segment_instances`` /     which points hang together: the connected pieces of every class as instances, and the keep-mask of every
``component_filter``        group's connected bulk (``knn.components``: a lock-free union-find over the kNN table, one call for all)
``build_codebook``          lifted features -> leaves: wide k-means (``kmeans.wide_lloyd``, D up to 1024) into the ``leaf_ind`` /
                            ``leaf_lang_feat`` / ``occu_count`` the text queries above take -- no trained instance features needed
``click_features`` /        the reference's own click route (scripts/render_by_click.py:35-66,138-166), batched over clicks, in
``select_leaves_by_click``  plain torch

CPU tensors raise: there is no CPU path (the plain-torch click helpers and vote-table readers run wherever their inputs live).
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from . import _lib
from . import knn as _knn
from . import rasterizer as _rasterizer
from . import renderer as _renderer
from ._lib import check, ptr

SPLIT_GROUPS = 64          # groups of one split: a bit each in a leaf's 64-bit word

QueryRender = namedtuple("QueryRender", "images silhouettes kept counts")
LabelMap = namedtuple("LabelMap", "label weight second alpha")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); the query kernels have no CPU path")


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def _i64(t):
    return t.detach().to(torch.int64).contiguous()


def _bytes(t):
    return None if t is None else t.detach().to(torch.bool).contiguous().view(torch.uint8)


# ---- text -> leaves -------------------------------------------------------------------------------------------------------
def _similarity(text_feats, leaf_lang_feat, occu_count, min_occu, centers, leaf_num, max_dist, top):
    _need_gpu(text_feats, "text_feats")
    _need_gpu(leaf_lang_feat, "leaf_lang_feat")
    if text_feats.dim() != 2 or leaf_lang_feat.dim() != 2 or text_feats.shape[1] != leaf_lang_feat.shape[1]:
        raise ValueError(f"text_feats must be [Q, D] and leaf_lang_feat [K, D], got {tuple(text_feats.shape)} and "
                         f"{tuple(leaf_lang_feat.shape)}")
    (Q, D), K, dev = text_feats.shape, leaf_lang_feat.shape[0], text_feats.device
    if K < 1 or D < 1:
        raise ValueError(f"need at least one leaf and one feature, got K={K} D={D}")
    lib = _lib.lib()
    if K > lib.ogs_query_max_leaves():
        raise ValueError(f"K={K} leaves: a query's similarities are ranked in LDS, at most {lib.ogs_query_max_leaves()}")
    if top > lib.ogs_query_max_top():
        raise ValueError(f"top={top}: at most {lib.ogs_query_max_top()}")
    valid = None
    if occu_count is not None:
        if occu_count.shape != (K,):
            raise ValueError(f"occu_count must be [{K}], got {tuple(occu_count.shape)}")
        valid = _bytes(~(occu_count.to(dev) < min_occu))           # `feat[occu_count < min_occu] *= 0`
    cd = 0
    if top > 0:
        if centers.dim() != 2 or centers.shape[0] < K:
            raise ValueError(f"leaf_centers must be [>= {K}, C], got {tuple(centers.shape)}")
        _need_gpu(centers, "leaf_centers")
        centers, cd = _f32(centers), centers.shape[1]
    sim = torch.empty(Q, K, dtype=torch.float32, device=dev)
    selected = torch.empty(Q, top, dtype=torch.int32, device=dev) if top > 0 else None
    count = torch.empty(Q, dtype=torch.int32, device=dev) if top > 0 else None
    text, leaf = _f32(text_feats), _f32(leaf_lang_feat)
    check(lib.ogs_query_select(Q, K, D, ptr(text), ptr(leaf), ptr(valid), ptr(centers if top > 0 else None), cd,
                               float(leaf_num), float(max_dist), top, ptr(sim), ptr(selected), ptr(count), _stream()),
          "ogs_query_select")
    return sim, selected, count


def select_leaves_by_text(text_feats, leaf_lang_feat, occu_count, leaf_centers, leaf_num, min_occu=5, top=10, max_dist=0.9):
    """(sim [Q, K] fp32, selected [Q, top] int32, count [Q] int32) for all query texts at once.

    Leaves with ``occu_count < min_occu`` are zeroed, both sides are normalised as ``F.normalize`` does, ``sim`` is the fp32
    dot product.  ``selected[q, 0]`` is the argmax (lowest index on ties); the other ``min(top, K) - 1`` highest, ranked
    descending with ties to the lowest index, are appended in rank order when ``candidate - best < leaf_num`` (signed, so
    every lower id qualifies: the reference's rule, reproduced) and the fp32 distance of the two rows of ``leaf_centers``
    (``leaf_code_book["ins_feat"]``, [K + 1, 6]) is below ``max_dist``; the rest of the row is -1.  ``leaf_num`` is the
    reference's ``K / root_num``.  No read-back; K is limited to ``ogs_query_max_leaves()`` (8192), above that ValueError."""
    if int(top) < 1:
        raise ValueError("top must be at least 1")
    return _similarity(text_feats, leaf_lang_feat, occu_count, min_occu, leaf_centers, leaf_num, max_dist, int(top))


# ---- ScanNet point classes and metrics -----------------------------------------------------------------------------------------
def classify_points(text_feats, leaf_lang_feat, occu_count, leaf_ind, min_occu=2):
    """pred [N] int64 = ``argmax_t sim[t, leaf] + 1`` of every point's leaf, ``leaf_ind`` clamped at K - 1 (:144); leaves with
    ``occu_count < min_occu`` are zeroed and therefore map to class 0 + 1.  Negative leaf ids clamp to 0."""
    _need_gpu(leaf_ind, "leaf_ind")
    if leaf_ind.dim() != 1:
        raise ValueError(f"leaf_ind must be [N], got {tuple(leaf_ind.shape)}")
    sim, _, _ = _similarity(text_feats, leaf_lang_feat, occu_count, min_occu, None, 0.0, 0.0, 0)
    T, K = sim.shape
    if T < 1:
        raise ValueError("need at least one class text")
    n, dev = leaf_ind.shape[0], sim.device
    ind = _i64(leaf_ind)
    cls = torch.empty(K, dtype=torch.int32, device=dev)
    pred = torch.empty(n, dtype=torch.int64, device=dev)
    check(_lib.lib().ogs_query_classify(n, ptr(ind), K, T, ptr(sim), ptr(cls), ptr(pred), _stream()), "ogs_query_classify")
    return pred


def confusion_table(gt, pred, total_classes, ignore=None):
    """conf [C, C] int64 on the device: conf[g, r] = points with label g predicted r, after ``gt[ignore] = 0`` (:131-132) and
    ``pred[gt == 0] = 0`` (:58).  Values outside [0, total_classes) AFTER those two rules raise ValueError (one min / max
    read-back): a label under ``ignore`` and a prediction at an unlabelled point may hold anything."""
    _need_gpu(gt, "gt")
    _need_gpu(pred, "pred")
    C = int(total_classes)
    if gt.dim() != 1 or pred.shape != gt.shape or (ignore is not None and ignore.shape != gt.shape):
        raise ValueError(f"gt, pred and ignore must be [N] alike, got {tuple(gt.shape)}, {tuple(pred.shape)}"
                         + ("" if ignore is None else f", {tuple(ignore.shape)}"))
    lib = _lib.lib()
    if C < 1 or C > lib.ogs_query_max_classes():
        raise ValueError(f"total_classes={C}: the table of a workgroup lives in LDS, 1 to {lib.ogs_query_max_classes()} classes")
    n, dev = gt.shape[0], gt.device
    g, r = _i64(gt), _i64(pred)
    if n > 0:
        # checked as they are counted: an ignored label is 0, a prediction at an unlabelled point is 0 (a sentinel such as -1
        # there is overwritten by the reference too)
        g_seen = g if ignore is None else g.masked_fill(ignore.to(dev).to(torch.bool), 0)
        r_seen = r.masked_fill(g_seen == 0, 0)
        lo_g, hi_g, lo_r, hi_r = torch.stack((g_seen.min(), g_seen.max(), r_seen.min(), r_seen.max())).tolist()
        if lo_g < 0 or hi_g >= C or lo_r < 0 or hi_r >= C:
            raise ValueError(f"gt in [{lo_g}, {hi_g}] / pred in [{lo_r}, {hi_r}] outside [0, {C})")
    conf = torch.empty(C, C, dtype=torch.int64, device=dev)
    ign = _bytes(None if ignore is None else ignore.to(dev))
    check(lib.ogs_query_confusion(n, ptr(g), ptr(r), ptr(ign), C, ptr(conf), _stream()), "ogs_query_confusion")
    return conf


def metrics_from_confusion(conf):
    """``(ious, mean_iou, accuracy, mean_class_accuracy)`` of ``calculate_metrics`` from its confusion table, with the
    reference's arithmetic: per-class counts held in fp32 tensors, IoU and class accuracy fp32 quotients, the means over the
    classes >= 1 that occur in ``gt`` (nan when there are none), ``accuracy`` a Python quotient of integers."""
    conf = conf.detach().cpu().to(torch.int64)
    C = conf.shape[0]
    diag, row, col = conf.diagonal(), conf.sum(1), conf.sum(0)
    intersection, union, total = torch.zeros(C), torch.zeros(C), torch.zeros(C)
    intersection[1:] = diag[1:].to(torch.float32)
    union[1:] = (row + col - diag)[1:].to(torch.float32)
    total[1:] = row[1:].to(torch.float32)
    ious = torch.zeros(C)
    valid_union = union != 0
    ious[valid_union] = intersection[valid_union] / union[valid_union]
    present = torch.nonzero(row[1:] > 0).flatten() + 1
    mean_iou = ious[present].mean().item()
    correct, valid_points = int(diag[1:].sum()), int(row[1:].sum())
    accuracy = correct / valid_points if valid_points > 0 else float("nan")
    class_accuracy = intersection / total
    return ious, mean_iou, accuracy, class_accuracy[present].mean().item()


def segmentation_metrics(gt, pred, total_classes, ignore=None):
    """``calculate_metrics(gt, pred, total_classes)`` of scripts/eval_scannet.py, ``ignore`` being its ``ignored_pts``: one
    pass over the points on the GPU, one read-back of the [C, C] table, the same four results (``ious`` a CPU fp32 tensor)."""
    return metrics_from_confusion(confusion_table(gt, pred, total_classes, ignore))


# ---- the split ------------------------------------------------------------------------------------------------------------
def _pad_selections(selections, dev):
    """[Q, L] int64 ids padded with -1 from either form: a list of id tensors, or the (selected, count) pair"""
    if isinstance(selections, (tuple, list)) and len(selections) == 2 and torch.is_tensor(selections[0]) \
            and selections[0].dim() == 2:
        selected, count = selections
        if count.shape != (selected.shape[0],):
            raise ValueError(f"count must be [{selected.shape[0]}], got {tuple(count.shape)}")
        sel = selected.to(dev).to(torch.int64)
        live = torch.arange(sel.shape[1], device=dev)[None, :] < count.to(dev)[:, None]
        return torch.where(live, sel, torch.full_like(sel, -1))
    rows = [torch.as_tensor(s).to(dev).to(torch.int64).flatten() for s in selections]
    if any(torch.as_tensor(s).dim() > 1 for s in selections):
        raise ValueError("every selection must be a 1-D tensor of leaf ids")
    if not rows:
        return torch.empty(0, 0, dtype=torch.int64, device=dev)
    return torch.nn.utils.rnn.pad_sequence(rows, batch_first=True, padding_value=-1)


def leaf_group_table(selections, num_leaves, device):
    """[K, ceil(Q / 64)] int64 words, bit q % 64 of word q // 64 of row k set when query q lists leaf k; ids outside
    [0, K) select nothing.  Built on the device, no read-back."""
    sel = _pad_selections(selections, device)
    Q, K = sel.shape[0], int(num_leaves)
    W = max(1, (Q + SPLIT_GROUPS - 1) // SPLIT_GROUPS)
    member = torch.zeros(K + 1, W * SPLIT_GROUPS, dtype=torch.bool, device=device)       # row K: the ids that select nothing
    if sel.numel():
        ids = torch.where((sel >= 0) & (sel < K), sel, torch.full_like(sel, K))
        member[ids, torch.arange(Q, device=device)[:, None].expand_as(ids)] = True
    bit = torch.ones(SPLIT_GROUPS, dtype=torch.int64, device=device) << torch.arange(SPLIT_GROUPS, device=device)
    return (member[:K].view(K, W, SPLIT_GROUPS).to(torch.int64) * bit).sum(-1).contiguous(), Q


class _Split:
    """One split of up to 64 groups: count + scan at construction; ``scatter(group_keep)`` gives (begin, rows)."""

    def __init__(self, leaf_ind, words, Q, row_ok):
        self.lib, self.n, self.K, self.Q, self.dev = _lib.lib(), leaf_ind.shape[0], words.shape[0], int(Q), leaf_ind.device
        self.leaf_ind, self.words, self.row_ok = leaf_ind, words, row_ok
        self.tmp = torch.empty(self.lib.ogs_query_split_tmp_bytes(self.n, self.Q), dtype=torch.uint8, device=self.dev)
        check(self.lib.ogs_query_split_count(self.n, ptr(leaf_ind), self.K, ptr(words), ptr(row_ok), self.Q, ptr(self.tmp),
                                             _stream()), "ogs_query_split_count")
        self.begin = torch.empty(self.Q + 1, dtype=torch.int32, device=self.dev)
        self.counts = torch.empty(self.Q, dtype=torch.int32, device=self.dev)
        self._scan(None)

    def _scan(self, keep):
        check(self.lib.ogs_query_split_scan(self.n, self.Q, ptr(keep), ptr(self.tmp), ptr(self.begin), ptr(self.counts),
                                            _stream()), "ogs_query_split_scan")

    def scatter(self, group_keep, total):
        """rows [total] int64 and begin [Q + 1] int32 for the kept groups; `total` = the sum of their counts, which the
        caller has read (the scatter writes nothing at or past it)."""
        keep = _bytes(group_keep)
        if keep is not None:
            self._scan(keep)
        rows = torch.empty(int(total), dtype=torch.int64, device=self.dev)
        check(self.lib.ogs_query_split_scatter(self.n, ptr(self.leaf_ind), self.K, ptr(self.words), ptr(self.row_ok), self.Q,
                                               ptr(keep), ptr(self.tmp), ptr(rows), int(total), _stream()),
              "ogs_query_split_scatter")
        return self.begin, rows


def multi_split(leaf_ind, leaf_groups, num_groups, row_ok=None, group_keep=None):
    """(begin [Q + 1] int64, rows int64, counts [Q] int64): ``rows[begin[q]:begin[q + 1]]`` is
    ``torch.nonzero(member[:, q]).flatten()``, ascending, with ``member[p, q] = bit q of leaf_groups[leaf_ind[p]] & row_ok[p]
    & group_keep[q]``; ``counts`` are the group sizes BEFORE ``group_keep``.  ``leaf_groups`` is [K] or [K, ceil(Q / 64)]
    int64 words (``leaf_group_table``); leaf ids outside [0, K) are in no group.  More than 64 groups run as one split per
    64.  One read-back of the counts per split (the size of ``rows``)."""
    _need_gpu(leaf_ind, "leaf_ind")
    _need_gpu(leaf_groups, "leaf_groups")
    Q = int(num_groups)
    words = leaf_groups.reshape(leaf_groups.shape[0], -1)
    if leaf_ind.dim() != 1 or words.dtype != torch.int64 or words.shape[1] * SPLIT_GROUPS < Q:
        raise ValueError(f"leaf_ind must be [N] and leaf_groups [K, >= {(Q + 63) // 64}] int64, got {tuple(leaf_ind.shape)} and "
                         f"{tuple(leaf_groups.shape)} {leaf_groups.dtype}")
    if row_ok is not None and row_ok.shape != leaf_ind.shape:
        raise ValueError(f"row_ok must be [{leaf_ind.shape[0]}], got {tuple(row_ok.shape)}")
    if group_keep is not None and group_keep.shape != (Q,):
        raise ValueError(f"group_keep must be [{Q}], got {tuple(group_keep.shape)}")
    dev = leaf_ind.device
    ind, ok = _i64(leaf_ind), _bytes(row_ok)
    begins, rows, counts, base = [torch.zeros(1, dtype=torch.int64, device=dev)], [], [], 0
    for c0 in range(0, Q, SPLIT_GROUPS):
        qc = min(SPLIT_GROUPS, Q - c0)
        sp = _Split(ind, words[:, c0 // SPLIT_GROUPS].contiguous(), qc, ok)
        keep = None if group_keep is None else group_keep[c0:c0 + qc].to(dev).to(torch.bool)
        cnt = sp.counts.to(torch.int64)
        total = int((cnt if keep is None else cnt * keep).sum())                       # the read-back
        b, r = sp.scatter(keep, total)
        begins.append(b[1:].to(torch.int64) + base)
        rows.append(r)
        counts.append(cnt)
        base += total
    check(_lib.lib().ogs_check_async_status(), "ogs_check_async_status")
    if not rows:
        return begins[0], torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    return torch.cat(begins), torch.cat(rows), torch.cat(counts)


# ---- all queries of a view ------------------------------------------------------------------------------------------------------
def _visible(means3D, opacity, settings, scales, rotations, cov3D):
    """radii > 0 of the view's pass; a radius does not depend on colour, the means stand in for the [P, 3] colour input"""
    return _rasterizer.visible_radii(means3D, opacity, settings, means3D, scales=scales, rotations=rotations,
                                     cov3D_precomp=cov3D) > 0


def _render_groups(local, num, settings, means3D, opacity, scales, rotations, cov3D, shs, colors):
    """Images of the subsets {r : local[r] == g}, g < num, of the given rows: the plain pass on the indexed subset for one
    subset (what render() does for a selection), one grouped pass otherwise.  -> (colour list, alpha list)

    The one-subset / grouped branch restates renderer._render_subsets (on gathered rows and without its mask bookkeeping);
    the images are bit-equal to render()'s only while the two make the same rasterizer calls, so change them together."""
    pick = lambda t, m: None if t is None else t[m]
    means2D = torch.zeros_like(means3D)
    if num == 1:
        m = local == 0
        color, _, _, alpha = _rasterizer.GaussianRasterizer(settings)(
            means3D=means3D[m], means2D=means2D[m], shs=pick(shs, m), colors_precomp=pick(colors, m), opacities=opacity[m],
            scales=pick(scales, m), rotations=pick(rotations, m), cov3D_precomp=pick(cov3D, m))
        return [color], [alpha]
    color, _, _, alpha = _rasterizer.rasterize_groups(means3D, means2D, opacity, local, num, settings, shs=shs,
                                                      colors_precomp=colors, scales=scales, rotations=rotations,
                                                      cov3D_precomp=cov3D)
    return list(color.unbind(0)), list(alpha.unbind(0))


@torch.no_grad()
def render_queries(view, pc, pipe, bg, iteration, leaf_cluster_idx, selections, pre_mask=None, better_vis=True, seg_rgb=True,
                   post_process=True, root_num=64, leaf_num=10, num_leaves=None):
    """Object image and silhouette of every query of one view: for each q what

        render(view, pc, pipe, bg, iteration, rescale=False, leaf_cluster_idx=leaf_cluster_idx,
               selected_leaf_id=selections[q], render_feat_map=False, render_cluster=False, better_vis=..., seg_rgb=...,
               post_process=..., pre_mask=..., root_num=..., leaf_num=...)

    returns as ``leaf_clusters_imgs[0]`` (its first three channels when ``seg_rgb``) and ``leaf_cluster_silhouettes[0]``, or
    None where that call returns empty lists -- bit for bit, from one preprocess, one split, one kNN launch and one grouped
    rasterizer pass per 64 queries instead of one of each per query.  Forward only (no autograd graph).

    ``selections``: a list of 1-D leaf-id tensors, or the ``(selected, count)`` pair of ``select_leaves_by_text``.  An empty
    selection renders nothing (None).  ``num_leaves``: size of the leaf table, default ``root_num * leaf_num + 1`` (the k-means
    dummy id included); ids beyond it select nothing.

    Returns ``QueryRender(images, silhouettes, kept, counts)``: lists of Q entries; ``counts[q]`` is the number of Gaussians
    of query q left after the row filters (0 when the `< 100` rule dropped it), ``kept[q]`` whether it was rendered
    (``counts[q] >= 10``).  Host read-backs per 64 queries: the group counts after the split, the group counts after the kNN
    filter (only with ``post_process``), and the rasterizer's own list-length read per pass -- none grows with Q."""
    xyz = pc.get_xyz
    _need_gpu(xyz, "the model")
    _need_gpu(leaf_cluster_idx, "leaf_cluster_idx")
    dev, P = xyz.device, xyz.shape[0]
    if leaf_cluster_idx.shape != (P,):
        raise ValueError(f"leaf_cluster_idx must be [{P}], got {tuple(leaf_cluster_idx.shape)}")
    if pre_mask is not None and pre_mask.shape != (P,):
        raise ValueError(f"pre_mask must be [{P}], got {tuple(pre_mask.shape)}")
    settings = _rasterizer.GaussianRasterizationSettings(
        image_height=int(view.image_height), image_width=int(view.image_width), tanfovx=math.tan(view.FoVx * 0.5),
        tanfovy=math.tan(view.FoVy * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=view.world_view_transform,
        projmatrix=view.full_proj_transform, sh_degree=pc.active_sh_degree, campos=view.camera_center, prefiltered=False,
        debug=pipe.debug)
    means3D, opacity = xyz.detach(), pc.get_opacity.detach()
    scales = rotations = cov3D = None
    if pipe.compute_cov3D_python:
        cov3D = pc.get_covariance(1.0).detach()
    else:
        scales, rotations = pc.get_scaling.detach(), pc.get_rotation.detach()
    if better_vis and scales is None:
        raise ValueError("better_vis filters by the scales: not available with pipe.compute_cov3D_python")
    shs = colors = None
    if seg_rgb:
        if pipe.convert_SHs_python:
            raise ValueError("seg_rgb renders from the SH coefficients: not available with pipe.convert_SHs_python")
        shs = pc.get_features.detach()
    else:
        colors = ((pc.get_ins_feat(origin=False) + 1) / 2).detach()

    K = int(num_leaves) if num_leaves is not None else int(round(float(root_num) * float(leaf_num))) + 1
    table, Q = leaf_group_table(selections, K, dev)
    images, sils, kept_all, counts_all = [None] * Q, [None] * Q, [False] * Q, [0] * Q
    if Q == 0 or P == 0:
        return QueryRender(images, sils, kept_all, counts_all)

    row_ok = _visible(means3D, opacity, settings, scales, rotations, cov3D)
    occ = getattr(view, "bClusterOccur", None)
    if occ is not None and occ[None] == False:                                   # noqa: E712  render() :284-285, as it stands
        row_ok = torch.zeros_like(row_ok)
    if pre_mask is not None:
        row_ok = row_ok & pre_mask.to(dev)
    if better_vis:                                                               # small Gaussians only (:293-296)
        row_ok = row_ok & (scales < 0.1).all(dim=1)
    ind, ok = _i64(leaf_cluster_idx), _bytes(row_ok)
    per_pass = int(_renderer.GROUPS_PER_PASS)

    for c0 in range(0, Q, SPLIT_GROUPS):
        qc = min(SPLIT_GROUPS, Q - c0)
        sp = _Split(ind, table[:, c0 // SPLIT_GROUPS].contiguous(), qc, ok)
        cnt = sp.counts.tolist()                                                 # read-back 1: the Q counts
        keep = [(c >= 100 if better_vis else c > 0) for c in cnt]                # at least 100 per query (:295)
        sizes = [c if k else 0 for c, k in zip(cnt, keep)]
        total = sum(sizes)
        if total == 0:
            continue
        begin32, rows = sp.scatter(None if all(keep) else torch.tensor(keep, device=dev), total)
        sizes_t = torch.tensor(sizes, dtype=torch.int64, device=dev)
        gid = torch.repeat_interleave(torch.arange(qc, device=dev), sizes_t, output_size=total)
        g_means = means3D[rows]
        if post_process:                                                         # the kNN filter of every query, one launch
            kk = _knn.isqrt(sizes_t).to(torch.int32)                            # K = int(n ** 0.5) per query (:298)
            _, s1, s2 = _knn.ksum_contiguous(_f32(g_means), begin32, kk)
            ok_rows = _knn.keep_from_sums(gid, begin32, kk, s1, s2)
            gid = torch.where(ok_rows, gid, torch.full_like(gid, -1))
            left = torch.zeros(qc + 1, dtype=torch.int64, device=dev).index_add_(0, gid + 1, torch.ones_like(gid))
            sizes = left[1:].tolist()                                            # read-back 2
        check(_lib.lib().ogs_check_async_status(), "ogs_check_async_status")
        drawn = [q for q in range(qc) if sizes[q] >= 10]                         # at least 10 per query (:313)
        for q in range(qc):
            counts_all[c0 + q], kept_all[c0 + q] = int(sizes[q]), sizes[q] >= 10
        pick = lambda t: None if t is None else t[rows]
        g = dict(means3D=g_means, opacity=opacity[rows], scales=pick(scales), rotations=pick(rotations), cov3D=pick(cov3D),
                 shs=pick(shs), colors=pick(colors))
        for p0 in range(0, len(drawn), per_pass):
            chunk = drawn[p0:p0 + per_pass]
            remap = torch.full((qc + 1,), -1, dtype=torch.int32, device=dev)
            remap[torch.tensor(chunk, device=dev)] = torch.arange(len(chunk), dtype=torch.int32, device=dev)
            local = remap[torch.where(gid >= 0, gid, torch.full_like(gid, qc))]
            imgs, alphas = _render_groups(local, len(chunk), settings, **g)
            for q, img, alpha in zip(chunk, imgs, alphas):
                images[c0 + q], sils[c0 + q] = img, alpha
    return QueryRender(images, sils, kept_all, counts_all)


# ---- pixel -> label ------------------------------------------------------------------------------------------------------------
def _kept_pass_of_view(view, pc, pipe, bg, xyz, scaling_modifier):
    """The UN-RESCALED ungrouped streaming pass of a view, for the kernels that walk a finished pass again: the pass ``render()``
    kept for this camera when the model is frozen (a look at ``rasterizer.KEPT_PASSES``, not a lookup: slots and counters stay
    as they are), else one pass run here (its colour is never read, so the means stand in for it) whose state the caller drops.
    None when nothing reaches a tile of the view.  Call under ``no_grad``."""
    frozen = _renderer._frozen_geometry_key(view, pc, pipe, xyz, scaling_modifier)
    if frozen is not None:
        e = _rasterizer.KEPT_PASSES.slots.get(frozen[0])
        if e is not None and e.key[0] == frozen[1] and e.full_binning == bool(_rasterizer.FULL_BINNING):
            return e
    if xyz.shape[0] == 0:
        return None
    settings = _rasterizer.GaussianRasterizationSettings(
        image_height=int(view.image_height), image_width=int(view.image_width), tanfovx=math.tan(view.FoVx * 0.5),
        tanfovy=math.tan(view.FoVy * 0.5), bg=bg, scale_modifier=float(scaling_modifier), viewmatrix=view.world_view_transform,
        projmatrix=view.full_proj_transform, sh_degree=pc.active_sh_degree, campos=view.camera_center,
        prefiltered=False, debug=pipe.debug)
    means3D = xyz.detach()
    scales = rotations = cov3D = None
    if pipe.compute_cov3D_python:
        cov3D = pc.get_covariance(scaling_modifier).detach()
    else:
        scales, rotations = pc.get_scaling.detach(), pc.get_rotation.detach()
    sink: list = []
    _rasterizer._RasterizeGaussians.apply(means3D, torch.zeros_like(means3D), None, means3D, pc.get_opacity.detach(),
                                          scales, rotations, cov3D, settings, 0, None, None, 1, sink, True)
    return sink[0] if sink else None


def _forward_only(pc, pipe, xyz, who):
    if torch.is_grad_enabled():
        probe = [xyz, pc.get_opacity] + ([] if pipe.compute_cov3D_python else [pc.get_scaling, pc.get_rotation])
        if any(t.requires_grad for t in probe):
            raise RuntimeError(f"{who} is forward only: call it under torch.no_grad() or detach the model")


def render_label_map(view, pc, pipe, bg, iteration, point_labels, num_labels, pre_mask=None, scaling_modifier=1.0):
    """``LabelMap(label [H,W] int32, weight, second, alpha [H,W] fp32)`` of one view: per pixel the label whose Gaussians carry the
    largest summed blend weight (lowest label on an exact tie, -1 where no labelled Gaussian contributes), that weight, the
    runner-up label's weight, and the alpha of the full-scene render.  ``point_labels`` [P] integers: leaf ids
    (click -> leaf -> ``render_queries``), instance ids, or ``classify_points`` output (a 2D class map); values outside
    [0, num_labels) are unlabelled.  ``pre_mask`` [P] bool sets the labels of masked-out points to -1: they still occlude, as in the
    full-scene render.

    The map is one launch over the UN-RESCALED pass of the view: the pass ``render()`` kept for this camera when the model is
    frozen (``rasterizer.KEPT_PASSES``), else one pass run here and dropped afterwards (its colour is never read, so the means
    stand in for it, as in ``render_queries``); nothing is admitted to the cache by this call.  Forward only: runs under
    ``no_grad`` and raises when a model tensor requires grad while grad mode is on."""
    xyz = pc.get_xyz
    _need_gpu(xyz, "the model")
    if not torch.is_tensor(point_labels):
        raise ValueError("point_labels must be a tensor")
    _need_gpu(point_labels, "point_labels")
    P = xyz.shape[0]
    if point_labels.shape != (P,):
        raise ValueError(f"point_labels must be [{P}], got {tuple(point_labels.shape)}")
    if pre_mask is not None and pre_mask.shape != (P,):
        raise ValueError(f"pre_mask must be [{P}], got {tuple(pre_mask.shape)}")
    _forward_only(pc, pipe, xyz, "render_label_map")
    with torch.no_grad():
        dev = xyz.device
        H, W = int(view.image_height), int(view.image_width)
        labels = point_labels.to(dev)
        if pre_mask is not None:
            labels = torch.where(pre_mask.to(dev).to(torch.bool), labels, torch.full_like(labels, -1))
        kept = _kept_pass_of_view(view, pc, pipe, bg, xyz, scaling_modifier)
        if kept is None:
            # nothing reaches a tile of this view: an empty map
            z = lambda: torch.zeros(H, W, dtype=torch.float32, device=dev)
            return LabelMap(torch.full((H, W), -1, dtype=torch.int32, device=dev), z(), z(), z())
        return LabelMap(*_rasterizer.label_map(kept, labels, num_labels))


def _window(pixels_xy, radius, W, H):
    """(x [K, n], y [K, n], inside [K, n]) of the (2r+1)^2 window around every click, in the reference's order (x outer, y inner,
    render_by_click.py:46-48); positions outside the image are flagged, their coordinates clamped into it"""
    xy = torch.as_tensor(pixels_xy)
    if xy.dim() != 2 or xy.shape[1] != 2 or xy.is_floating_point():
        raise ValueError(f"pixels_xy must be [K, 2] integers (x, y), got {tuple(xy.shape)} {xy.dtype}")
    r = int(radius)
    if r < 0:
        raise ValueError("radius must be >= 0")
    xy = xy.to(torch.int64)
    d = torch.arange(-r, r + 1, device=xy.device)
    x = (xy[:, 0, None, None] + d[None, :, None]).expand(-1, -1, 2 * r + 1).reshape(xy.shape[0], -1)
    y = (xy[:, 1, None, None] + d[None, None, :]).expand(-1, 2 * r + 1, -1).reshape(xy.shape[0], -1)
    inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    return x.clamp(0, W - 1), y.clamp(0, H - 1), inside


def labels_at_pixels(label_map, pixels_xy, radius=0):
    """[K] int64: per click (x, y) the label with the largest summed ``weight`` over the (2r+1)^2 window clamped to the image,
    the lowest label on a tie, -1 when the window holds no label.  ``label_map``: a ``LabelMap`` (or any (label, weight, ...)
    pair of [H, W] tensors).  Plain torch where the map lives, no read-back and no atomics (the same bits every run; K * n * n
    compares for windows of n = (2r+1)^2 pixels); the result, one id per click, is what
    ``render_queries(..., selections=[ids[k:k + 1] ...])`` takes."""
    label, weight = label_map[0], label_map[1]
    if label.dim() != 2 or weight.shape != label.shape:
        raise ValueError(f"label and weight must be [H, W] alike, got {tuple(label.shape)} and {tuple(weight.shape)}")
    H, W = label.shape
    xy = torch.as_tensor(pixels_xy).to(label.device)
    x, y, inside = _window(xy, radius, W, H)
    lab = label[y, x].to(torch.int64)                                   # [K, n]
    valid = inside & (lab >= 0)
    w = torch.where(valid, weight[y, x].to(torch.float32), torch.zeros((), dtype=torch.float32, device=label.device))
    # total[k, j] = summed weight of the label of window pixel j: every pixel of one label holds the same sum
    same = (lab[:, :, None] == lab[:, None, :]) & valid[:, None, :]
    total = (same.to(torch.float32) * w[:, None, :]).sum(-1)
    total = torch.where(valid, total, torch.full_like(total, -1.0))
    top = total.max(dim=1, keepdim=True).values
    big = torch.iinfo(torch.int64).max
    cand = torch.where(valid & (total == top), lab, torch.full_like(lab, big))
    best = cand.min(dim=1).values
    return torch.where(best == big, torch.full_like(best, -1), best)


def click_features(ins_feat_map, pixels_xy, radius=5, quantize=True):
    """[K, C] fp32 click values of the reference (render_by_click.py:35-53,61): the mean of the rendered feature map
    ``ins_feat_map`` [C, H, W] (values in [0, 1]; C = 6: the two three-channel images of a checkpoint) over the (2r+1)^2 window
    clamped to the image, then ``* 2 - 1``.  ``quantize``: the map first takes the 8-bit rounding ``save_image`` applies
    (``mul(255).add(0.5).clamp(0, 255)`` to uint8) and the mean is divided by 255, as the reference reads it back from PNG
    files.  Plain torch where the map lives."""
    if ins_feat_map.dim() != 3:
        raise ValueError(f"ins_feat_map must be [C, H, W], got {tuple(ins_feat_map.shape)}")
    _, H, W = ins_feat_map.shape
    xy = torch.as_tensor(pixels_xy).to(ins_feat_map.device)
    x, y, inside = _window(xy, radius, W, H)
    v = ins_feat_map.detach().to(torch.float32)
    if quantize:
        v = v.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)
    v = v[:, y, x].to(torch.float64)                                    # [C, K, n]
    mean = (v * inside[None].to(torch.float64)).sum(-1) / inside.sum(-1)[None].to(torch.float64)
    mean = mean.t().to(torch.float32)
    return (mean / 255 if quantize else mean) * 2 - 1


def select_leaves_by_click(root_feats, leaf_feats, root_centers, leaf_centers):
    """[K] int64 leaf ids: option (2) of the reference's click selection (render_by_click.py:143-161) for K clicks at once.
    ``root_feats`` / ``leaf_feats`` [K, D]: the click values read off the level-1 / level-2 feature maps (``click_features``);
    ``root_centers`` [R, D + 3]: the root code book's ``ins_feat`` (its last three columns, the positions, are dropped);
    ``leaf_centers`` [N + 1, D]: the leaf code book's ``ins_feat`` (its last row, the dummy, is dropped).  An unassigned leaf
    (all-zero row sum) gets distance 999.  Per click: the nearest root, then the nearest leaf among that root's
    ``[int(root * N / R), int((root + 1) * N / R))``.  Plain torch, no read-back."""
    rc = root_centers[:, :-3].to(torch.float32)
    lc = leaf_centers[:-1].to(torch.float32)
    rf, lf = root_feats.to(torch.float32), leaf_feats.to(torch.float32)
    if rf.dim() != 2 or lf.dim() != 2 or rf.shape[0] != lf.shape[0] or rf.shape[1] != rc.shape[1] or lf.shape[1] != lc.shape[1]:
        raise ValueError(f"click values [K, {rc.shape[1]}] / [K, {lc.shape[1]}] expected, got {tuple(rf.shape)} and {tuple(lf.shape)}")
    R, N = rc.shape[0], lc.shape[0]
    if R < 1 or N < 1:
        raise ValueError("need at least one root and one leaf")
    d_root = torch.norm(rf[:, None, :] - rc[None, :, :], dim=2)
    d_leaf = torch.norm(lf[:, None, :] - lc[None, :, :], dim=2)
    d_leaf = torch.where((lc.sum(-1) == 0)[None, :], torch.full_like(d_leaf, 999.0), d_leaf)
    root = torch.argmin(d_root, dim=1)
    leaf_num = N / R                                                    # a Python float, as in the reference
    start = torch.floor(root.to(torch.float64) * leaf_num).to(torch.int64)
    end = torch.floor((root + 1).to(torch.float64) * leaf_num).to(torch.int64)
    k = torch.arange(N, device=d_leaf.device)[None, :]
    inside = (k >= start[:, None]) & (k < end[:, None])
    return torch.argmin(torch.where(inside, d_leaf, torch.full_like(d_leaf, float("inf"))), dim=1)


# ---- pixel labels -> Gaussians -------------------------------------------------------------------------------------------------
VOTE_QUANTUM = 2.0 ** -32          # one unit of a vote table (include/ogs_query.h: ogs_raster_label_votes)


def lift_labels(views, pc, pipe, bg, iteration, label_images, num_labels, rows=None, num_rows=None, scaling_modifier=1.0):
    """int64 [R, num_labels + 1] vote table over all ``views`` (fixed point, ``votes_as_float``): cell [r, l] = the blend weight
    alpha * T that the Gaussians of row r put on the pixels whose label image says l, summed over the views and seen through the
    occlusion of the full scene; column ``num_labels`` collects the pixels without a label (a value outside [0, num_labels)).
    ``label_images``: per view an [H, W] integer tensor on the GPU (SAM instance ids, class ids, prompt masks); ``rows`` [P]
    integers map the Gaussians to rows (leaf ids; outside [0, num_rows): not counted), None: one row per Gaussian.

    One launch per view (``rasterizer.label_votes``) over the view's UN-RESCALED pass: the one ``render()`` kept for the camera
    when the model is frozen, else a pass run here and dropped, the rule of ``render_label_map``.  A view no Gaussian reaches adds
    nothing.  Forward only: runs under ``no_grad`` and raises when a model tensor requires grad while grad mode is on."""
    xyz = pc.get_xyz
    _need_gpu(xyz, "the model")
    views, label_images = list(views), list(label_images)
    if len(views) != len(label_images):
        raise ValueError(f"{len(views)} views but {len(label_images)} label images")
    P = xyz.shape[0]
    if rows is not None:
        if not torch.is_tensor(rows) or rows.shape != (P,):
            raise ValueError(f"rows must be a [{P}] tensor")
        if num_rows is None:
            raise ValueError("num_rows must be given with rows")
        _need_gpu(rows, "rows")
    R = P if rows is None else int(num_rows)
    L = int(num_labels)
    if R < 1 or L < 0:
        raise ValueError(f"need num_rows >= 1 and num_labels >= 0, got {R} and {L}")
    for view, img in zip(views, label_images):
        if not torch.is_tensor(img) or tuple(img.shape) != (int(view.image_height), int(view.image_width)):
            raise ValueError(f"a label image must be a [{int(view.image_height)}, {int(view.image_width)}] tensor")
        _need_gpu(img, "label_images")
    _forward_only(pc, pipe, xyz, "lift_labels")
    with torch.no_grad():
        dev = xyz.device
        table = torch.zeros(R, L + 1, dtype=torch.int64, device=dev)
        row32 = None if rows is None else _rasterizer._int32_or_outside(rows, R, dev)
        for view, img in zip(views, label_images):
            kept = _kept_pass_of_view(view, pc, pipe, bg, xyz, scaling_modifier)
            if kept is not None:
                _rasterizer.label_votes(kept, img, L, rows=row32, num_rows=R, out=table)
        return table


def votes_as_float(table):
    """a vote table in units of blend weight: fp64, ``table * 2^-32`` (exact below 2^21 of summed weight per cell)"""
    if table.dtype is not torch.int64:
        raise ValueError(f"a vote table is int64, got {table.dtype}")
    return table.to(torch.float64) * VOTE_QUANTUM


def _rows_of_call(xyz, rows, num_rows):
    """(P, R) of a lift call after the checks ``lift_labels`` makes on ``rows`` / ``num_rows``"""
    P = xyz.shape[0]
    if rows is not None:
        if not torch.is_tensor(rows) or rows.shape != (P,):
            raise ValueError(f"rows must be a [{P}] tensor")
        if num_rows is None:
            raise ValueError("num_rows must be given with rows")
        _need_gpu(rows, "rows")
    R = P if rows is None else int(num_rows)
    if R < 1:
        raise ValueError(f"need num_rows >= 1, got {R}")
    return P, R


def lift_features(views, pc, pipe, bg, iteration, feature_images, valid_images=None, rows=None, num_rows=None,
                  scaling_modifier=1.0):
    """int64 [R, D + 1] table over all ``views`` (fixed point, ``features_from_votes``): cell [r, c < D] = the sum over the views'
    valid pixels of alpha * T * F[c] of the Gaussians of row r, seen through the occlusion of the full scene; column D the summed
    alpha * T itself.  ``feature_images``: per view a floating [D, H, W] tensor on the GPU (CLIP / DINO / LSeg maps,
    ``pesudo_ins_feat``, an error image), the same D for all; ``valid_images``: None, or per view None or a bool / integer [H, W]
    tensor whose zero pixels contribute nothing; ``rows`` [P] integers map the Gaussians to rows (leaf ids; outside
    [0, num_rows): not counted), None: one row per Gaussian.

    One call per view (``rasterizer.feature_votes``, whose range contract holds per view) into one table, over the view's
    UN-RESCALED pass: the one ``render()`` kept for the camera when the model is frozen, else a pass run here and dropped, the
    rule of ``lift_labels``.  A view no Gaussian reaches adds nothing.  Forward only: runs under ``no_grad`` and raises when a
    model tensor requires grad while grad mode is on."""
    xyz = pc.get_xyz
    _need_gpu(xyz, "the model")
    views, feature_images = list(views), list(feature_images)
    if len(views) != len(feature_images):
        raise ValueError(f"{len(views)} views but {len(feature_images)} feature images")
    valid_images = [None] * len(views) if valid_images is None else list(valid_images)
    if len(views) != len(valid_images):
        raise ValueError(f"{len(views)} views but {len(valid_images)} valid images")
    if not views:
        raise ValueError("need at least one view: the table's width is that of its feature image")
    P, R = _rows_of_call(xyz, rows, num_rows)
    D = None
    for view, img, ok in zip(views, feature_images, valid_images):
        hw = (int(view.image_height), int(view.image_width))
        if not torch.is_tensor(img) or not img.is_floating_point() or img.dim() != 3 or tuple(img.shape[1:]) != hw or img.shape[0] < 1:
            raise ValueError(f"a feature image must be a floating [D, {hw[0]}, {hw[1]}] tensor")
        D = int(img.shape[0]) if D is None else D
        if int(img.shape[0]) != D:
            raise ValueError(f"the feature images have {D} and {int(img.shape[0])} channels")
        _need_gpu(img, "feature_images")
        if ok is not None:
            if not torch.is_tensor(ok) or ok.is_floating_point() or tuple(ok.shape) != hw:
                raise ValueError(f"a valid image must be a bool or integer [{hw[0]}, {hw[1]}] tensor")
            _need_gpu(ok, "valid_images")
    _forward_only(pc, pipe, xyz, "lift_features")
    with torch.no_grad():
        dev = xyz.device
        table = torch.zeros(R, D + 1, dtype=torch.int64, device=dev)
        row32 = None if rows is None else _rasterizer._int32_or_outside(rows, R, dev)
        for view, img, ok in zip(views, feature_images, valid_images):
            kept = _kept_pass_of_view(view, pc, pipe, bg, xyz, scaling_modifier)
            if kept is not None:
                _rasterizer.feature_votes(kept, img, valid=ok, rows=row32, num_rows=R, out=table)
        return table


# ---- Gaussians -> dense per-pixel vectors: the lifted features back in the image -----------------------------------------------
class _FeatureMapOfPass(torch.autograd.Function):
    """forward: rasterizer.feature_map over a finished pass; backward: its adjoint in the features, rasterizer.feature_votes with the
    upstream gradient as the feature image.  The geometry of the pass gets no gradient."""

    @staticmethod
    def forward(ctx, features, kept, rows, channels_last):
        out, alpha = _rasterizer.feature_map(kept, features, rows=rows, channels_last=channels_last, with_alpha=True)
        ctx.kept, ctx.rows, ctx.channels_last = kept, rows, bool(channels_last)
        ctx.shape, ctx.dtype = tuple(features.shape), features.dtype
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    def backward(ctx, grad_map, grad_alpha):
        if grad_map is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        R, D = ctx.shape
        G = grad_map.detach().to(torch.float32)
        if ctx.channels_last:
            G = G.permute(2, 0, 1)
        G = G.contiguous()
        H, W = int(G.shape[1]), int(G.shape[2])
        # The vote table is fixed point: quantum 2^-32, a partial and a cell below 2^31.  A cell is at most max|G| times the
        # weight its row collects, and a view holds at most H * W of weight, so G is brought to max|G| in [2^(t-1), 2^t) with
        # t = min(24, 30 - ceil(log2(H W))) by a power of two chosen on the device (no read-back; a zero gradient gives exponent 0 and
        # stays zero), and the table is scaled back: exact both ways, so a tiny gradient (a mean loss) keeps its relative precision.
        t = min(24, 30 - max(1, math.ceil(math.log2(H * W))))          # 24: a partial, 64 * max|G|, below 2^31 too
        _, e = torch.frexp(G.abs().amax())
        shift = (t - e).clamp(-120, 120).to(torch.int32)
        votes = _rasterizer.feature_votes(ctx.kept, torch.ldexp(G, shift), rows=ctx.rows,
                                          num_rows=None if ctx.rows is None else R)
        grad = torch.ldexp(votes_as_float(votes[:, :D]), -shift).to(ctx.dtype)
        return grad, None, None, None


FeatureMap = namedtuple("FeatureMap", "features alpha")


def render_feature_map(view, pc, pipe, bg, iteration, features, rows=None, normalize=False, channels_last=False,
                       scaling_modifier=1.0):
    """``FeatureMap(features [D,H,W] fp32 (``channels_last``: [H,W,D]), alpha [H,W] fp32)`` of one view: a feature table rendered
    through the occlusion of the full scene, in one launch whatever D is (``rasterizer.feature_map``) -- the way back from
    ``lift_features`` / ``features_from_votes`` to the image, and what ``relevancy_maps`` reads.  ``features``: floating [R, D] on
    the GPU, finite; ``rows`` [P] integers map every Gaussian to its row (``leaf_ind`` with a [leaves, D] table; outside [0, R):
    the Gaussian occludes and adds nothing), None: one row per Gaussian, R = P.  The map is ``sum alpha * T * X[row]`` with a zero
    background; ``normalize=True`` divides it by ``clamp(alpha, 1e-8)``: the blend-weighted mean feature.

    Differentiable in ``features`` (and nothing else): the backward is the adjoint kernel, ``rasterizer.feature_votes`` with the
    upstream gradient as the feature image, scaled by a power of two into its fixed-point range and back, so features of any
    width train on frozen geometry with both directions in HIP.  The geometry gets no gradient: the call raises when a model
    tensor requires grad while grad mode is on.  The pass is the UN-RESCALED one ``render()`` kept for this camera when the model
    is frozen, else one pass run here and dropped afterwards, the rule of ``render_label_map``."""
    xyz = pc.get_xyz
    _need_gpu(xyz, "the model")
    if not torch.is_tensor(features) or not features.is_floating_point() or features.dim() != 2 or features.shape[0] < 1 \
            or features.shape[1] < 1:
        raise ValueError("features must be a floating [R, D] tensor")
    _need_gpu(features, "features")
    P = xyz.shape[0]
    if rows is not None:
        if not torch.is_tensor(rows) or rows.shape != (P,):
            raise ValueError(f"rows must be a [{P}] tensor")
        _need_gpu(rows, "rows")
    elif features.shape[0] != P:
        raise ValueError(f"features must be [{P}, D] without rows, got {tuple(features.shape)}")
    _forward_only(pc, pipe, xyz, "render_feature_map")
    dev = xyz.device
    H, W, D = int(view.image_height), int(view.image_width), int(features.shape[1])
    with torch.no_grad():
        kept = _kept_pass_of_view(view, pc, pipe, bg, xyz, scaling_modifier)
        row32 = None if rows is None else _rasterizer._int32_or_outside(rows, int(features.shape[0]), dev)
    if kept is None:
        # nothing reaches a tile of this view: an empty map that still hangs on the features
        out = torch.zeros((H, W, D) if channels_last else (D, H, W), dtype=torch.float32, device=dev) + 0.0 * features.sum().float()
        return FeatureMap(out, torch.zeros(H, W, dtype=torch.float32, device=dev))
    out, alpha = _FeatureMapOfPass.apply(features, kept, row32, bool(channels_last))
    if normalize:
        out = out / (alpha[..., None] if channels_last else alpha[None]).clamp_min(1e-8)
    return FeatureMap(out, alpha)


def relevancy_maps(feature_map, text_feats, canon_feats=None, channels_last=False, chunk=1 << 16):
    """[Q, H, W] fp32: per pixel the cosine similarity of the rendered feature (``render_feature_map``: [D, H, W], or [H, W, D]
    with ``channels_last``) to every row of ``text_feats`` [Q, D]; both sides normalised as ``F.normalize`` does, so a pixel
    without a feature scores 0.  With ``canon_feats`` [K, D] (LERF's canonical negatives: "object", "things", "stuff",
    "texture") the LERF relevancy instead: ``min over k of softmax(10 * [sim_q, sim_canon_k])[0]``, 0.5 where the pixel has no
    feature.  Plain torch where the map lives, differentiable, ``chunk`` pixels at a time over views of the map: no [H * W, D]
    copy is made in either layout."""
    if feature_map.dim() != 3 or text_feats.dim() != 2:
        raise ValueError("feature_map must be [D, H, W] (or [H, W, D] with channels_last) and text_feats [Q, D]")
    H, W, D = (feature_map.shape if channels_last else (feature_map.shape[1], feature_map.shape[2], feature_map.shape[0]))
    if text_feats.shape[1] != D or (canon_feats is not None and (canon_feats.dim() != 2 or canon_feats.shape[1] != D)):
        raise ValueError(f"the map has {D} channels, text_feats / canon_feats must be [*, {D}]")
    fm = feature_map.to(torch.float32)
    norm = lambda t: torch.nn.functional.normalize(t.to(device=fm.device, dtype=torch.float32), dim=1)
    text = norm(text_feats)
    canon = None if canon_feats is None else norm(canon_feats)
    flat = fm.reshape(H * W, D) if channels_last else fm.reshape(D, H * W)
    parts = []
    for p0 in range(0, H * W, int(chunk)):
        f = flat[p0:p0 + int(chunk)] if channels_last else flat[:, p0:p0 + int(chunk)]
        length = f.norm(dim=1 if channels_last else 0).clamp_min(1e-12)
        dots = (lambda t: (t @ f.t() if channels_last else t @ f) / length[None])
        sim = dots(text)                                                       # [Q, n]
        if canon is not None:
            sim = torch.sigmoid(10.0 * (sim[:, None, :] - dots(canon)[None, :, :])).amin(dim=1)     # the pairwise softmax's first entry
        parts.append(sim)
    return torch.cat(parts, dim=1).reshape(text.shape[0], H, W)


def features_from_votes(table, min_weight=0.0):
    """``(feat [R, D] fp64, weight [R] fp64)`` of a feature-vote table [R, D + 1]: the blend-weighted mean feature of every row,
    ``sums / weight``, and the row's weight (column D) in units of blend weight.  Rows with ``weight <= min_weight`` (never seen,
    or seen too little to trust) get a zero feature.  Plain torch where the table lives."""
    if table.dim() != 2 or table.shape[1] < 2 or table.dtype is not torch.int64:
        raise ValueError(f"a feature-vote table is int64 [R, D + 1] with D >= 1, got {table.dtype} {tuple(table.shape)}")
    weight = votes_as_float(table[:, -1])
    sums = votes_as_float(table[:, :-1])
    ok = weight > float(min_weight)
    feat = torch.where(ok[:, None], sums / torch.where(ok, weight, torch.ones_like(weight))[:, None], torch.zeros_like(sums))
    return feat, weight


Codebook = namedtuple("Codebook", "leaf_ind leaf_feat occu_count dist valid")


def build_codebook(features, k, weights=None, metric="cosine", iters=10, init=None, seed=0):
    """Cluster lifted per-Gaussian features into the per-leaf table the text queries take: the training-free route
    lift -> (diffuse) -> cluster -> ``select_leaves_by_text`` / ``classify_points`` / ``render_queries``.

    ``features`` [N, D] and ``weights`` [N] are what ``features_from_votes`` returns (fp64 is cast to fp32); D up to 1024, k up to
    16384.  A row is VALID when its weight is positive (no weights: every row) and it is not all zero; the other rows are
    assigned like any row but move no centre.  ``init`` [k, D] are the starting centres, or ``None``: the valid rows at a
    ``torch.randperm`` seeded with ``seed`` (ValueError when there are fewer than k), or ``"k-means++"``: exact D^2 seeding over
    the valid rows with their weights (``kmeans.wide_seed``, HIP, drawn from ``seed``; ValueError when fewer than k distinct rows
    could be seeded) -- the start to take for scenes whose clusters differ widely in size.  ``"cosine"`` normalises the starting
    centres and keeps them unit vectors; ``"l2"`` clusters the raw vectors.  ``iters`` Lloyd iterations of
    ``kmeans.wide_lloyd`` (HIP, the same bytes every run), then the final assignment.

    Returns ``Codebook(leaf_ind [N] int64, leaf_feat [k, D] fp32, occu_count [k] int64 -- valid rows per leaf, dist [N] fp32,
    valid [N] bool)``: ``leaf_feat`` / ``occu_count`` are ``select_leaves_by_text``'s ``leaf_lang_feat`` / ``occu_count`` and
    ``leaf_ind`` is ``classify_points``'s."""
    from . import kmeans as _kmeans
    if features.dim() != 2:
        raise ValueError(f"features must be [N, D], got {tuple(features.shape)}")
    N, D = features.shape
    k = int(k)
    if weights is not None and tuple(weights.shape) != (N,):
        raise ValueError(f"weights must be [{N}], got {tuple(weights.shape)}")
    plus_plus = isinstance(init, str)
    if plus_plus and init != "k-means++":
        raise ValueError(f"init must be None, \"k-means++\" or a [{k}, {D}] tensor, got {init!r}")
    if init is not None and not plus_plus and tuple(init.shape) != (k, D):
        raise ValueError(f"init must be [{k}, {D}], got {tuple(init.shape)}")
    if metric not in _kmeans.WIDE_METRICS:
        raise ValueError(f"metric must be one of {sorted(_kmeans.WIDE_METRICS)}, got {metric!r}")
    lib = _lib.lib()
    if not 1 <= D <= lib.ogs_kmeans_wide_max_dim() or not 1 <= k <= lib.ogs_kmeans_wide_max_k():
        raise ValueError(f"D={D}, k={k}: the wide k-means takes 1 <= D <= {lib.ogs_kmeans_wide_max_dim()} and "
                         f"1 <= k <= {lib.ogs_kmeans_wide_max_k()}")
    with torch.no_grad():
        valid = (features != 0).any(dim=1)
        if weights is not None:
            valid &= weights.to(features.device) > 0
        if init is None:
            rows = torch.nonzero(valid).reshape(-1)
            if rows.numel() < k:
                raise ValueError(f"{rows.numel()} valid rows cannot seed k={k} centres")
            gen = torch.Generator().manual_seed(int(seed))
            init = features[rows[torch.randperm(rows.numel(), generator=gen)[:k].to(rows.device)]]
        _need_gpu(features, "features")
        feat = _f32(features)
        if plus_plus:
            seed_w = valid.to(torch.float32) if weights is None else torch.where(valid, weights.to(feat.device, torch.float32), 0.0)
            init, _, _, _, stats = _kmeans.wide_seed(feat, k, metric, seed_w, int(seed))
            seeded = int(stats[0])                       # the one read-back of a seeded build
            if seeded < k:
                raise ValueError(f"k-means++ could seed {seeded} of k={k} centres: too few distinct valid rows")
        centers = init.detach().to(device=feat.device, dtype=torch.float32).contiguous().clone()
        if metric == "cosine":
            centers = torch.nn.functional.normalize(centers, dim=1)
        w = valid.to(torch.float32) if weights is None else torch.where(valid, weights.to(feat.device, torch.float32), 0.0)
        ids, dist, _, _ = _kmeans.wide_lloyd(feat, centers, int(iters), metric, w)
        occu = torch.bincount(ids[valid], minlength=k)
        return Codebook(ids, centers, occu, dist, valid)


def neighbor_weights(d2, idx, valid=None, bandwidth=None):
    """Row-normalised Gaussian weights fp32 [n, K] on the kNN table of ``knn.neighbors``: ``w = exp(-d2 / (2 * h_i))`` on the
    slots that count, 0 elsewhere, every row divided by its sum.  A slot counts when ``idx >= 0``, its d2 is finite and, with
    ``valid`` (bool [R], indexed by idx), ``valid[idx]`` holds.  ``h_i`` is the mean d2 of the row's counting slots (a row
    whose counting slots are all at distance 0 weighs them equally), or ``bandwidth`` (a number or [n]) where given.  Rows
    without a counting slot stay all-zero.  Plain torch where the table lives, computed in fp64."""
    w, total = _raw_neighbor_weights(d2, idx, valid, bandwidth)
    return (w / torch.where(total > 0, total, torch.ones_like(total))).to(torch.float32)


def _raw_neighbor_weights(d2, idx, valid, bandwidth):
    """(w fp64 [n, K] before the division, their row sums fp64 [n, 1]) of ``neighbor_weights``"""
    if d2.shape != idx.shape or d2.dim() != 2:
        raise ValueError(f"d2 and idx must be [n, K] alike, got {tuple(d2.shape)} and {tuple(idx.shape)}")
    ok = (idx >= 0) & torch.isfinite(d2)
    if valid is not None:
        ok &= valid.to(torch.bool)[idx.clamp_min(0).to(torch.int64)]
    d = torch.where(ok, d2, torch.zeros_like(d2)).to(torch.float64)
    if bandwidth is None:
        h = d.sum(dim=1) / ok.sum(dim=1).clamp_min(1)
    else:
        h = torch.as_tensor(bandwidth, dtype=torch.float64, device=d2.device).expand(d2.shape[0])
    arg = torch.where(h[:, None] > 0, d / (2.0 * torch.where(h > 0, h, torch.ones_like(h)))[:, None], torch.zeros_like(d))
    w = torch.where(ok, torch.exp(-arg), torch.zeros_like(d))
    return w, w.sum(dim=1, keepdim=True)


LABEL_TABLE_BYTES = 256 << 20          # budget of the [rows, num_labels] fp32 table of one chunk of transfer_labels


def _cross_lists(src_xyz, dst_xyz, k, max_dist, index):
    """(idx, d2) of the k nearest source rows of every destination row, idx = -1 on the slots farther than max_dist"""
    if src_xyz.dim() != 2 or src_xyz.shape[1] != 3 or dst_xyz.dim() != 2 or dst_xyz.shape[1] != 3:
        raise ValueError(f"src_xyz and dst_xyz must be [n, 3] and [m, 3], got {tuple(src_xyz.shape)} and {tuple(dst_xyz.shape)}")
    if int(k) < 1:
        raise ValueError(f"k must be at least 1, got {k}")
    if max_dist is not None and not float(max_dist) >= 0:
        raise ValueError(f"max_dist must be a distance >= 0 or None, got {max_dist}")
    if index is None:
        index = _knn.Index(src_xyz)
    elif index.n != src_xyz.shape[0]:
        raise ValueError(f"index was built on {index.n} rows, src_xyz has {src_xyz.shape[0]}")
    idx, d2 = index.query(dst_xyz, int(k))
    if max_dist is not None:
        idx = torch.where(d2 <= float(max_dist) ** 2, idx, torch.full_like(idx, -1))
    return idx, d2


def transfer_labels(src_xyz, src_labels, dst_xyz, k=1, num_labels=None, max_dist=None, ignore=None, index=None):
    """Labels of one point set carried onto another by exact nearest neighbours (``knn.Index.query``), int64 [m]: every row of
    ``dst_xyz`` [m, 3] takes a label from its ``k`` nearest rows of ``src_xyz`` [n, 3] with labels ``src_labels`` [n].

    ``k = 1``: the label of the nearest source row.  ``k > 1``: the label with the largest sum of ``neighbor_weights`` over the
    k neighbours, the LOWEST label where two sums are equal.  A neighbour counts when it lies within ``max_dist`` (None: any
    distance; ``d2 <= max_dist ** 2`` on the fp32 d2), its row is not marked in ``ignore`` (bool [n]) and its label lies in
    ``[0, num_labels)``; a row without a counting neighbour gets -1.  ``num_labels=None`` takes ``src_labels.max() + 1``, the
    one value this function reads back.  ``index``: a ``knn.Index`` of ``src_xyz`` to search instead of building one.

    The sums of a chunk of rows live in a [rows, num_labels] fp32 table of at most ``LABEL_TABLE_BYTES``, filled slot by slot
    (one writer per element and slot: the same bytes every run).  The ScanNet use: ``classify_points`` on a densified model,
    this onto the GT vertices, then ``segmentation_metrics`` -- no ``--frozen_init_pts`` needed."""
    if src_labels.dim() != 1 or src_labels.shape[0] != src_xyz.shape[0]:
        raise ValueError(f"src_labels must be [{src_xyz.shape[0]}], got {tuple(src_labels.shape)}")
    if ignore is not None and ignore.shape != src_labels.shape:
        raise ValueError(f"ignore must be [{src_xyz.shape[0]}] like src_labels, got {tuple(ignore.shape)}")
    if num_labels is not None and int(num_labels) < 1:
        raise ValueError(f"num_labels must be at least 1, got {num_labels}")
    idx, d2 = _cross_lists(src_xyz, dst_xyz, k, max_dist, index)
    dev, m, k = idx.device, idx.shape[0], idx.shape[1]
    lab = src_labels.detach().to(dev).to(torch.int64)
    if num_labels is None:
        num_labels = int(lab.max()) + 1 if lab.numel() else 1
    num_labels = max(int(num_labels), 1)
    good = (lab >= 0) & (lab < num_labels)
    if ignore is not None:
        good &= ~ignore.to(dev).to(torch.bool)
    if lab.numel() == 0:                                            # no source row: every list is empty
        return torch.full((m,), -1, dtype=torch.int64, device=dev)
    slot_lab = lab[idx.clamp_min(0).to(torch.int64)]                # [m, k]; looked at only where the slot counts
    counts = (idx >= 0) & good[idx.clamp_min(0).to(torch.int64)]
    none = torch.full((m,), -1, dtype=torch.int64, device=dev)
    if k == 1:
        return torch.where(counts[:, 0], slot_lab[:, 0], none)
    w = neighbor_weights(d2, torch.where(counts, idx, torch.full_like(idx, -1)))
    out = torch.empty(m, dtype=torch.int64, device=dev)
    rows = max(1, LABEL_TABLE_BYTES // (4 * num_labels))
    every_label = torch.arange(num_labels, device=dev)
    for r0 in range(0, m, rows):
        r1 = min(m, r0 + rows)
        table = torch.zeros((r1 - r0, num_labels), dtype=torch.float32, device=dev)
        row = torch.arange(r1 - r0, device=dev)
        for s in range(k):                                          # one slot at a time: no two writers of an element
            col = torch.where(counts[r0:r1, s], slot_lab[r0:r1, s], torch.zeros_like(row))
            table[row, col] += w[r0:r1, s]                          # a slot that does not count weighs 0
        best = table.max(dim=1, keepdim=True).values
        out[r0:r1] = torch.where(table == best, every_label, num_labels).min(dim=1).values
    return torch.where(counts.any(dim=1), out, none)


def transfer_features(src_xyz, src_feat, dst_xyz, k=8, max_dist=None, valid=None, bandwidth=None, index=None):
    """Per-point rows of one point set carried onto another: ``(feat fp32 [m, D], weight fp32 [m])``, every row of ``dst_xyz``
    [m, 3] the ``neighbor_weights`` mean of ``src_feat`` [n, D] over its ``k`` exact nearest rows of ``src_xyz`` [n, 3]
    (``knn.Index.query``, then one ``knn.aggregate`` launch with R = n; no [m, k, D] buffer).

    A neighbour counts when it lies within ``max_dist`` (None: any distance) and, with ``valid`` (bool [n]), ``valid`` holds for
    its row; ``bandwidth`` as in ``neighbor_weights``.  ``weight`` is the sum of the weights BEFORE the rows are normalised: 0
    where no neighbour counts, and the feature row is then all zero.  When ``src_feat`` requires grad the sum is
    ``knn.gather_sum`` over ``knn.reverse_edges(idx, num_rows=n)``: differentiable in the features, gradients without float
    atomics.  ``index``: a ``knn.Index`` of ``src_xyz`` to search instead of building one.  Use: lifted features, codebook
    rows or ``_ins_feat`` across ``densify_and_prune``, onto another checkpoint, or onto a scan for display."""
    if src_feat.dim() != 2 or src_feat.shape[0] != src_xyz.shape[0] or src_feat.shape[1] < 1:
        raise ValueError(f"src_feat must be [{src_xyz.shape[0]}, D], got {tuple(src_feat.shape)}")
    if valid is not None and valid.shape != (src_xyz.shape[0],):
        raise ValueError(f"valid must be [{src_xyz.shape[0]}], got {tuple(valid.shape)}")
    idx, d2 = _cross_lists(src_xyz, dst_xyz, k, max_dist, index)
    n, m = src_feat.shape[0], idx.shape[0]
    if n == 0:
        return (torch.zeros((m, src_feat.shape[1]), dtype=torch.float32, device=idx.device),
                torch.zeros(m, dtype=torch.float32, device=idx.device))
    w, total = _raw_neighbor_weights(d2, idx, None if valid is None else valid.to(idx.device), bandwidth)
    w = (w / torch.where(total > 0, total, torch.ones_like(total))).to(torch.float32)
    if src_feat.requires_grad:
        feat = _knn.gather_sum(src_feat, idx, w)                    # reverse_edges(idx, num_rows=n), built in the backward
    else:
        feat = _knn.aggregate(src_feat, idx, w)
    return feat, total[:, 0].to(torch.float32)


def diffuse_features(X, idx, w, steps=1, rate=1.0, fixed=None):
    """Diffusion of per-Gaussian rows over their kNN graph, fp32 [n, D]: every step is
    ``X <- where(fixed | row_has_no_neighbour, X, (1 - rate) * X + rate * knn.aggregate(X, idx, w))`` -- one
    ``ogs_knn_aggregate`` launch, no [n, K, D] buffer.  idx, w [n, K] as ``knn.neighbors`` / ``neighbor_weights`` give them; a row
    has no neighbour when none of its slots has ``idx >= 0`` and a non-zero weight, and then keeps its value, as the ``fixed``
    rows (bool [n]) do.  ``steps = 0`` returns the input as fp32.  Forward only; ``diffuse`` is the same with a backward.

    Two uses.  FILL what ``features_from_votes`` left at zero: ``ok = weight > min_weight``;
    ``w = neighbor_weights(d2, idx, valid=ok)``; ``diffuse_features(feat, idx, w, steps, fixed=ok)`` -- unseen Gaussians take
    the weighted mean of their seen neighbours, seen ones stay, and further steps carry values into regions no seen Gaussian
    touches (pass ``valid=None`` weights for those).  SMOOTH lifted features, or a ``votes_as_float`` label table before
    ``labels_from_votes``, with ``fixed=None`` and ``rate < 1``."""
    _need_gpu(X, "X")
    if X.dim() != 2 or idx.shape != w.shape or idx.dim() != 2 or idx.shape[0] != X.shape[0]:
        raise ValueError(f"X must be [n, D] and idx, w [n, K], got {tuple(X.shape)}, {tuple(idx.shape)}, {tuple(w.shape)}")
    with torch.no_grad():
        X = _f32(X)
        keep = ~((idx >= 0) & (w != 0)).any(dim=1)
        if fixed is not None:
            keep |= fixed.to(torch.bool)
        rate = float(rate)
        for _ in range(int(steps)):
            agg = _knn.aggregate(X, idx, w)
            X = torch.where(keep[:, None], X, agg if rate == 1.0 else (1.0 - rate) * X + rate * agg)
        return X


def diffuse(X, idx, w, steps=1, rate=1.0, fixed=None, reverse=None):
    """``diffuse_features`` with a backward: the same steps, the same bytes forward, differentiable in ``X`` and ``w`` -- every
    step is one ``knn.gather_sum``, whose gradients come from the reverse-edge lists and the per-edge dots (no [n, K, D] buffer
    and no float atomics in either direction).  Which rows keep their value (``fixed``, or no slot with ``idx >= 0`` and a
    non-zero weight) is decided from the VALUES of ``w`` and carries no gradient.  ``reverse``: ``knn.reverse_edges(idx)``;
    when None the lists are built once, in the first backward, and shared by all steps."""
    _need_gpu(X, "X")
    if X.dim() != 2 or idx.shape != w.shape or idx.dim() != 2 or idx.shape[0] != X.shape[0]:
        raise ValueError(f"X must be [n, D] and idx, w [n, K], got {tuple(X.shape)}, {tuple(idx.shape)}, {tuple(w.shape)}")
    reverse = _knn.LazyReverse.of(reverse, idx, X.shape[0])
    with torch.no_grad():
        keep = ~((idx >= 0) & (w != 0)).any(dim=1)
        if fixed is not None:
            keep |= fixed.to(torch.bool)
    X = X.to(torch.float32)
    rate = float(rate)
    for _ in range(int(steps)):
        agg = _knn.gather_sum(X, idx, w, reverse)
        X = torch.where(keep[:, None], X, agg if rate == 1.0 else (1.0 - rate) * X + rate * agg)
    return X.contiguous()


class _NeighborSmoothness(torch.autograd.Function):
    @staticmethod
    def forward(ctx, F, w, idx, rev, mean):
        Fc, ic, wc = _knn._gather_args(F, idx, w)
        _, total = _knn._smoothness_fwd(Fc, ic, wc)
        if mean:                                        # over the valid slots; a graph without one has energy 0 and loss 0
            norm = torch.where(total[1] > 0, 1.0 / total[1].clamp_min(1.0), torch.zeros_like(total[1]))
        else:
            norm = torch.ones_like(total[1])
        ctx.save_for_backward(Fc, ic, wc, norm)
        ctx.rev, ctx.dtypes = rev, (F.dtype, w.dtype)
        return (total[0] * norm).to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        Fc, ic, wc, norm = ctx.saved_tensors
        scale = (grad.to(torch.float64) * norm).to(torch.float32).reshape(1).contiguous()
        begin, slots = ctx.rev.get()
        gF, gw = _knn._smoothness_bwd(Fc, ic, wc, begin, slots, scale, ctx.needs_input_grad[1])
        return (gF.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None,
                gw.to(ctx.dtypes[1]) if gw is not None else None, None, None, None)


def neighbor_smoothness(F, idx, w, reverse=None, reduction="mean"):
    """Smoothness of per-Gaussian rows over their kNN graph as a loss: ``sum_i sum_k w[i, k] * |F[i] - F[idx[i, k]]|^2`` over the
    slots with ``0 <= idx < n``, a scalar fp32 tensor, differentiable in ``F`` [n, D] and ``w`` [n, K].  ``reduction="mean"``
    divides by the number of such slots (counted on the device; 0 when there is none), ``"sum"`` does not.

    Fused in both directions (``ogs_knn_smoothness_fwd`` / ``_bwd``): the differences are taken before they are squared, so
    equal rows cost exactly 0; no [n, K, D] buffer; the total is an fp64 sum in a fixed order; the gradient of ``F`` takes its
    out-edges from ``idx`` and its in-edges from the reverse lists, one writer per element -- the same bytes every run.
    ``reverse``: ``knn.reverse_edges(idx)``, built in the first backward when None.  The row energies alone:
    ``knn.smoothness_energy``.  No double backward.  Measured forward + backward against the torch composition: 6.1 against
    16.8 ms at 2 M x 16, D = 6 (the narrow shape is the slow one per byte: one column per thread), 1.91 against 12.2 ms at
    500 k x 16, D = 64; ahead at both shapes tried."""
    if reduction not in ("mean", "sum"):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    _knn._check_gather_args(F, idx, w)
    if idx.shape[0] != F.shape[0]:
        raise ValueError(f"a square graph: idx must have the {F.shape[0]} rows of F, got {idx.shape[0]}")
    return _NeighborSmoothness.apply(F, w, idx, _knn.LazyReverse.of(reverse, idx, F.shape[0]), reduction == "mean")


def lift_mask_features(views, pc, pipe, bg, iteration, label_images, mask_feats, rows=None, num_rows=None, scaling_modifier=1.0):
    """Features that exist per 2D MASK lifted to Gaussians: ``label_images`` holds per view an [H, W] integer image of mask ids
    (the SAM ids of ``association.sam_mask_ids``; a value outside [0, L_v) is no mask) and ``mask_feats`` per view an [L_v, D]
    tensor with the feature of every mask (the reference's ``view.original_mask_feat``).  Returns ``(feat_sum [R, D] fp64,
    weight [R] fp64)``: the sum over the views and masks of (blend weight alpha * T of row r on the mask's pixels) * (the mask's
    feature), and the summed weight on masked pixels; ``feat_sum / weight`` is the row's mean feature, and with
    ``rows = leaf_ind`` a ``leaf_feat`` for ``select_leaves_by_text``.

    Per view ONE ``rasterizer.label_votes`` launch into a per-view table (reused while L_v stays the same), then
    ``votes_as_float(table[:, :L_v]) @ mask_feats[v]`` in fp64: no feature image is ever made.  It equals ``lift_features`` of the
    image F(p) = mask_feats[lab(p)] with the unmasked pixels invalid, up to fp32 rounding of that route's partials.  Pass rule and
    forward-only rule as in ``lift_labels``."""
    xyz = pc.get_xyz
    _need_gpu(xyz, "the model")
    views, label_images, mask_feats = list(views), list(label_images), list(mask_feats)
    if not (len(views) == len(label_images) == len(mask_feats)):
        raise ValueError(f"{len(views)} views, {len(label_images)} label images and {len(mask_feats)} mask feature tables")
    if not views:
        raise ValueError("need at least one view: the width of the result is that of its mask features")
    P, R = _rows_of_call(xyz, rows, num_rows)
    D = None
    for view, img, mf in zip(views, label_images, mask_feats):
        if not torch.is_tensor(img) or tuple(img.shape) != (int(view.image_height), int(view.image_width)):
            raise ValueError(f"a label image must be a [{int(view.image_height)}, {int(view.image_width)}] tensor")
        if not torch.is_tensor(mf) or not mf.is_floating_point() or mf.dim() != 2:
            raise ValueError("mask features must be a floating [L, D] tensor per view")
        D = int(mf.shape[1]) if D is None else D
        if int(mf.shape[1]) != D:
            raise ValueError(f"the mask features have {D} and {int(mf.shape[1])} channels")
        _need_gpu(img, "label_images")
        _need_gpu(mf, "mask_feats")
    _forward_only(pc, pipe, xyz, "lift_mask_features")
    with torch.no_grad():
        dev = xyz.device
        feat_sum = torch.zeros(R, D, dtype=torch.float64, device=dev)
        weight = torch.zeros(R, dtype=torch.float64, device=dev)
        row32 = None if rows is None else _rasterizer._int32_or_outside(rows, R, dev)
        table = None
        for view, img, mf in zip(views, label_images, mask_feats):
            L = int(mf.shape[0])
            kept = _kept_pass_of_view(view, pc, pipe, bg, xyz, scaling_modifier)
            if kept is None:
                continue
            if table is None or table.shape[1] != L + 1:
                table = torch.zeros(R, L + 1, dtype=torch.int64, device=dev)
            else:
                table.zero_()
            _rasterizer.label_votes(kept, img, L, rows=row32, num_rows=R, out=table)
            feat_sum, weight = _mask_votes_times_feats(table, mf, feat_sum, weight)
        return feat_sum, weight


def _mask_votes_times_feats(table, mask_feats, feat_sum, weight):
    """one view of ``lift_mask_features``: the label-vote table [R, L + 1] of the view times its mask features [L, D], in fp64;
    column L (no mask) carries no feature and no weight"""
    L = table.shape[1] - 1
    votes = votes_as_float(table[:, :L])
    return feat_sum + votes @ mask_feats.detach().to(device=table.device, dtype=torch.float64), weight + votes.sum(dim=1)


def labels_from_votes(table, min_weight=0.0, min_share=0.0):
    """``(label [R] int64, weight, second, total [R] fp64)`` of a vote table [R, L + 1]: per row the label with the largest vote
    among the columns 0..L-1 (an exact tie, decided on the integers, goes to the lowest label), that vote, the largest vote of any
    other label, and the row's whole weight, column L included.  The label is -1 where the row holds no labelled weight, where
    ``weight < min_weight`` or where ``weight / total < min_share``.  Plain torch where the table lives."""
    if table.dim() != 2 or table.shape[1] < 1 or table.dtype is not torch.int64:
        raise ValueError(f"a vote table is int64 [R, L + 1], got {table.dtype} {tuple(table.shape)}")
    R, L = table.shape[0], table.shape[1] - 1
    dev = table.device
    total = table.sum(dim=1)
    if L == 0:
        zero = torch.zeros(R, dtype=torch.float64, device=dev)
        return torch.full((R,), -1, dtype=torch.int64, device=dev), zero, zero.clone(), votes_as_float(total)
    part = table[:, :L]
    top = part.max(dim=1).values
    cols = torch.arange(L, device=dev)[None, :]
    arg = torch.where(part == top[:, None], cols, torch.full_like(cols, L)).min(dim=1).values       # first maximum: lowest label
    rest = torch.where(cols == arg[:, None], torch.full_like(part, -1), part)
    second = rest.max(dim=1).values.clamp_min(0)
    weight, total_f = votes_as_float(top), votes_as_float(total)
    # weight / total >= min_share without the quotient: total > 0 wherever top > 0
    ok = (top > 0) & (weight >= float(min_weight)) & (weight >= float(min_share) * total_f)
    label = torch.where(ok, arg, torch.full_like(arg, -1))
    return label, weight, votes_as_float(second), total_f


def leaves_from_votes(table, min_share=0.5, min_weight=1.0):
    """The selection rule of ``select_leaves_by_masks`` on a table [leaves, M + 1] lifted with ``rows = leaf_ind``: for every
    prompt m the ascending int64 ids of the leaves k with ``votes[k, m] >= min_weight`` (in units of blend weight) and
    ``votes[k, m] >= min_share * total[k]``, ``total`` being the leaf's whole visible weight, outside every prompt included."""
    if table.dim() != 2 or table.shape[1] < 1 or table.dtype is not torch.int64:
        raise ValueError(f"a vote table is int64 [R, M + 1], got {table.dtype} {tuple(table.shape)}")
    inside = votes_as_float(table[:, :-1])
    total = votes_as_float(table.sum(dim=1))
    ok = (inside > 0) & (inside >= float(min_weight)) & (inside >= float(min_share) * total[:, None])
    return [torch.nonzero(ok[:, m]).flatten() for m in range(ok.shape[1])]


def select_leaves_by_masks(views, pc, pipe, bg, iteration, prompt_images, num_prompts, leaf_ind, num_leaves, min_share=0.5,
                           min_weight=1.0):
    """Mask prompts -> leaves: ``prompt_images`` holds per view an [H, W] integer image with the value m in [0, num_prompts)
    inside prompt m (a SAM mask, a box) and -1 elsewhere.  The images are lifted with ``rows = leaf_ind`` (``lift_labels``: one
    launch per view, full-scene occlusion), and prompt m selects the leaves whose weight inside it is at least ``min_weight`` and
    at least ``min_share`` of the leaf's visible weight over the views (``leaves_from_votes``).  Returns a list of
    ``num_prompts`` ascending leaf-id tensors, what ``render_queries`` takes as ``selections``.  The two defaults (half of the
    leaf's weight, one pixel's worth of weight) are conveniences, not tuned values."""
    table = lift_labels(views, pc, pipe, bg, iteration, prompt_images, num_prompts, rows=leaf_ind, num_rows=num_leaves)
    return leaves_from_votes(table, min_share=min_share, min_weight=min_weight)


# ---- which points hang together -------------------------------------------------------------------------------------------------
def _max_d2_of(max_dist, dev):
    """max_dist squared as ONE fp32 multiply, on the device (None stays None)"""
    if max_dist is None:
        return None
    if isinstance(max_dist, torch.Tensor):
        m = max_dist.detach().to(dev).to(torch.float32).reshape(1)
    else:
        if not float(max_dist) >= 0:
            raise ValueError(f"max_dist must be a distance >= 0 or None, got {max_dist}")
        m = torch.full((1,), float(max_dist), dtype=torch.float32, device=dev)
    return m * m


def _neighbour_table(xyz, k, neighbors):
    """(idx, d2) of ``knn.neighbors(xyz, k)``, or the pair handed in"""
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"points must be [n, 3], got {tuple(xyz.shape)}")
    if neighbors is None:
        if int(k) < 1:
            raise ValueError(f"k must be at least 1, got {k}")
        return _knn.neighbors(xyz, int(k))
    idx, d2 = neighbors
    if idx.dim() != 2 or idx.shape[0] != xyz.shape[0] or d2.shape != idx.shape:
        raise ValueError(f"neighbors must be (idx, d2), both [{xyz.shape[0]}, K], got {tuple(idx.shape)} and {tuple(d2.shape)}")
    return idx, d2


def _instance_labels(xyz, labels, min_size, ignore):
    """(lab, lab32) of the instance segmentations: the labels on the device, and as int32 with -1 on every row that belongs to no
    instance (a negative label, or one that ``ignore`` names)"""
    _need_gpu(xyz, "xyz")
    _need_gpu(labels, "labels")
    n, dev = xyz.shape[0] if xyz.dim() else -1, xyz.device
    if labels.dim() != 1 or labels.shape[0] != n:
        raise ValueError(f"labels must be [{n}], got {tuple(labels.shape)}")
    if int(min_size) < 1:
        raise ValueError(f"min_size must be at least 1, got {min_size}")
    lab = labels.detach().to(dev)
    active = lab >= 0
    if ignore is not None:
        if isinstance(ignore, torch.Tensor) and ignore.dtype is torch.bool:
            if ignore.shape != lab.shape:
                raise ValueError(f"a bool ignore marks rows and must be [{n}], got {tuple(ignore.shape)}")
            active &= ~ignore.to(dev)
        else:
            active &= ~torch.isin(lab, torch.as_tensor(ignore, device=dev).to(lab.dtype).reshape(-1))
    return lab, torch.where(active, lab, torch.full_like(lab, -1)).to(torch.int32)


def _instances_of(comp, sizes, first, lab, min_size):
    """The four values of the instance segmentations from numbered components: those with fewer than ``min_size`` members are
    dropped, the rest renumbered in order"""
    keep = sizes >= int(min_size)                                   # sizes past the count are 0
    new_id = torch.cumsum(keep, dim=0, dtype=torch.int32) - 1
    num = int(keep.sum())                                           # the one read-back
    at = comp.clamp_min(0).to(torch.int64)
    instance = torch.where((comp >= 0) & keep[at], new_id[at], torch.full_like(comp, -1))
    kept = torch.argsort((~keep).to(torch.uint8), stable=True)[:num]            # the kept components, ascending
    return instance, num, lab[first[kept].to(torch.int64)], sizes[kept]


@torch.no_grad()
def segment_instances(xyz, labels, k=16, max_dist=None, min_size=1, ignore=None, neighbors=None):
    """Per-point classes -> instances: the spatially connected pieces of every class, ``(instance, num_instances,
    instance_label, instance_size)``.

    One ``knn.neighbors(xyz, k)`` call (or ``neighbors = (idx, d2)`` of an earlier one) and one ``knn.components`` call under the
    same-label rule: two points are joined when one lists the other among its k nearest, both carry the same label >= 0 and --
    with ``max_dist`` -- they lie within it (``d2 <= max_dist * max_dist``, the square one fp32 multiply).  Rows with a negative
    label, and rows whose label is named in ``ignore`` (a label value or a collection of them; a bool tensor [n] marks ROWS
    instead), belong to no instance.  Components with fewer than ``min_size`` members are dropped and the rest renumbered in
    order, so instances are numbered by ascending smallest member row.

    ``instance`` int32 [n] (-1: none), ``num_instances`` an int -- the one value this function reads back --,
    ``instance_label`` [num] in the dtype of ``labels`` and ``instance_size`` int32 [num].  A table of k <= 32 neighbours does
    not hold every point within ``max_dist`` and has no core-point rule: ``segment_instances_dbscan`` is the exact form."""
    lab, lab32 = _instance_labels(xyz, labels, min_size, ignore)
    idx, d2 = _neighbour_table(xyz, k, neighbors)
    comp, _, sizes, first = _knn.components(idx, d2, _max_d2_of(max_dist, lab.device), lab32)
    return _instances_of(comp, sizes, first, lab, min_size)


@torch.no_grad()
def segment_instances_dbscan(xyz, labels, eps, min_pts=8, min_size=1, ignore=None):
    """``segment_instances`` by exact DBSCAN instead of the kNN graph: ``(instance, num_instances, instance_label,
    instance_size)`` with the same meaning, the same ``min_size`` / ``ignore`` handling and the same one read-back.

    One ``knn.dbscan(xyz, eps, min_pts, labels)`` call under the same-label rule: a row is a core when at least ``min_pts`` rows
    of its own label (itself included) lie within ``eps``; cores within ``eps`` of each other share an instance; a non-core row
    joins the instance of its nearest core within ``eps`` and joins nothing else, so a thin bridge of sparse points between two
    objects does not merge them; rows with no core in reach are noise (-1).  Instances are numbered by ascending smallest CORE
    row, ``instance_size`` counts the border rows too."""
    lab, lab32 = _instance_labels(xyz, labels, min_size, ignore)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"points must be [n, 3], got {tuple(xyz.shape)}")
    r = _knn.dbscan(xyz, eps, min_pts, lab32)
    return _instances_of(r.cluster, r.sizes, r.first, lab, min_size)


@torch.no_grad()
def component_filter(points, group=None, num_groups=1, k=16, max_dist=None, min_share=None):
    """Keep-mask bool [n] that keeps the connected bulk of every group and drops what floats beside it -- the counterpart of
    ``knn.outlier_mask``, which removes SPARSE points but keeps a dense floater.

    ``group`` [n] integer ids (None: one group of all rows); rows with an id outside ``[0, num_groups)`` are not kept.  All
    groups go through one ``knn.neighbors(points, k)`` and one ``knn.components`` call with the group as the label: two rows are
    joined when one lists the other, both lie in the same group and -- with ``max_dist`` -- within that distance.
    ``min_share=None`` keeps the largest component of every group (equal sizes: the one whose smallest row comes first);
    otherwise every component with ``size >= min_share * rows of its group`` (compared in fp64) is kept.  The per-group
    reduction runs over per-component tensors in torch; nothing is read back.  Use: ``render_queries(..., pre_mask=
    component_filter(xyz, leaf_group, num_groups))``.  ``density_filter`` is the same filter on exact DBSCAN clusters: every
    point within ``eps`` counts, and a thin chain of sparse points joins nothing."""
    lab, G = _filter_groups(points, group, num_groups, min_share)
    idx, d2 = _neighbour_table(points, k, None)
    comp, _, sizes, first = _knn.components(idx, d2, _max_d2_of(max_dist, points.device), lab)
    return _keep_bulk(comp, sizes, first, lab, G, min_share)


@torch.no_grad()
def density_filter(points, group=None, num_groups=1, eps=None, min_pts=8, min_share=None):
    """``component_filter`` by exact DBSCAN: keep-mask bool [n] that keeps the dense bulk of every group and drops sparse points AND
    dense floaters beside it.

    All groups go through one ``knn.dbscan(points, eps, min_pts, group)`` call: clusters never cross groups, a row is kept when
    its cluster is; noise rows, and rows with an id outside ``[0, num_groups)``, are not kept.  ``min_share=None`` keeps the
    largest cluster of every group (equal sizes: the one whose smallest core row comes first); otherwise every cluster with
    ``size >= min_share * clustered rows of its group`` (compared in fp64).  ``eps`` is required: a float >= 0 or a one-element
    device tensor.  Nothing is read back.  Use: ``render_queries(..., pre_mask=density_filter(xyz, leaf_group, num_groups,
    eps=...))``."""
    if eps is None:
        raise ValueError("density_filter needs eps")
    lab, G = _filter_groups(points, group, num_groups, min_share)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [n, 3], got {tuple(points.shape)}")
    r = _knn.dbscan(points, eps, min_pts, lab)
    return _keep_bulk(r.cluster, r.sizes, r.first, lab, G, min_share)


def _filter_groups(points, group, num_groups, min_share):
    """(lab int32 [n], G) of the bulk filters: the group of every row, -1 outside ``[0, num_groups)``"""
    _need_gpu(points, "points")
    n, dev, G = points.shape[0] if points.dim() else -1, points.device, int(num_groups)
    if G < 1:
        raise ValueError(f"num_groups must be at least 1, got {num_groups}")
    if min_share is not None and not 0.0 <= float(min_share) <= 1.0:
        raise ValueError(f"min_share must lie in [0, 1] or be None, got {min_share}")
    if group is None:
        if G != 1:
            raise ValueError("group=None means one group")
        lab = torch.zeros(n if n > 0 else 0, dtype=torch.int32, device=dev)
    else:
        _need_gpu(group, "group")
        if group.shape != (n,):
            raise ValueError(f"group must be [{n}], got {tuple(group.shape)}")
        lab = torch.where((group < 0) | (group >= G), -1, group).to(torch.int32)
    return lab, G


def _keep_bulk(comp, sizes, first, lab, G, min_share):
    """The per-group reduction of the bulk filters over numbered components"""
    n, dev = comp.shape[0], comp.device
    # per component c (tensors of n entries, the ones past the count hold first = -1): its group, slot G for none
    real = first >= 0
    cgroup = torch.where(real, lab[first.clamp_min(0).to(torch.int64)], torch.full_like(first, G)).to(torch.int64)
    size64 = sizes.to(torch.int64)
    if min_share is None:
        gmax = torch.zeros(G + 1, dtype=torch.int64, device=dev).scatter_reduce(0, cgroup, size64, "amax", include_self=True)
        best = real & (size64 == gmax[cgroup])
        c = torch.arange(n, dtype=torch.int64, device=dev)
        gbest = torch.full((G + 1,), n, dtype=torch.int64, device=dev).scatter_reduce(0, cgroup, torch.where(best, c, n), "amin",
                                                                                      include_self=True)
        keep_comp = real & (c == gbest[cgroup])
    else:
        gsize = torch.zeros(G + 1, dtype=torch.int64, device=dev).index_add_(0, cgroup, size64)
        keep_comp = real & (size64.to(torch.float64) >= float(min_share) * gsize[cgroup].to(torch.float64))
    return (comp >= 0) & keep_comp[comp.clamp_min(0).to(torch.int64)]
