"""CPU: the table -> decision logic of opengaussian_amd.association against a restatement of the reference's per-cluster /
per-leaf loops (train.py construct_pseudo_ins_feat, stages 2.2 and 3) on hand-made images and masks -- no rasterizer.
Tables come both from the images (tables_from_images) and from label histograms as the statistics pass returns them."""
import torch

from opengaussian_amd import association as A

H, W, C = 24, 20, 6


def _scene(seed, G, L, thr):
    g = torch.Generator().manual_seed(seed)
    # disjoint masks: blocky label image (rows 1..L-1; row 0 and a "filtered" row stay empty, as in pesudo_mask_bool)
    coarse = torch.randint(-1, L, (H // 4, W // 4), generator=g)
    labels = coarse.repeat_interleave(4, 0).repeat_interleave(4, 1)
    labels[(labels == 0) | (labels == L - 1)] = -1
    masks = labels[None] == torch.arange(L)[:, None, None]                      # [L, H, W]
    pseudo_feat = torch.rand(L, C, generator=g)[labels.clamp_min(0)].permute(2, 0, 1) * (labels >= 0)
    # subset images: a blob of the subset's colour over a few cells, plus noise; alpha high inside the blob
    imgs = torch.empty(G, C, H, W)
    alpha = torch.zeros(G, H, W)
    for k in range(G):
        cell = coarse.flatten()[torch.randint(0, coarse.numel(), (3,), generator=g)]
        blob = torch.isin(labels, cell) | (torch.rand(H, W, generator=g) < 0.05)
        base = torch.rand(C, generator=g)
        imgs[k] = base[:, None, None] + 0.05 * torch.rand(C, H, W, generator=g)
        alpha[k] = torch.where(blob, 0.85 + 0.15 * torch.rand(H, W, generator=g), 0.5 * torch.rand(H, W, generator=g))
    # a few subsets take the pseudo features themselves: their distances are small and they get matched
    present = torch.unique(labels[labels >= 0])
    for k in range(0, G, 3):
        lk = present[torch.randint(0, present.numel(), (1,), generator=g)]
        imgs[k] = pseudo_feat + 0.01 * torch.rand(C, H, W, generator=g)
        alpha[k] = torch.where(labels == lk, torch.full((H, W), 0.95), alpha[k] * 0.5)
    return labels.to(torch.int32), masks, pseudo_feat, imgs, alpha > thr


def _stats_tables(labels, imgs, sil, L):
    """what the statistics pass returns, computed on the host from the images"""
    G = imgs.shape[0]
    bucket = torch.where(labels >= 0, labels, torch.full_like(labels, L)).long().flatten()
    count = torch.zeros(G, L + 1, dtype=torch.int64)
    fsum = torch.zeros(G, L + 1, C, dtype=torch.float64)
    for k in range(G):
        s = sil[k].flatten()
        count[k] = torch.bincount(bucket[s], minlength=L + 1)
        for c in range(C):
            fsum[k, :, c] = torch.bincount(bucket[s], weights=imgs[k, c].flatten()[s].double(), minlength=L + 1)
    return A.tables_from_stats(count, fsum.float(), L)


def _ref_mean(feat, masks, image_mask=None):
    m = masks.float() if image_mask is None else masks.float() * image_mask.float()
    return (feat[None] * m[:, None]).sum(dim=(2, 3)) / m.sum(dim=(1, 2)).clamp(min=1)[:, None]


def _restated_coarse(imgs, sils, masks, pseudo_feat):
    """stage 2.2's per-cluster loop, restated on images"""
    out = []
    for img, sil in zip(imgs, sils):
        iou = (masks & sil[None]).float().sum(dim=(1, 2)) / (masks.float().sum(dim=(1, 2)) + 1e-6)
        inters = masks[iou > 0.2]
        ids = torch.nonzero(iou > 0.2).flatten()
        a = _ref_mean(pseudo_feat, inters)
        b = _ref_mean(img, inters, sil)
        l1 = (a - b).abs().sum(dim=1)
        l2 = (a - b).pow(2).sum(dim=1).sqrt()
        keep = ids[(l1 < 0.9) & (l2 < 0.5)]
        if keep.numel() > 10:
            keep = ids[torch.topk(l1, 10, largest=False)[1]]
        out.append(keep)
    return out


def _restated_leaf(imgs, sils, masks, pseudo_feat):
    """stage 3's per-root block, restated on images: IoU, pair mean, pairwise l1, joint score, best mask"""
    inter = (sils[:, None] & masks[None]).float().sum(dim=(2, 3))
    union = (sils[:, None] | masks[None]).float().sum(dim=(2, 3)) + 1e-6
    ious = inter / union
    m = sils[:, None].float()
    pred = (imgs * m).sum(dim=(2, 3)) / (m.expand(-1, C, -1, -1).sum(dim=(2, 3)) + 1e-6)
    pm = _ref_mean(pseudo_feat, masks)
    l1 = (pred[:, None] - pm[None]).abs().sum(dim=2)
    scores = ious * (1 - l1)
    best, ind = scores.max(dim=-1)
    b = best > 0.2
    return ind * b, best * b, b, scores


def _same_selection(got, want, what):
    assert sorted(got.tolist()) == sorted(want.tolist()), f"{what}: {got.tolist()} != {want.tolist()}"


def test_coarse_decisions_match_restated_loop():
    for seed in range(6):
        L = 9 + 4 * seed
        labels, masks, pf, imgs, sils = _scene(seed, G=12, L=L, thr=0.9)
        want = _restated_coarse(imgs, sils, masks, pf)
        mask_pix = masks.flatten(1).sum(dim=1).float()
        pm = _ref_mean(pf, masks)
        assert any(w.numel() for w in want), "the scene must select some masks"
        for name, tables in (("images", A.tables_from_images(imgs, sils, masks)), ("stats", _stats_tables(labels, imgs, sils, L))):
            got = A.coarse_decisions(tables[0], tables[1], mask_pix, pm)
            for k, (g_, w_) in enumerate(zip(got, want)):
                _same_selection(g_, w_, f"seed {seed} cluster {k} ({name})")


def test_coarse_topk_over_all_intersecting_masks():
    """more than 10 masks pass the distance filter: the 10 smallest l1 over EVERY intersecting mask are taken"""
    L = 16
    labels = (torch.arange(H * W) % (L - 1) + 1).view(H, W).to(torch.int32)
    masks = labels[None] == torch.arange(L)[:, None, None]
    pf = torch.zeros(C, H, W) + 0.5
    imgs = (pf + 0.001 * torch.arange(H * W).view(1, H, W) / (H * W))[None]
    sils = torch.ones(1, H, W, dtype=torch.bool)
    want = _restated_coarse(imgs, sils, masks, pf)
    got = A.coarse_decisions(*A.tables_from_images(imgs, sils, masks)[:2], masks.flatten(1).sum(dim=1).float(), _ref_mean(pf, masks))
    assert want[0].numel() == 10
    _same_selection(got[0], want[0], "topk")


def test_leaf_decisions_match_restated_loop():
    for seed in range(6):
        L = 7 + 5 * seed
        labels, masks, pf, imgs, sils = _scene(100 + seed, G=15, L=L, thr=0.8)
        want = _restated_leaf(imgs, sils, masks, pf)
        mask_pix = masks.flatten(1).sum(dim=1).float()
        pm = _ref_mean(pf, masks)
        assert bool(want[2].any()) and not bool(want[2].all()), "the scene must match some leaves and not others"
        for name, tables in (("images", A.tables_from_images(imgs, sils, masks)), ("stats", _stats_tables(labels, imgs, sils, L))):
            inter, _, sil_count, feat_sil = tables
            ind, score, b, scores = A.leaf_decisions(inter, feat_sil, sil_count, mask_pix, pm)
            assert torch.allclose(scores, want[3], atol=1e-5), name
            assert torch.allclose(score, want[1], atol=1e-5), name
            top2 = want[3].topk(2, dim=1).values
            clear = ((top2[:, 0] - top2[:, 1]) > 1e-5) & ((want[1] - 0.2).abs() > 1e-5)
            assert torch.equal(b[clear], want[2][clear]), name
            assert torch.equal(ind[clear], want[0][clear]), name


def test_label_image_of_mask_rows():
    labels = torch.tensor([[-1, 1, 1], [2, 2, -1]], dtype=torch.int32)
    rows = labels[None] == torch.arange(4)[:, None, None]
    assert torch.equal(A.labels_of_mask_rows(rows), labels)
    rows[3, 0, 0] = rows[3, 0, 1] = True                  # row 3 overlaps row 1 at (0, 1)
    assert A.labels_of_mask_rows(rows) is None
    empty = torch.zeros(0, 2, 3, dtype=torch.bool)
    assert torch.equal(A.labels_of_mask_rows(empty), torch.full((2, 3), -1, dtype=torch.int32))


def test_sam_mask_ids_match_reference_numbering():
    """ids relative to the previous level, -1 (and anything below) -> 0 = invalid"""
    sam = torch.tensor([[[0, 1], [2, -1]], [[3, 4], [-1, 5]]])
    assert torch.equal(A.sam_mask_ids(sam, 1), torch.tensor([[1, 2], [0, 3]]))
    assert torch.equal(A.sam_mask_ids(sam, 0), torch.tensor([[1, 2], [3, 0]]))
