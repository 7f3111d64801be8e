"""GPU: association.construct_pseudo_ins_feat (grouped label statistics) against a restatement of the reference's
construct_pseudo_ins_feat loops written on render() + mask_ops (which the goldens pin to the reference): pseudo labels,
stage 2.2 (mode="leaf") and stage 3 (mode="lang") on a synthetic scene of 6 cameras with 4-level SAM label images made of
Voronoi cells, and the CPU RNG state afterwards."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from opengaussian_amd.synthetic import make_camera

pytestmark = pytest.mark.gpu

W, H, FOC = 96, 72, 80.0
K1, K2 = 6, 4
V = 6
LANG_DIM = 8


class _Model:
    """what render() and the drivers read from GaussianModel"""

    def __init__(self, dev, seed=0):
        g = torch.Generator().manual_seed(seed)
        P = 5000
        centres = torch.stack([torch.rand(K1, generator=g) * 2.4 - 1.2, torch.rand(K1, generator=g) * 1.6 - 0.8,
                               torch.rand(K1, generator=g) * 2 + 4], dim=1)
        coarse = torch.randint(0, K1, (P,), generator=g)
        sub = torch.randn(K1, K2, 3, generator=g) * 0.25
        leaf_local = torch.randint(0, K2, (P,), generator=g)
        xyz = centres[coarse] + sub[coarse, leaf_local] + torch.randn(P, 3, generator=g) * 0.08
        leaf = coarse * K2 + leaf_local
        leaf[:40] = K1 * K2                                   # the dummy leaf id
        small = (leaf == 5)                                   # a leaf with fewer than 10 points
        leaf[small.nonzero().flatten()[5:]] = 4
        base = torch.randn(K1 * K2 + 1, 6, generator=g)
        self._xyz = xyz.to(dev)
        self._scaling = torch.exp(torch.randn(P, 3, generator=g) * 0.3 - 3.3).to(dev)
        q = torch.randn(P, 4, generator=g)
        self._rotation = (q / q.norm(dim=1, keepdim=True)).to(dev)
        self._opacity = torch.sigmoid(torch.randn(P, 1, generator=g) + 2.0).to(dev)
        self._features = (0.3 * torch.randn(P, 16, 3, generator=g)).to(dev)
        self._ins_feat = (base[leaf] + 0.15 * torch.randn(P, 6, generator=g)).to(dev)
        self.coarse, self.leaf = coarse.to(dev), leaf.to(dev)
        self.active_sh_degree = self.max_sh_degree = 3
        self.iClusterSubNum = None

    get_xyz = property(lambda s: s._xyz)
    get_scaling = property(lambda s: s._scaling)
    get_rotation = property(lambda s: s._rotation)
    get_opacity = property(lambda s: s._opacity)
    get_features = property(lambda s: s._features)

    def get_ins_feat(self, origin=False):
        return F.normalize(self._ins_feat, dim=1)


class _View:
    def __init__(self, k, dev, model):
        cam = make_camera(W, H, FOC, FOC, t=torch.tensor([0.15 * (k - 2.5), 0.05 * (k % 3 - 1), 0.0]))
        for name in ("image_width", "image_height", "FoVx", "FoVy"):
            setattr(self, name, getattr(cam, name))
        self.world_view_transform = cam.world_view_transform.to(dev)
        self.full_proj_transform = cam.full_proj_transform.to(dev)
        self.camera_center = cam.camera_center.to(dev)
        self.image_name = f"view_{5 - k:02d}"
        self.data_on_gpu = True
        self.bClusterOccur = None
        self.cluster_masks = None
        self.pesudo_ins_feat = self.pesudo_mask_bool = None
        # 4 SAM levels: Voronoi cells of projected Gaussians, ids continuing from the previous level; -1 = invalid
        g = torch.Generator().manual_seed(100 + k)
        p = model._xyz.cpu()
        uv = torch.stack([p[:, 0] / p[:, 2] * FOC + W / 2 + 0.15 * (k - 2.5) / p[:, 2] * FOC,
                          p[:, 1] / p[:, 2] * FOC + H / 2], dim=1)
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        pix = torch.stack([xs.flatten(), ys.flatten()], dim=1)
        levels, base = [], 0
        for n_cells in (3, 6, 12, 20):
            seeds = uv[torch.randint(0, p.shape[0], (n_cells,), generator=g)]
            cell = torch.cdist(pix, seeds).argmin(dim=1).view(H, W)
            ids = cell + base
            ids[:, :4] = -1
            ids[(torch.rand(H, W, generator=g) < 0.02)] = -1
            levels.append(ids)
            base = int(ids.max()) + 1
        self.original_sam_mask = torch.stack(levels).to(dev)
        self.original_mask_feat = torch.randn(base, LANG_DIM, generator=g).to(dev)

    def to_gpu(self):
        self.data_on_gpu = True

    def to_cpu(self):
        self.data_on_gpu = False


class _Scene:
    def __init__(self, model, views, path):
        self.gaussians, self._views, self.model_path = model, views, path

    def getTrainCameras(self):
        return list(self._views)


# ---- the reference's loops, restated on render() + mask_ops ------------------------------------------------------------
def _restated(scene, render_args, mode, cluster_indices, root_num=K1, leaf_num=K2, sam_level=3):
    from opengaussian_amd import mask_ops as mo
    from opengaussian_amd.renderer import render
    pc = scene.gaussians
    views = sorted(scene.getTrainCameras(), key=lambda c: c.image_name)
    for view in views:
        feat = render(view, pc, *render_args, rescale=False, origin_feat=True)["ins_feat"]
        sam = view.original_sam_mask
        mid = sam[sam_level].clone() - (sam[sam_level - 1].max().cpu() + 1)
        mid = mid.clamp_min(-1) + 1
        onehot = F.one_hot(mid.long(), num_classes=int(mid.max()) + 1).permute(2, 0, 1)
        mid = onehot.argmax(dim=0)
        mask_bool = onehot[1:]
        mean, var, cnt = mo.mask_feature_mean(feat, mask_bool, return_var=True)
        mean = torch.cat((torch.zeros(1, 6, device=mean.device), mean))
        drop = torch.cat((torch.tensor([False], device=var.device), var > 0.006))
        drop[torch.nonzero(cnt > cnt.max() * 0.8).squeeze() + 1] = False
        fm = mean.clone()
        fm[drop] *= 0
        view.pesudo_ins_feat = fm[mid].permute(2, 0, 1)
        mb = torch.cat((torch.zeros_like(mask_bool[:1]), mask_bool))
        mb[drop] *= 0
        view.pesudo_mask_bool = mb.to(torch.bool)
    if mode == "leaf":
        sub = torch.ones(cluster_indices.max() + 1).to(torch.int32)
        for view in views:
            pkg = render(view, pc, *render_args, cluster_idx=cluster_indices, rescale=False, render_feat_map=False,
                         render_cluster=True, origin_feat=True, better_vis=True, root_num=root_num, leaf_num=leaf_num)
            occur, masks, i = pkg["cluster_occur"], [], -1
            for c in range(int(cluster_indices.max()) + 1):
                if not occur[c]:
                    continue
                i += 1
                sil = (pkg["cluster_silhouettes"][i] > 0.9).unsqueeze(0)
                iou = mo.calculate_iou(view.pesudo_mask_bool, sil, base="former")
                inter = view.pesudo_mask_bool[iou[0] > 0.2]
                a = mo.mask_feature_mean(view.pesudo_ins_feat, inter)
                b = mo.mask_feature_mean(pkg["cluster_imgs"][i], inter, image_mask=sil)
                l1, l2 = (a - b).abs().sum(1), (a - b).pow(2).sum(1).sqrt()
                chosen = inter[(l1 < 0.9) & (l2 < 0.5)]
                if chosen.shape[0] > 10:
                    chosen = inter[torch.topk(l1, 10, largest=False)[1]]
                union = chosen.sum(0).to(torch.bool)
                if not union.any():
                    occur[c] = False
                    continue
                masks.append(union)
                sub[c] = max(sub[c], chosen.shape[0])
            if view.cluster_masks is None:
                view.cluster_masks, view.bClusterOccur = masks, occur
        pc.iClusterSubNum = (sub + 1).clamp(max=leaf_num)
        return None
    scores_of = {}
    match = torch.zeros(root_num * leaf_num, len(views), 3).cuda()
    for root in range(root_num):
        for v, view in enumerate(views):
            pkg = render(view, pc, *render_args, leaf_cluster_idx=cluster_indices, rescale=False, render_feat_map=False,
                         render_cluster=True, origin_feat=True, better_vis=False, selected_root_id=root,
                         root_num=root_num, leaf_num=leaf_num)
            ids = pkg["occured_leaf_id"]
            if len(ids) == 0:
                continue
            imgs = torch.stack(pkg["leaf_clusters_imgs"])
            sil = pkg["leaf_cluster_silhouettes"] > 0.8
            ious = mo.calculate_iou(view.pesudo_mask_bool, sil)
            pred = mo.pair_mask_feature_mean(imgs, sil)
            pm = mo.mask_feature_mean(view.pesudo_ins_feat, view.pesudo_mask_bool)
            scores = ious * (1 - (pred[:, None] - pm[None]).abs().sum(2))
            best, ind = scores.max(dim=-1)
            ok = best > 0.2
            best[~ok] *= 0
            ind[~ok] *= 0
            match[torch.tensor(ids).cuda(), v] = torch.stack((ind, best, ok), dim=1).float()
            for k, leaf in enumerate(ids):
                scores_of[(leaf, v)] = scores[k]
    return match, scores_of


def _setup(dev, tmp, name, occur=None):
    model = _Model(dev)
    views = [_View(k, dev, model) for k in range(V)]
    if occur is not None:
        for v in views:
            v.bClusterOccur = occur.clone()
    path = os.path.join(tmp, name)
    os.makedirs(path, exist_ok=True)
    return _Scene(model, views, path)


def _args(dev):
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    return (pipe, torch.tensor([0.1, 0.3, 0.2], device=dev), 0)


def _sorted(scene):
    return sorted(scene.getTrainCameras(), key=lambda c: c.image_name)


def test_stage_2_2_matches_restated_loop(gpu_device, tmp_path):
    from opengaussian_amd.association import construct_pseudo_ins_feat
    from opengaussian_amd.renderer import render
    dev = gpu_device
    with torch.no_grad():
        a, b = _setup(dev, str(tmp_path), "a"), _setup(dev, str(tmp_path), "b")
        torch.manual_seed(7)
        _restated(a, _args(dev), "leaf", a.gaussians.coarse)
        state_ref = torch.get_rng_state()
        torch.manual_seed(7)
        construct_pseudo_ins_feat(b, render, _args(dev), cluster_indices=b.gaussians.coarse, mode="leaf", root_num=K1,
                                  leaf_num=K2)
        assert torch.equal(torch.get_rng_state(), state_ref)
    occurring = 0
    for va, vb in zip(_sorted(a), _sorted(b)):
        assert torch.equal(va.pesudo_mask_bool, vb.pesudo_mask_bool), va.image_name
        assert torch.allclose(va.pesudo_ins_feat, vb.pesudo_ins_feat, atol=1e-6), va.image_name
        assert vb.bClusterOccur.device.type == "cpu" and vb.bClusterOccur.dtype == torch.bool
        assert torch.equal(va.bClusterOccur, vb.bClusterOccur), va.image_name
        assert len(va.cluster_masks) == len(vb.cluster_masks)
        for ma, mb in zip(va.cluster_masks, vb.cluster_masks):
            assert torch.equal(ma, mb), va.image_name
        occurring += int(va.bClusterOccur.sum())
    assert occurring > 0, "the scene must associate some coarse clusters"
    assert torch.equal(a.gaussians.iClusterSubNum, b.gaussians.iClusterSubNum)


@pytest.mark.parametrize("with_occur", [False, True])
def test_stage_3_matches_restated_loop(gpu_device, tmp_path, with_occur):
    from opengaussian_amd.association import construct_pseudo_ins_feat, write_cluster_lang
    from opengaussian_amd.renderer import render
    dev = gpu_device
    occur = None
    if with_occur:
        occur = torch.ones(K1, dtype=torch.bool)
        occur[2] = False
    with torch.no_grad():
        a, b = _setup(dev, str(tmp_path), "a", occur), _setup(dev, str(tmp_path), "b", occur)
        torch.manual_seed(3)
        match_ref, scores_of = _restated(a, _args(dev), "lang", a.gaussians.leaf)
        write_cluster_lang(a, _sorted(a), match_ref, a.gaussians.leaf, K1, K2, 3, False)
        state_ref = torch.get_rng_state()
        torch.manual_seed(3)
        match_got = construct_pseudo_ins_feat(b, render, _args(dev), cluster_indices=b.gaussians.leaf, mode="lang",
                                              root_num=K1, leaf_num=K2)
        assert torch.equal(torch.get_rng_state(), state_ref)
    for va, vb in zip(_sorted(a), _sorted(b)):
        assert torch.equal(va.pesudo_mask_bool, vb.pesudo_mask_bool)
    za = np.load(os.path.join(a.model_path, "cluster_lang.npz"))
    zb = np.load(os.path.join(b.model_path, "cluster_lang.npz"))
    assert np.array_equal(za["leaf_ind"], zb["leaf_ind"])
    assert float(match_ref[:, :, 2].sum()) > 0, "the scene must match some leaves"
    if with_occur:
        assert not match_got[2 * K2:3 * K2].any()
    # the leaves rendered nowhere: zero rows in both (the dummy leaf, the leaf with 5 points, the unseen root)
    seen = torch.zeros(K1 * K2, V, dtype=torch.bool)
    for leaf, v in scores_of:
        seen[leaf, v] = True
    assert not match_got[~seen.to(match_got.device)].any()
    assert not seen[5].any()
    # per (leaf, view): the same mask id and b_matched unless the best score sits within 1e-5 of 0.2 or of the runner-up
    flips = 0
    for (leaf, v), sc in scores_of.items():
        top = sc.topk(min(2, sc.numel())).values
        near = abs(float(top[0]) - 0.2) < 1e-5 or (top.numel() > 1 and float(top[0] - top[1]) < 1e-5)
        want, got = match_ref[leaf, v], match_got[leaf, v]
        if near and not torch.equal(want[[0, 2]], got[[0, 2]]):
            flips += 1
            continue
        assert torch.equal(want[[0, 2]], got[[0, 2]]), (leaf, v, want, got)
        assert abs(float(want[1] - got[1])) <= 1e-5, (leaf, v, want, got)
    if flips == 0:
        for k in ("leaf_feat", "leaf_score", "occu_count"):
            assert np.allclose(za[k], zb[k], atol=1e-5, rtol=1e-5), k
