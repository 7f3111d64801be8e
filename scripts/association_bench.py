"""ms per view of the 2D-3D association (train.py construct_pseudo_ins_feat, stages 2.2 and 3): the reference-structured loop
over render() + mask_ops ("old") against opengaussian_amd.association ("new"), with the peak device memory of each.

  python scripts/association_bench.py [--views 8] [--classes C4,C3] [--out profiles/association_bench.json]

Scenes: C4-class (2 M Gaussians, 648 x 484, k1 = 64, k2 = 5) and C3-class (500 k, 988 x 731, k1 = 32, k2 = 10); clusters are
spatial (nearest of k1 random centres, then of k2 sub-centres), SAM level 3 is a Voronoi label image of ~120 cells per view.
Only the per-view association work is timed (the stage-2.1 pseudo-label renders are common to both paths and not timed).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import types

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from opengaussian_amd import association as A  # noqa: E402
from opengaussian_amd import mask_ops as mo  # noqa: E402
from opengaussian_amd.renderer import render  # noqa: E402
from opengaussian_amd.synthetic import make_camera, make_scene  # noqa: E402

CLASSES = {"C4": (2_000_000, 648, 484, 520.0, 64, 5), "C3": (500_000, 988, 731, 780.0, 32, 10)}


class Model:
    def __init__(self, P, W, H, f, k1, k2, dev):
        sc = make_scene(P, W, H, f, f, seed=1, log_scale_mean=-4.0)
        self._xyz = sc.means3D.to(dev)
        self._scaling = sc.scales.to(dev)
        self._rotation = sc.rotations.to(dev)
        self._opacity = sc.opacities.to(dev)
        self._features = sc.shs.to(dev)
        g = torch.Generator(device=dev).manual_seed(2)
        centres = self._xyz[torch.randint(0, P, (k1,), generator=g, device=dev)]
        coarse = torch.cat([torch.cdist(x, centres).argmin(1) for x in self._xyz.split(1 << 18)])
        leaf = torch.empty_like(coarse)
        for c in range(k1):
            idx = torch.nonzero(coarse == c).flatten()
            sub = self._xyz[idx[torch.randint(0, max(idx.numel(), 1), (k2,), generator=g, device=dev)]] if idx.numel() else centres[:k2]
            leaf[idx] = c * k2 + torch.cdist(self._xyz[idx], sub).argmin(1)
        base = torch.randn(k1 * k2, 6, generator=g, device=dev)
        self._ins_feat = base[leaf] + 0.2 * torch.randn(P, 6, generator=g, device=dev)
        self.coarse, self.leaf = coarse, leaf
        self.active_sh_degree = self.max_sh_degree = 3
        self.iClusterSubNum = None

    get_xyz = property(lambda s: s._xyz)
    get_scaling = property(lambda s: s._scaling)
    get_rotation = property(lambda s: s._rotation)
    get_opacity = property(lambda s: s._opacity)
    get_features = property(lambda s: s._features)

    def get_ins_feat(self, origin=False):
        return F.normalize(self._ins_feat, dim=1)


class View:
    def __init__(self, k, W, H, f, dev):
        cam = make_camera(W, H, f, f, t=torch.tensor([0.05 * (k - 3.5), 0.0, 0.0]))
        for n in ("image_width", "image_height", "FoVx", "FoVy"):
            setattr(self, n, getattr(cam, n))
        self.world_view_transform = cam.world_view_transform.to(dev)
        self.full_proj_transform = cam.full_proj_transform.to(dev)
        self.camera_center = cam.camera_center.to(dev)
        self.image_name = f"v{k:02d}"
        self.data_on_gpu, self.bClusterOccur, self.cluster_masks = True, None, None
        g = torch.Generator(device=dev).manual_seed(10 + k)
        ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                                torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
        pix = torch.stack([xs.flatten(), ys.flatten()], 1)
        levels, base = [], 0
        for n in (8, 30, 60, 120):
            seeds = torch.rand(n, 2, generator=g, device=dev) * torch.tensor([W, H], device=dev)
            ids = torch.cdist(pix, seeds).argmin(1).view(H, W) + base
            ids[:, :8] = -1
            levels.append(ids)
            base = int(ids.max()) + 1
        self.original_sam_mask = torch.stack(levels)
        self.original_mask_feat = torch.randn(base, 512, generator=g, device=dev)

    def to_gpu(self):
        pass

    def to_cpu(self):
        pass


def old_stage3(views, pc, args, k1, k2):
    for v, view in enumerate(views):
        for root in range(k1):
            pkg = render(view, pc, *args, leaf_cluster_idx=pc.leaf, rescale=False, render_feat_map=False, render_cluster=True,
                         origin_feat=True, better_vis=False, selected_root_id=root, root_num=k1, leaf_num=k2)
            if not pkg["occured_leaf_id"]:
                continue
            imgs = torch.stack(pkg["leaf_clusters_imgs"])
            sil = pkg["leaf_cluster_silhouettes"] > 0.8
            ious = mo.calculate_iou(view.pesudo_mask_bool, sil)
            pred = mo.pair_mask_feature_mean(imgs, sil)
            pm = mo.mask_feature_mean(view.pesudo_ins_feat, view.pesudo_mask_bool)
            scores = ious * (1 - (pred[:, None] - pm[None]).abs().sum(2))
            scores.max(dim=-1)


def new_stage3(views, pc, args, k1, k2):
    pipe, bg = args[0], args[1]
    feat = (pc.get_ins_feat(origin=True) + 1) / 2
    for view in views:
        labels, L, pmb = A._view_labels(view)
        mask_pix = pmb.flatten(1).sum(1).float()
        pm = mo.mask_feature_mean(view.pesudo_ins_feat, pmb)
        viewed = A._viewed(view, pc, pipe, bg, feat)
        gid, kept = A._leaf_groups(view, viewed, pc.leaf, k1, k2)
        _, count, fsum, _ = A._stats_pass(view, pc, pipe, bg, A._compact(gid, kept, k1 * k2), kept.numel(), labels, L, feat, 0.8)
        inter, _, sc, fs = A.tables_from_stats(count, fsum, L)
        A.leaf_decisions(inter, fs, sc, mask_pix, pm)


def old_stage22(views, pc, args, k1, k2):
    for view in views:
        pkg = render(view, pc, *args, cluster_idx=pc.coarse, rescale=False, render_feat_map=False, render_cluster=True,
                     origin_feat=True, better_vis=True, root_num=k1, leaf_num=k2)
        occur, i = pkg["cluster_occur"], -1
        for c in range(k1):
            if not occur[c]:
                continue
            i += 1
            sil = (pkg["cluster_silhouettes"][i] > 0.9).unsqueeze(0)
            iou = mo.calculate_iou(view.pesudo_mask_bool, sil, base="former")
            inter = view.pesudo_mask_bool[iou[0] > 0.2]
            a = mo.mask_feature_mean(view.pesudo_ins_feat, inter)
            b = mo.mask_feature_mean(pkg["cluster_imgs"][i], inter, image_mask=sil)
            l1, l2 = (a - b).abs().sum(1), (a - b).pow(2).sum(1).sqrt()
            sel = inter[(l1 < 0.9) & (l2 < 0.5)]
            if sel.shape[0] > 10:
                sel = inter[torch.topk(l1, 10, largest=False)[1]]
            bool(sel.sum(0).to(torch.bool).any())


def new_stage22(views, pc, args, k1, k2):
    saved = [(v.cluster_masks, v.bClusterOccur) for v in views]
    A._stage_coarse(views, pc, args[0], args[1], render, args, pc.coarse, k1, k2, False)
    for v, (cm, oc) in zip(views, saved):
        v.cluster_masks, v.bClusterOccur = cm, oc


def timed(fn, views, *a):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    with torch.no_grad():
        fn(views, *a)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(views), (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--classes", default="C4,C3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    rargs = (pipe, torch.zeros(3, device=dev), 0)
    result = {}
    for name in args.classes.split(","):
        P, W, H, f, k1, k2 = CLASSES[name]
        pc = Model(P, W, H, f, k1, k2, dev)
        views = [View(k, W, H, f, dev) for k in range(args.views)]
        with torch.no_grad():
            for view in views:
                A.pseudo_labels(view, render(view, pc, *rargs, rescale=False, origin_feat=True)["ins_feat"], 3)
            # warm-up of both paths on one view (library load, allocator)
            new_stage3(views[:1], pc, rargs, k1, k2)
            old_stage3(views[:1], pc, rargs, k1, k2)
        row = {"P": P, "W": W, "H": H, "k1": k1, "k2": k2, "views": args.views}
        for stage, old, new in (("stage3", old_stage3, new_stage3), ("stage2_2", old_stage22, new_stage22)):
            ms_new, mb_new = timed(new, views, pc, rargs, k1, k2)
            ms_old, mb_old = timed(old, views, pc, rargs, k1, k2)
            row[stage] = {"old_ms_per_view": round(ms_old, 2), "new_ms_per_view": round(ms_new, 2),
                          "speedup": round(ms_old / ms_new, 2), "old_peak_mib": round(mb_old, 1),
                          "new_peak_mib": round(mb_new, 1)}
        result[name] = row
        print(json.dumps({name: row}), flush=True)
        del pc, views
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "result": result}, fh, indent=1)


if __name__ == "__main__":
    main()
