"""Open-vocabulary query step, measured (run on the MI355X; writes profiles/query_bench.json).

Object pass   C3-class synthetic scene (500 k Gaussians, 988 x 731), K = 320 random leaves, Q = 14 and Q = 21 queries of 1-3
              leaves each, one frame:
                new     query.render_queries -- one preprocess, one split, one kNN launch, one grouped pass
                parent  the loop of Q render(selected_leaf_id=...) calls, which is what a user had before
              one process, alternating legs, 3 repeats after a warm-up of each; the images of the two legs are compared.
              The kernels of one `new` call are listed once, outside the timed window (HIP events per launch).
Point eval    N = 2 M points, 19 class texts, K = 320 leaves, D = 512:
                new        query.classify_points + query.segmentation_metrics
                reference  the reference's route as it runs it: similarity / argmax / gather on the GPU, then everything moved
                           to the CPU and 4 reductions per class there (scripts/eval_scannet.py:55-93,157-165, restated)
                torch_gpu  the same classes, then a torch.bincount confusion table on the GPU and the same metrics from it
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opengaussian_amd import _lib, query                      # noqa: E402
from opengaussian_amd.renderer import render                  # noqa: E402
from opengaussian_amd.synthetic import make_camera, make_scene  # noqa: E402

REPEATS = 3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(legs, repeats=REPEATS):
    """{name: {"ms": [...], "median": m, "min": a, "max": b}} -- every leg warmed once, then the legs in turn, `repeats` times"""
    for fn in legs.values():
        fn()
    times = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            times[name].append(timed(fn)[0])
    return {name: dict(ms=[round(t, 3) for t in ts], median=round(statistics.median(ts), 3), min=round(min(ts), 3),
                       max=round(max(ts), 3)) for name, ts in times.items()}


class Model:
    """what render() reads of the reference's GaussianModel, frozen"""

    def __init__(self, sc, dev):
        self._xyz, self._scaling, self._rotation = sc.means3D.to(dev), sc.scales.to(dev), sc.rotations.to(dev)
        self._opacity, self._features, self._ins_feat = sc.opacities.to(dev), sc.shs.to(dev), (sc.ins_feat.to(dev) * 2 - 1)
        self.active_sh_degree = self.max_sh_degree = 3

    get_xyz = property(lambda s: s._xyz)
    get_scaling = property(lambda s: s._scaling)
    get_rotation = property(lambda s: s._rotation)
    get_opacity = property(lambda s: s._opacity)
    get_features = property(lambda s: s._features)

    def get_ins_feat(self, origin=False):
        return F.normalize(self._ins_feat, dim=1)


def object_pass(dev):
    P, W, H, f, K = 500_000, 988, 731, 800.0, 320
    pc = Model(make_scene(P, W, H, f, f, seed=0), dev)
    cam = make_camera(W, H, f, f).to(dev)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = torch.zeros(3, device=dev)
    g = torch.Generator().manual_seed(0)
    leaf = torch.randint(0, K, (P,), generator=g).to(dev)
    out = {"scene": dict(P=P, W=W, H=H, leaves=K), "runs": []}
    for Q in (14, 21):
        sels = [torch.randperm(K, generator=g)[:int(torch.randint(1, 4, (1,), generator=g))].to(dev) for _ in range(Q)]
        kw = dict(better_vis=True, seg_rgb=True, post_process=True, root_num=64, leaf_num=5)

        def new():
            with torch.no_grad():
                return query.render_queries(cam, pc, pipe, bg, 0, leaf, sels, **kw)

        def parent():
            with torch.no_grad():
                return [render(cam, pc, pipe, bg, 0, rescale=False, leaf_cluster_idx=leaf, selected_leaf_id=s, render_feat_map=False,
                               render_cluster=False, **kw) for s in sels]
        res = alternate({"new": new, "parent": parent})
        a, b = new(), parent()
        same = sum(int((a.images[q] is None and not b[q]["leaf_clusters_imgs"]) or
                       (a.images[q] is not None and len(b[q]["leaf_clusters_imgs"]) == 1 and
                        torch.equal(a.images[q], b[q]["leaf_clusters_imgs"][0][:3]) and
                        torch.equal(a.silhouettes[q], b[q]["leaf_cluster_silhouettes"][0:1]))) for q in range(Q))
        del a, b
        _lib.prof_enable(1)
        new()
        kernels = _lib.prof_collect()
        _lib.prof_enable(0)
        res.update(Q=Q, leaves_per_query=[int(s.numel()) for s in sels], images_bit_equal=f"{same}/{Q}",
                   speedup_median=round(res["parent"]["median"] / res["new"]["median"], 2),
                   new_kernels_ms={k: round(v["total_ms"], 3) for k, v in sorted(kernels.items(), key=lambda kv: -kv[1]["total_ms"])},
                   new_kernel_ms_total=round(sum(v["total_ms"] for v in kernels.values()), 3))
        print(json.dumps(res), flush=True)
        out["runs"].append(res)
    return out


def reference_route(text, leaf_feat, occu, leaf_ind, gt, C):
    """eval_scannet.py:143-144,158-165 restated: classes on the GPU, metrics on the CPU with one reduction per class and kind"""
    lf = leaf_feat.clone()
    lf[occu < 2] *= 0.0
    sim = F.normalize(text, dim=1) @ F.normalize(lf, dim=1).t()
    pred = torch.argmax(sim, dim=0)[leaf_ind.clamp(max=lf.shape[0] - 1)] + 1
    gt, pred = gt.cpu(), pred.cpu()
    pred[gt == 0] = 0
    inter, union, total, ious = torch.zeros(C), torch.zeros(C), torch.zeros(C), torch.zeros(C)
    for c in range(1, C):
        inter[c] = torch.sum((gt == c) & (pred == c)).item()
        union[c] = torch.sum((gt == c) | (pred == c)).item()
        total[c] = torch.sum(gt == c).item()
    ok = union != 0
    ious[ok] = inter[ok] / union[ok]
    present = torch.unique(gt)
    present = present[present != 0]
    valid = gt != 0
    n_valid = torch.sum(valid).item()
    acc = torch.sum((gt == pred) & valid).item() / n_valid if n_valid > 0 else float("nan")
    return ious, ious[present].mean().item(), acc, (inter / total)[present].mean().item()


def torch_gpu_route(text, leaf_feat, occu, leaf_ind, gt, C):
    lf = leaf_feat.clone()
    lf[occu < 2] *= 0.0
    sim = F.normalize(text, dim=1) @ F.normalize(lf, dim=1).t()
    pred = torch.argmax(sim, dim=0)[leaf_ind.clamp(max=lf.shape[0] - 1)] + 1
    pred = torch.where(gt == 0, torch.zeros_like(pred), pred)
    conf = torch.bincount(gt * C + pred, minlength=C * C).reshape(C, C)
    return query.metrics_from_confusion(conf)


def point_eval(dev):
    N, T, K, D = 2_000_000, 19, 320, 512
    g = torch.Generator().manual_seed(1)
    text, leaf_feat = torch.randn(T, D, generator=g).to(dev), torch.randn(K, D, generator=g).to(dev)
    occu = torch.randint(0, 20, (K,), generator=g).to(dev)
    leaf_ind = torch.randint(0, K + 1, (N,), generator=g).to(dev)
    gt = torch.randint(0, T + 1, (N,), generator=g).to(dev)
    C = T + 1
    legs = {"new": lambda: query.segmentation_metrics(gt, query.classify_points(text, leaf_feat, occu, leaf_ind), C),
            "reference": lambda: reference_route(text, leaf_feat, occu, leaf_ind, gt, C),
            "torch_gpu": lambda: torch_gpu_route(text, leaf_feat, occu, leaf_ind, gt, C)}
    res = alternate(legs)
    a, b, c = (fn() for fn in legs.values())
    res.update(N=N, classes=T, leaves=K, D=D, ious_equal_reference=bool(torch.equal(a[0], b[0])),
               ious_equal_torch_gpu=bool(torch.equal(a[0], c[0])), scalars_equal_reference=list(a[1:]) == list(b[1:]),
               speedup_vs_reference=round(res["reference"]["median"] / res["new"]["median"], 1),
               speedup_vs_torch_gpu=round(res["torch_gpu"]["median"] / res["new"]["median"], 2))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_properties(0).name, "ogs_version": int(_lib.lib().ogs_version()), "repeats": REPEATS,
           "point_eval": point_eval(dev), "object_pass": object_pass(dev)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
