"""Generate tests/golden/sam_refine_golden.npz by RUNNING THE REFERENCE's own MultiViewSAMMaskRefiner.refine_sam_masks on the CPU.

Run in the build container only (``python tests/golden/make_sam_refine_golden.py``): the reference never travels, only the
vectors do.  utils/sam_refinement_utils.py is loaded by path (importlib) with ``sys.modules`` stand-ins for what it imports:
``rerun``, ``cv2``, ``matplotlib`` (+ pyplot, mpl_toolkits), ``gaussian_renderer``, ``scene.cameras``, ``scene.gaussian_model``
are empty modules carrying the names it binds; ``ashawkey_diff_gaussian_rasterization`` is the oracle-backed rasterizer of
make_render_golden.py; ``utils.sh_utils`` is the reference's own file.  Device "cuda" is mapped to the CPU and
``visualize_results`` (rerun) is a no-op.

The scene is tests/golden/sam_refine_cases.py.  Stored: the inputs and, recorded while the reference runs, the visibility
matrix, the stage-1 pairs, the id mapping and the remapped masks, per stage-2 pair the dominant id, q_max, whether the lit
footprint reaches the image border and how many labels lie under it, the winners (the reference's vote rule, restated here,
on the recorded pairs: expand_masks keeps its winner local; the final masks pin it), the final masks.  Per pair a `fragile` flag: depth-test margin under 1e-3, top minus second label sum
under 3 units of q, or q_max <= 2 -- where an implementation with another operation order may legitimately decide otherwise.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import refine_restatement as rr                       # noqa: E402  (q_gap, visibility margin: fragility only)
from tests.golden import make_render_golden as mrg               # noqa: E402
from tests.golden import sam_refine_cases as sc                  # noqa: E402

REF = "/root/reference"
NO_VOTE = rr.NO_VOTE


def load_reference_refiner():
    def module(name, **names):
        m = types.ModuleType(name)
        m.__dict__.update(names)
        sys.modules[name] = m
        return m
    module("rerun")
    module("cv2")
    mpl = module("matplotlib"); mpl.__path__ = []
    mpl.pyplot = module("matplotlib.pyplot")
    tk = module("mpl_toolkits"); tk.__path__ = []
    tk.mplot3d = module("mpl_toolkits.mplot3d", Axes3D=object)
    module("gaussian_renderer", render=None)
    scene = module("scene"); scene.__path__ = []
    module("scene.cameras", Camera=object)
    module("scene.gaussian_model", GaussianModel=object)
    module("ashawkey_diff_gaussian_rasterization", GaussianRasterizationSettings=mrg.GaussianRasterizationSettings,
           GaussianRasterizer=mrg.GaussianRasterizer)
    utils = module("utils"); utils.__path__ = []
    mrg._load_by_path("utils.sh_utils", os.path.join(REF, "utils", "sh_utils.py"))
    return mrg._load_by_path("ref_sam_refinement_utils", os.path.join(REF, "utils", "sam_refinement_utils.py"))


def main():
    ref = load_reference_refiner()
    model, cams, masks = sc.model(), sc.cameras(), sc.masks()
    N, ncam = model.get_xyz.shape[0], len(cams)
    assert int((model.get_opacity >= 0.99).sum()) >= 1001
    refiner = ref.MultiViewSAMMaskRefiner(verbose_logging=False)
    refiner.visualize_results = lambda **kw: None

    log = {"stage": 1, "pairs": {1: [], 2: []}, "image": None, "shape": {}}
    single, splat = refiner.render_single_gaussian, refiner.get_splat_id_and_weights

    def render_single_gaussian(*a, **kw):
        out = single(*a, **kw)
        log["image"] = out[0]
        return out

    def get_splat_id_and_weights(camera, gaussians, gaussian_id, sam_mask):
        dom, weights, seen = splat(camera=camera, gaussians=gaussians, gaussian_id=gaussian_id, sam_mask=sam_mask)
        q = ref.fix_image(log["image"])[:, :, 0]
        cam = [i for i, c in enumerate(cams) if c is camera][0]
        lit = q > 0
        edge = bool(lit[0].any() or lit[-1].any() or lit[:, 0].any() or lit[:, -1].any())
        log["pairs"][log["stage"]].append((int(gaussian_id), cam, int(dom), bool(seen), int(q.max()), rr.q_gap(sam_mask, q)))
        if log["stage"] == 2:
            log["shape"][int(gaussian_id), cam] = (edge, int(torch.unique(sam_mask[lit]).numel()))
        return dom, weights, seen

    remap = ref.create_consistent_id_mapping

    def create_consistent_id_mapping(m):
        log["stage"] = 2
        log["mapping"], log["refined"] = remap(m)
        return log["mapping"], log["refined"]

    refiner.render_single_gaussian, refiner.get_splat_id_and_weights = render_single_gaussian, get_splat_id_and_weights
    ref.create_consistent_id_mapping = create_consistent_id_mapping
    correspondence = {}
    project = refiner.project_3d_points_to_image_batch

    def project_3d_points_to_image_batch(camera, **kw):
        u, v, visible = project(camera=camera, **kw)
        correspondence[[i for i, c in enumerate(cams) if c is camera][0]] = visible.reshape(-1).clone()
        return u, v, visible

    refiner.project_3d_points_to_image_batch = project_3d_points_to_image_batch
    with mrg._CudaToCpu(), torch.no_grad():
        final = refiner.refine_sam_masks(cams, [m.clone() for m in masks], model, sam_level=sc.SAM_LEVEL)

    vis = torch.stack([correspondence[c] for c in range(ncam)], dim=1)
    margin = torch.stack([rr.visibility(cams[c], model.get_xyz, cams[c].depth_map)[1] for c in range(ncam)], dim=1)
    dom = np.full((N, ncam), NO_VOTE, np.int64)
    qmax = np.zeros((N, ncam), np.int64)
    fragile = (margin < 1e-3).numpy()
    found = {}
    for g, c, d, seen, qm, gap in log["pairs"][2]:
        qmax[g, c] = qm
        fragile[g, c] |= (gap < 3 and seen) or qm <= 2
        if seen:
            dom[g, c] = d
            found.setdefault(g, []).append(d)
    winners = np.full(N, NO_VOTE, np.int64)
    for g, ds in found.items():
        votes = {}
        for d in ds:
            votes[d] = votes.get(d, 0) + 1
        winners[g] = max(votes, key=votes.get)
    s1 = [(g, c, d, qm, gap) for g, c, d, seen, qm, gap in log["pairs"][1] if seen]
    n_vis = int(vis.sum())
    n_frag = int((fragile & vis.numpy()).sum())
    assert n_frag <= 0.05 * n_vis, (n_frag, n_vis)

    # the cases the scene is there for
    assert not vis[6:12].any(), "behind the camera / off-screen centres must fail the visibility test"
    assert vis[1:6].any() and (qmax[1:6][vis[1:6].numpy()] == 0).all(), "a visible pair whose every q is 0"
    assert vis[0].any() and (dom[0][vis[0].numpy()] != NO_VOTE).all(), "the whole-image footprint"
    assert len({g for g, *_ in s1}) == 2 and len(s1) >= 3, "two stage-1 Gaussians with pairs"
    first = {(c, d) for g, c, d, *_ in s1 if g == s1[0][0]}
    assert any((c, d) in first for g, c, d, *_ in s1 if g != s1[0][0]), "the second meets the first's relabelling"
    occluded = sum(int(((rr.visibility(cams[c], model.get_xyz, cams[c].depth_map, 1e9)[0]) & ~vis[:, c]).sum()) for c in range(ncam))
    assert occluded > 0, "centres in bounds but occluded"
    edge_clipped = np.zeros((N, ncam), bool)
    labels_under = np.zeros((N, ncam), np.int64)
    for (g, c), (edge, n_labels) in log["shape"].items():
        edge_clipped[g, c], labels_under[g, c] = edge, n_labels
    assert edge_clipped[1:].any(), "a footprint clipped by the image edge (other than the whole-image disc)"
    assert (labels_under == 1).any() and (labels_under > 2).any(), "a footprint inside one label, and one over several"

    store = {"visibility": vis.numpy(), "fragile": fragile, "dominant": dom, "q_max": qmax, "winners": winners,
             "stage1_pairs": np.array([(g, c, d) for g, c, d, *_ in s1], np.int64),
             "id_mapping": np.array(sorted(log["mapping"].items()), np.int64),
             "current_max_id": np.array(refiner.current_max_id), "edge_clipped": edge_clipped, "labels_under": labels_under}
    for c in range(ncam):
        store[f"refined/{c}"] = log["refined"][c].numpy()
        store[f"final/{c}"] = final[c].numpy()
        store[f"depth_map/{c}"] = cams[c].depth_map.numpy()
    store.update(sc.pack_inputs(model, cams, masks))
    path = os.path.join(HERE, "sam_refine_golden.npz")
    np.savez_compressed(path, **store)
    print("visible pairs", n_vis, "render-visible", int((dom != NO_VOTE).sum()), "fragile", n_frag, "stage-1 pairs", s1,
          "occluded", occluded, "disc seen by", vis[0].tolist())
    print("wrote", len(store), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
