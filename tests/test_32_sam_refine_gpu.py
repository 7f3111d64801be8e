"""GPU: the batched SAM-refinement kernels (opengaussian_amd/sam_refine.py, csrc/refine.hip) against the reference's loop --
tests/refine_restatement.py over this library's drop-in GaussianRasterizer, one P = 1 tiny pass per (Gaussian, camera) pair --
and against the fixture recorded from the reference's own code on the CPU oracle.

Integer outputs (visibility, q_max, dominant ids, winners, base counters) are compared exactly.  Two conditions on the inputs
are asserted first: every depth test keeps a margin of 1e-5 (the restatement and the kernel round the distance differently),
and -- the restatement sums fp32 weights where the kernels sum integers -- no pair's top two label sums tie exactly
(`q_gap` >= 1) unless every tied label holds a single pixel.  Accumulated weights: 1e-5 of the camera's largest accumulated
weight (at least 1.0, the largest single weight).  Final masks: equal except where the restatement's top two channels are
within 1e-3 or its maximum within 1e-3 of the 0.5 threshold; such pixels are first asserted to be at most 1 %.  Outside test
(a) the EXACT ties are left out of that count (they are still left out of the comparison): a Gaussian of opacity >= 0.99
saturates at q = q_max around its centre, so its weight there is exactly 1.0 -- an exact tie with the initial 1.0 of the
pixel's own label wherever that label is not the winner, which a label per pixel or a lone whole-image disc makes common."""
import os

import numpy as np
import pytest
import torch

from tests import refine_restatement as rr
from tests.golden import sam_refine_cases as sc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_refine_golden.npz")
STRIDE1 = 7          # stage-1 stride of the 64-Gaussian scenes: eight stage-1 Gaussians, later ones meet relabelled ids


def run_both(model, cams, masks, **kw):
    from opengaussian_amd import rasterizer as R
    from opengaussian_amd.sam_refine import MultiViewSAMMaskRefiner
    res = rr.refine([c.to(model.get_xyz.device) for c in cams], masks, model, sc.hip_rasterize(model), sam_level=sc.SAM_LEVEL, **kw)
    refiner = MultiViewSAMMaskRefiner()
    refiner.keep_intermediates = True
    own = [c.to(model.get_xyz.device) for c in cams]
    tiny = R.PASS_STATS["tiny"]
    out = refiner.refine_sam_masks(own, masks, model, sam_level=sc.SAM_LEVEL, **kw)
    torch.cuda.synchronize()
    return res, refiner, out, own, R.PASS_STATS["tiny"] - tiny


def near_ties(res, c):
    """(pixels left out of the mask comparison, those of them that are not exact ties)"""
    best, second = res["top2"][c]
    near = ((best - second) < 1e-3) | ((best - 0.5).abs() < 1e-3)
    return near, near & (best != second)


def check(res, refiner, out, masks, ties_allowed=False, count_exact_ties=False):
    last, live = refiner.last, res["live"]
    assert last["live"] == live
    vis = res["visibility"]
    assert float(res["depth_margin"].min()) >= 1e-5, "input condition: a depth test within rounding of its threshold"
    assert torch.equal(last["visibility"], vis)
    if not ties_allowed:
        seen = res["dominant"] != rr.NO_VOTE
        assert int(res["q_gap"][seen].min()) >= 1 if seen.any() else True, "input condition: an exact tie of label sums"
    for j, c in enumerate(live):
        assert torch.equal(last["dominant"][:, j].long().cpu(), res["dominant"][:, c]), f"dominant ids, camera {c}"
        v = vis[:, c].cpu()
        assert torch.equal(last["q_max"][c].long().cpu()[v], res["q_max"][:, c][v]), f"q_max, camera {c}"
    assert torch.equal(last["winners"].long().cpu(), res["winners"])
    for m_out, m_in in zip(out, masks):
        assert (m_out is None) == (m_in is None)
    for c in live:
        uniq = res["unique_ids"][c]
        assert torch.equal(last["unique_ids"][c], uniq)
        assert torch.equal(last["base"][c].long(), res["base"][c]), f"base counters, camera {c}"
        level = res["refined_masks"][c][sc.SAM_LEVEL]
        assert torch.equal(last["refined_masks"][c], res["refined_masks"][c])
        acc = last["accumulators"][c]
        tol = 1e-5 * max(float(res["accumulators"][c].max()), 1.0)
        assert float((acc - res["accumulators"][c]).abs().max()) <= tol, f"accumulated weights, camera {c}"
        tol = 1e-5 * float(res["channels"][c].max())
        own = (level.unsqueeze(2) == uniq.view(1, 1, -1))
        start = own.float() * ((uniq != -1).float() + last["base"][c].float()).view(1, 1, -1)
        assert float((acc + start - res["channels"][c]).abs().max()) <= tol, f"channels, camera {c}"
        tie, inexact = near_ties(res, c)
        counted = tie if count_exact_ties else inexact
        assert float(counted.float().mean()) <= 0.01, f"input condition: {int(counted.sum())} near-tie pixels in camera {c}"
        got, want = out[c], res["final_masks"][c]
        assert got.dtype == masks[c].dtype and got.device == masks[c].device and got.shape == masks[c].shape
        got = got.to(want.device)
        assert torch.equal(got[sc.SAM_LEVEL][~tie], want[sc.SAM_LEVEL][~tie]), f"final mask, camera {c}"
        keep = [l for l in range(got.shape[0]) if l != sc.SAM_LEVEL]
        assert torch.equal(got[keep], want[keep])


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def scene64(gpu_device, golden):
    model, _, _ = sc.unpack_inputs(golden)
    model = model.cut(64).to(gpu_device)
    masks = [m.to(gpu_device) for m in sc.masks(void=(4, 4))]
    return model, sc.cameras(), masks


@pytest.fixture(scope="module")
def both64(scene64):
    model, cams, masks = scene64
    return run_both(model, cams, masks, stage1_stride=STRIDE1)


def test_a_kernels_against_the_per_pair_loop(both64, scene64):
    res, refiner, out, _, _ = both64
    assert int(res["visibility"].sum()) >= 60 and int((res["winners"] != rr.NO_VOTE).sum()) >= 20
    assert sum(1 for p in res["stage1_pairs"] if p) >= 4
    check(res, refiner, out, scene64[2], count_exact_ties=True)
    assert refiner.stats["pairs"] == int(res["visibility"].sum()) and refiner.stats["slow_path_pairs"] == 0


def test_b_against_the_reference_fixture(gpu_device, golden):
    from opengaussian_amd.sam_refine import MultiViewSAMMaskRefiner
    model, cams, masks = sc.unpack_inputs(golden)
    model, cams, masks = model.to(gpu_device), [c.to(gpu_device) for c in cams], [m.to(gpu_device) for m in masks]
    refiner = MultiViewSAMMaskRefiner()
    refiner.keep_intermediates = True
    refiner.refine_sam_masks(cams, masks, model, sam_level=sc.SAM_LEVEL)
    vis, frag = golden["visibility"], golden["fragile"]
    assert (frag & vis).sum() <= 0.05 * vis.sum()
    got_vis = refiner.last["visibility"].cpu().numpy()
    assert np.array_equal(got_vis[~frag], vis[~frag])
    got_dom = refiner.last["dominant"].long().cpu().numpy()
    sure = vis & ~frag
    assert np.array_equal(got_dom[sure], golden["dominant"][sure])
    settled = ~(frag & (vis | got_vis)).any(axis=1)                 # Gaussians none of whose pairs is fragile
    assert settled.sum() >= 0.9 * len(settled)
    assert np.array_equal(refiner.last["winners"].long().cpu().numpy()[settled], golden["winners"][settled])
    assert sorted(refiner.last["id_mapping"].items()) == [tuple(r) for r in golden["id_mapping"].tolist()]
    for c in range(3):
        assert np.array_equal(refiner.last["refined_masks"][c].cpu().numpy(), golden[f"refined/{c}"])
    assert refiner.current_max_id == int(golden["current_max_id"])


def _label_case(k, width=sc.W, height=sc.H):
    """one level with ids 1..k: k - 1 single-pixel labels (row-major from a start that differs per camera), every other pixel
    in label k.  A label sum is then either one term -- equal sums are equal weights, an exact tie both sides resolve to the
    lowest id -- or the one large label, which dominates whatever reaches it; no tie hangs on the order of an fp32 sum."""
    pix = torch.arange(width * height).reshape(1, height, width)
    return [torch.clamp((pix + 7 * c) % (width * height), max=k - 1).to(torch.int64) + 1 for c in range(3)]


@pytest.mark.parametrize("labels", ["one", "every_pixel", "above_capacity", "at_capacity"])
def test_c_label_table_edges(gpu_device, scene64, labels):
    from opengaussian_amd import _lib
    cap = int(_lib.lib().ogs_refine_wave_table_capacity())
    assert sc.W * sc.H > cap + 1
    k = {"one": 1, "every_pixel": sc.W * sc.H, "above_capacity": cap + 1, "at_capacity": cap}[labels]
    model, cams, _ = scene64
    masks = [m.to(gpu_device) for m in _label_case(k)]
    res, refiner, out, _, _ = run_both(model, cams, masks, stage1_stride=STRIDE1)
    assert all(res["unique_ids"][c].numel() == k for c in res["live"])
    check(res, refiner, out, masks, ties_allowed=k > 1)           # exact one-term ties: see _label_case
    if k > cap:
        assert refiner.stats["slow_path_pairs"] > 0, "the whole-image footprint meets more labels than a wave's table holds"
    else:
        assert refiner.stats["slow_path_pairs"] == 0


def test_d_camera_without_mask_and_camera_that_sees_nothing(scene64):
    model, cams, masks = scene64
    away = sc.make_camera(sc.W, sc.H, sc.FOCAL, (0.0, 6.0, 0.3), 0.2, look_away=True)         # above everything, looking up
    cams4, masks4 = [cams[0], cams[1], away, cams[2]], [masks[0], None, masks[1], masks[2]]
    res, refiner, out, own, _ = run_both(model, cams4, masks4, stage1_stride=STRIDE1)
    assert out[1] is None and not res["visibility"][:, 1].any() and not res["visibility"][:, 2].any()
    check(res, refiner, out, masks4)
    assert torch.equal(out[2], res["refined_masks"][2])              # nothing seen: the remapped mask comes back
    assert all(hasattr(c, "depth_map") and c.depth_map.shape == (1, sc.H, sc.W) for c in own)
    assert float(own[2].depth_map.abs().max()) == 0.0


def test_d_single_gaussian(scene64):
    model, cams, masks = scene64
    res, refiner, out, _, _ = run_both(model.cut(1), cams, masks, stage1_stride=1)
    assert res["visibility"].all() and int(res["q_max"].min()) == 197           # the whole-image disc, in every camera
    check(res, refiner, out, masks)
    assert refiner.stats["pairs"] == 3


def test_d_all_votes_tied_first_camera_wins(gpu_device, scene64):
    model, cams, _ = scene64
    masks = [torch.full((1, sc.H, sc.W), i, dtype=torch.int64, device=gpu_device) for i in (5, 9, 2)]
    res, refiner, out, _, _ = run_both(model, cams, masks, stage1_stride=10 ** 6, stage1_opacity=2.0)
    dom = res["dominant"]
    three = (dom != rr.NO_VOTE).all(dim=1)
    assert three.any() and (res["winners"][three] == 2).all()        # ids 5, 9, 2 remap to 2, 3, 1; camera 0 is met first
    first = torch.tensor([[int(i) for i in row if i != rr.NO_VOTE][0] if (row != rr.NO_VOTE).any() else rr.NO_VOTE
                          for row in dom])
    assert torch.equal(res["winners"], first)
    check(res, refiner, out, masks)


@pytest.mark.parametrize("size", [(64, 64), (17, 33)])
def test_d_other_image_sizes_and_derived_camera_attributes(gpu_device, scene64, size):
    width, height = size
    model = scene64[0]
    cams = sc.cameras(width, height, sc.FOCAL * width / sc.W, full=False)
    assert not hasattr(cams[0], "cx") and not hasattr(cams[0], "projection_matrix_no_t")
    masks = [m.to(gpu_device) for m in sc.masks(width, height, block=(max(height // 4, 2), max(width // 4, 2)), void=(2, 2))]
    res, refiner, out, _, _ = run_both(model, cams, masks, stage1_stride=STRIDE1)
    assert int(res["visibility"].sum()) >= 10
    check(res, refiner, out, masks)


@pytest.mark.parametrize("labels", ["blocks", "every_pixel"])
def test_d_rectangles_above_the_wave_limit_take_a_workgroup_per_pair(gpu_device, scene64, labels, monkeypatch):
    """96 x 64: the clipped rectangle of a whole-image footprint (6144 pixels) is above what one wave walks, so its label sums
    and its expansion run a workgroup per pair; with a label per pixel K = 6144 is also above the workgroup kernel's LDS
    table, so its sums go through the zeroed global rows -- one pair per launch here, to run the chunking."""
    from opengaussian_amd import _lib, sam_refine
    width, height = 96, 64
    assert width * height > int(_lib.lib().ogs_refine_wave_max_pixels())
    model = scene64[0].cut(64)
    for i in (20, 27):                 # two more whole-image footprints, translucent: in front of the disc without hiding it
        model.get_scaling[i] = torch.tensor([2.5, 2.5, 0.002], device=gpu_device)
        model.get_rotation[i] = torch.tensor([1.0, 0.0, 0.0, 0.0], device=gpu_device)
        model.get_opacity[i] = 0.25
    cams = sc.cameras(width, height, sc.FOCAL * width / sc.W, full=False)
    if labels == "blocks":
        masks = [m.to(gpu_device) for m in sc.masks(width, height, block=(16, 24), void=(2, 2))]
    else:
        masks = [m.to(gpu_device) for m in _label_case(width * height, width, height)]
        assert int(_lib.lib().ogs_refine_block_scratch_words(width * height)) == width * height
        monkeypatch.setattr(sam_refine, "_BLOCK_SCRATCH_BYTES", 4 * width * height)
    res, refiner, out, _, _ = run_both(model, cams, masks, stage1_stride=STRIDE1)
    assert int(res["visibility"].sum()) >= 10
    check(res, refiner, out, masks, ties_allowed=labels == "every_pixel")
    st = refiner.stats
    assert st["large_rect_pairs"] >= 3 and st["large_rect_expand_pairs"] >= 1
    if labels == "every_pixel":
        assert st["global_table_pairs"] == st["large_rect_pairs"] + st["slow_path_pairs"] and st["block_launches"] >= st["global_table_pairs"]


def test_e_end_to_end(both64, scene64, gpu_device):
    from opengaussian_amd.sam_refine import MultiViewSAMMaskRefiner
    model, cams, masks = scene64
    res, refiner, out, own, tiny_passes = both64
    assert tiny_passes == 0, "the kernel path issues no per-pair rasterizer call"
    for c, cam in enumerate(own):
        assert torch.allclose(cam.depth_map, res["depth_maps"][c], rtol=1e-6, atol=1e-6)
    assert any((out[c][sc.SAM_LEVEL] != res["refined_masks"][c][sc.SAM_LEVEL]).any() for c in range(3)), "nothing expanded"
    # a second run on int32 masks held on the CPU, with the geometry states recomputed instead of kept: the same masks
    again = MultiViewSAMMaskRefiner()
    again.geom_cache_bytes = 0
    out2 = again.refine_sam_masks([c.to(gpu_device) for c in cams], [m.cpu().to(torch.int32) for m in masks], model,
                                  sam_level=sc.SAM_LEVEL, stage1_stride=STRIDE1)
    assert again.stats["geometry_recomputed"] == 6
    for a, b in zip(out, out2):
        assert b.dtype == torch.int32 and b.device.type == "cpu" and torch.equal(a.cpu().to(torch.int32), b)
    assert again.current_max_id == refiner.current_max_id == res["current_max_id"]
