"""CPU: the SAM-refinement restatement (tests/refine_restatement.py) over the CPU oracle against the fixture recorded from the
reference's own refine_sam_masks (tests/golden/make_sam_refine_golden.py) -- the same rasterizer on both sides, so every
integer output and every mask is equal, no tolerance -- and the product's host-side stage 1 (label-class tables) against the
restatement's sequential pixel relabelling."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests import refine_restatement as rr
from tests.golden import sam_refine_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_refine_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def restated(golden):
    model, cams, masks = sc.unpack_inputs(golden)
    return rr.refine(cams, masks, model, sc.oracle_rasterize(model), sam_level=sc.SAM_LEVEL), cams


def test_fixture_inputs_are_the_scene_of_the_cases_module(golden):
    model, cams, masks = sc.unpack_inputs(golden)
    fresh = sc.model()
    for f in ("get_xyz", "get_opacity", "get_scaling", "get_rotation", "get_features"):
        assert torch.allclose(getattr(model, f), getattr(fresh, f), rtol=1e-6, atol=1e-7), f
    for got, want in zip(masks, sc.masks()):
        assert torch.equal(got, want)
    assert int((model.get_opacity >= 0.99).sum()) >= 1001 and model.get_xyz.shape[0] == sc.N_FULL
    assert all(-1 in m and 0 in m for m in masks)


def test_restatement_reproduces_the_reference_run(golden, restated):
    res, cams = restated
    ncam = len(cams)
    assert np.array_equal(res["visibility"].numpy(), golden["visibility"])
    pairs = [(g, c, d) for g, ps in zip(res["stage1_gaussians"], res["stage1_pairs"]) for c, d in ps]
    assert np.array_equal(np.array(pairs, np.int64).reshape(-1, 3), golden["stage1_pairs"])
    assert sorted(res["id_mapping"].items()) == [tuple(r) for r in golden["id_mapping"].tolist()]
    assert res["current_max_id"] == int(golden["current_max_id"])
    assert np.array_equal(res["dominant"].numpy(), golden["dominant"])
    vis = golden["visibility"]
    assert np.array_equal(res["q_max"].numpy()[vis], golden["q_max"][vis])
    assert np.array_equal(res["winners"].numpy(), golden["winners"])
    for c in range(ncam):
        assert np.array_equal(res["depth_maps"][c].numpy(), golden[f"depth_map/{c}"])
        assert np.array_equal(res["refined_masks"][c].numpy(), golden[f"refined/{c}"]), c
        assert np.array_equal(res["final_masks"][c].numpy(), golden[f"final/{c}"]), c
    assert any((golden[f"final/{c}"][sc.SAM_LEVEL] != golden[f"refined/{c}"][sc.SAM_LEVEL]).any() for c in range(ncam))


def test_fixture_covers_its_cases_and_keeps_the_fragile_share(golden):
    vis, frag, qmax, dom = golden["visibility"], golden["fragile"], golden["q_max"], golden["dominant"]
    assert (frag & vis).sum() <= 0.05 * vis.sum()
    assert not vis[6:12].any()                                      # behind the cameras, off-screen
    assert vis[1:6].any() and (qmax[1:6][vis[1:6]] == 0).all()      # visible, every q = 0
    assert vis[0].any() and (qmax[0][vis[0]] == 197).all()          # the whole-image disc
    s1 = golden["stage1_pairs"]
    assert len(set(s1[:, 0].tolist())) == 2
    first = {(c, d) for g, c, d in s1.tolist() if g == s1[0, 0]}
    assert any((c, d) in first for g, c, d in s1.tolist() if g != s1[0, 0])      # the second meets the first's relabelling
    seen = dom != rr.NO_VOTE
    assert golden["edge_clipped"][1:][seen[1:]].any()               # a footprint clipped by the image edge, not the disc's
    assert (golden["labels_under"][seen] == 1).any() and (golden["labels_under"][seen] > 2).any()    # inside one label
    assert os.path.getsize(GOLDEN) < 512 * 1024


@pytest.mark.parametrize("none_camera", [None, 1])
def test_stage1_tables_against_sequential_relabelling(golden, none_camera):
    from opengaussian_amd import sam_refine
    model, cams, masks = sc.unpack_inputs(golden)
    model = model.cut(30)
    if none_camera is not None:
        masks[none_camera] = None
    res = rr.refine(cams, masks, model, sc.oracle_rasterize(model), sam_level=sc.SAM_LEVEL, stage1_stride=1,
                    current_max_id=7)
    assert sum(1 for p in res["stage1_pairs"] if p) >= 10
    seen = set()
    hit_relabelled = False
    for p in res["stage1_pairs"]:
        hit_relabelled |= any(cd in seen for cd in p)
        seen.update(p)
    assert hit_relabelled, "some pair must meet an id an earlier Gaussian already relabelled"
    level_ids = [None if m is None else torch.unique(m[sc.SAM_LEVEL]).tolist() for m in masks]
    tables, top = sam_refine.stage1_tables(level_ids, res["stage1_pairs"], current_max_id=7)
    assert top == res["current_max_id"]
    mapping, refined = sam_refine.remap_masks(masks, sc.SAM_LEVEL, tables)
    assert mapping == res["id_mapping"]
    for got, want in zip(refined, res["refined_masks"]):
        assert (got is None and want is None) or torch.equal(got, want)


def test_consistent_id_mapping_keeps_zero_and_void():
    from opengaussian_amd import sam_refine
    assert sam_refine.consistent_id_mapping([7, -1, 0, 3, 3, 12, -5]) == {3: 1, 7: 2, 12: 3, 0: 0, -1: -1}


def test_import_and_signature():
    from opengaussian_amd.sam_refine import MultiViewSAMMaskRefiner
    sig = inspect.signature(MultiViewSAMMaskRefiner.refine_sam_masks)
    names = list(sig.parameters)
    assert names[:5] == ["self", "cameras", "sam_masks", "gaussians", "sam_level"] and sig.parameters["sam_level"].default == 0
    defaults = {"stage1_stride": 1000, "stage1_opacity": 0.99, "stage2_stride": 1, "depth_diff_threshold": 0.15,
                "dist_optical_center": 0.1, "accumulated_weight_threshold": 0.5}
    for k, v in defaults.items():
        assert sig.parameters[k].default == v and sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    init = inspect.signature(MultiViewSAMMaskRefiner.__init__)
    assert list(init.parameters) == ["self", "verbose_logging"] and init.parameters["verbose_logging"].default is False
    r = MultiViewSAMMaskRefiner(verbose_logging=True)
    assert r.current_max_id == 0


def test_cpu_model_is_refused(golden):
    from opengaussian_amd.sam_refine import MultiViewSAMMaskRefiner
    model, cams, masks = sc.unpack_inputs(golden)
    with pytest.raises(RuntimeError, match="no CPU path"):
        MultiViewSAMMaskRefiner().refine_sam_masks(cams, masks, model.cut(4))
