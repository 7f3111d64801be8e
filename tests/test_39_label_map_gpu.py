"""GPU: the label map (ogs_raster_label_map, rasterizer.label_map, query.render_label_map) against the pass's own alpha, the
one-hot route through the drop-in rasterizer, and the NumPy restatement; the click route end to end."""
import types

import numpy as np
import pytest
import torch

from tests import label_map_cases as lc
from tests import helpers
from tests.test_label_map_host import _case_names, case_by_id

pytestmark = pytest.mark.gpu

_RUNS: dict = {}


def _cap():
    from opengaussian_amd import _lib
    return int(_lib.lib().ogs_label_map_tile_capacity())


def _fresh_pass(sc, cam, dev, force_streaming=True):
    """one 3-channel pass of the scene through the streaming path -> (outputs, the state it left in keep_sink or None)"""
    from opengaussian_amd import rasterizer as R
    s = sc.to(dev)
    sink: list = []
    out = R._RasterizeGaussians.apply(s.means3D, torch.zeros_like(s.means3D), None, s.means3D, s.opacities, s.scales,
                                      s.rotations, None, helpers.settings_for(cam, (0, 0, 0), 0, dev), 0, None, None, 1, sink,
                                      force_streaming)
    return out, (sink[0] if sink else None)


def _one_hot_route(sc, cam, labels, L, dev):
    """(label, weight, second) from 12-channel passes of the drop-in rasterizer over one-hot colours, zero background: the
    weights of the labels the scene uses, ascending, stacked; then the rule of the map"""
    from opengaussian_amd.rasterizer import GaussianRasterizer
    s = sc.to(dev)
    lab = labels.to(dev)
    used = torch.unique(lab[(lab >= 0) & (lab < L)])
    Hh, Ww = cam.image_height, cam.image_width
    none = (torch.full((Hh, Ww), -1, dtype=torch.int32, device=dev), torch.zeros(Hh, Ww, device=dev), torch.zeros(Hh, Ww, device=dev))
    K = used.numel()
    if K == 0:
        return none
    rast = GaussianRasterizer(helpers.settings_for(cam, (0.0,) * 12, 0, dev))
    planes = []
    for c0 in range(0, K, 12):
        chunk = used[c0:c0 + 12]
        onehot = torch.zeros(lab.numel(), 12, device=dev)
        onehot[:, :chunk.numel()] = (lab[:, None] == chunk[None, :]).to(torch.float32)
        color, _, _, _ = rast(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities,
                              colors_precomp=onehot, scales=s.scales, rotations=s.rotations)
        planes.append(color[:chunk.numel()])
    Wl = torch.cat(planes)                                               # [K, H, W]
    top = Wl.max(0).values
    idx = torch.arange(K, device=dev)[:, None, None]
    arg = torch.where(Wl == top[None], idx, torch.full_like(idx, K)).min(0).values          # first maximum: lowest label
    won = top > 0
    label = torch.where(won, used[arg].to(torch.int32), none[0])
    weight = torch.where(won, top, none[1])
    rest = torch.where(idx == arg[None], torch.full_like(Wl, -1.0), Wl)
    second = torch.where(won, rest.max(0).values.clamp_min(0.0), none[1])
    return label, weight, second


def _run(name, dev):
    """everything the tests below compare, once per case"""
    if name in _RUNS:
        return _RUNS[name]
    from opengaussian_amd import rasterizer as R
    cap = _cap()
    name, c = case_by_id(name, cap)
    (color, radii, depth, alpha), kept = _fresh_pass(c["sc"], c["cam"], dev)
    assert kept is not None
    labels = c["labels"].to(dev)
    fresh = R.label_map(kept, labels, c["L"])
    kp = R.KeptPasses(budget_bytes=1 << 30)
    assert kp.admit("slot", "key", None, kept)
    entry = kp.slots["slot"]
    compact = R.label_map(entry, labels, c["L"])
    torch.cuda.synchronize()
    r = dict(name=name, case=c, alpha=alpha[0], kept=kept, entry=entry, fresh=fresh, compact=compact, cap=cap)
    _RUNS[name] = r
    return r


@pytest.mark.parametrize("name", _case_names())
def test_alpha_is_the_pass_alpha_bit_for_bit(gpu_device, name):
    r = _run(name, gpu_device)
    for layout in ("fresh", "compact"):
        label, weight, second, alpha = r[layout]
        assert label.dtype == torch.int32 and alpha.shape == r["alpha"].shape
        assert torch.equal(alpha, r["alpha"]), (layout, float((alpha - r["alpha"]).abs().max()))
    for a, b in zip(r["fresh"], r["compact"]):
        assert torch.equal(a, b), "the compacted layout gives other maps than the one the pass left"


@pytest.mark.parametrize("name", _case_names())
def test_maps_equal_the_one_hot_route_bit_for_bit(gpu_device, name):
    r = _run(name, gpu_device)
    c = r["case"]
    label, weight, second = _one_hot_route(c["sc"], c["cam"], c["labels"], c["L"], gpu_device)
    got = r["fresh"]
    print(name, "label mismatches", int((got[0] != label).sum()), "weight max diff", float((got[1] - weight).abs().max()),
          "second max diff", float((got[2] - second).abs().max()))
    assert torch.equal(got[0], label)
    assert torch.equal(got[1], weight)
    assert torch.equal(got[2], second)
    # what the maps say about themselves
    assert bool(((got[0] >= 0) == (got[1] > 0)).all()) and bool((got[2] <= got[1]).all()) and bool((got[1] <= got[3]).all())


@pytest.mark.parametrize("name", _case_names())
def test_maps_against_the_restatement(gpu_device, name):
    r = _run(name, gpu_device)
    o = lc.oracle(r["name"], r["cap"])
    label, weight, second, alpha = (t.cpu().numpy() for t in r["fresh"])
    dec = o["decided"]
    figs = dict(label_mismatch_decided=int((label[dec] != o["label"][dec]).sum()), decided=int(dec.sum()),
                labelled=int((o["label"] >= 0).sum()), weight=float(np.abs(weight - o["weight"]).max()),
                second=float(np.abs(second - o["second"]).max()), alpha=float(np.abs(alpha - o["alpha"]).max()))
    print(name, figs)
    np.testing.assert_array_equal(label[dec], o["label"][dec])
    assert figs["weight"] <= lc.BAR and figs["second"] <= lc.BAR and figs["alpha"] <= lc.BAR, figs
    if r["name"].startswith("cap_"):
        n = len(r["case"]["labels"])
        # a tile with more labels than table rows was really walked more than once: labels of every sub-pass win somewhere
        wins = np.unique(label[label >= 0])
        ranks = np.searchsorted(o["used"], wins) // r["cap"]
        assert set(ranks.tolist()) == set(range((n + r["cap"] - 1) // r["cap"])), (n, sorted(set(ranks.tolist())))


def test_two_runs_give_identical_bytes(gpu_device):
    from opengaussian_amd import rasterizer as R
    r = _run("P1500_L700", gpu_device)
    c = r["case"]
    again = R.label_map(r["kept"], c["labels"].to(gpu_device), c["L"])
    for a, b in zip(r["fresh"], again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_label_dtypes_and_gpu_side_validation(gpu_device):
    from opengaussian_amd import rasterizer as R
    r = _run("P300_L5", gpu_device)
    c = r["case"]
    lab = c["labels"].to(gpu_device)
    as32 = torch.where((lab >= 0) & (lab < c["L"]), lab, torch.full_like(lab, -1)).to(torch.int32)
    for a, b in zip(r["fresh"], R.label_map(r["kept"], as32, c["L"])):
        assert torch.equal(a, b)
    # L = 0: every Gaussian is unlabelled
    label, weight, second, alpha = R.label_map(r["kept"], lab, 0)
    assert bool((label == -1).all()) and not bool(weight.any()) and not bool(second.any()) and torch.equal(alpha, r["alpha"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.label_map(r["kept"], lab.cpu(), c["L"])


# ---- render_label_map ------------------------------------------------------------------------------------------------------------
def _model_of(sc, dev):
    from tests.golden import render_cases as rc
    g = torch.Generator().manual_seed(5)
    P = sc.means3D.shape[0]
    op = sc.opacities.clamp(1e-4, 1 - 1e-4)
    params = {"_xyz": sc.means3D.clone(), "_features_dc": 0.5 * torch.randn(P, 1, 3, generator=g),
              "_features_rest": 0.1 * torch.randn(P, 15, 3, generator=g), "_scaling": torch.log(sc.scales),
              "_rotation": sc.rotations.clone(), "_opacity": torch.log(op / (1 - op)), "_ins_feat": torch.randn(P, 6, generator=g)}
    return rc.TinyModel(params, dev, requires_grad=False)


PIPE = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


@pytest.fixture()
def kept_cache():
    from opengaussian_amd import rasterizer as R
    saved = R.KEPT_PASSES
    R.KEPT_PASSES = R.KeptPasses(budget_bytes=1 << 30)
    yield R
    R.KEPT_PASSES = saved


def test_render_label_map_from_a_kept_pass_equals_the_fresh_one(gpu_device, kept_cache):
    from opengaussian_amd import query
    from opengaussian_amd.renderer import render
    R = kept_cache
    c = lc.scene_case(1500, 70)
    model, cam = _model_of(c["sc"], gpu_device), c["cam"].to(gpu_device)
    bg = torch.zeros(3, device=gpu_device)
    labels = c["labels"].to(gpu_device)
    with torch.no_grad():
        fresh = query.render_label_map(cam, model, PIPE, bg, 0, labels, c["L"])
        assert not R.KEPT_PASSES.slots and R.KEPT_PASSES.stats["admitted"] == 0, "the call admits nothing"
        out = render(cam, model, PIPE, bg, 0, rescale=False)
        assert R.KEPT_PASSES.stats["admitted"] == 1
        stats = dict(R.KEPT_PASSES.stats)
        entry = next(iter(R.KEPT_PASSES.slots.values()))
        hits = entry.hits
        kept = query.render_label_map(cam, model, PIPE, bg, 0, labels, c["L"])
        assert R.KEPT_PASSES.stats == stats and entry.hits == hits and len(R.KEPT_PASSES.slots) == 1
    assert isinstance(kept, query.LabelMap)
    for a, b in zip(fresh, kept):
        assert torch.equal(a, b)
    assert torch.equal(kept.alpha, out["alpha"][0]) and bool((kept.label >= 0).any())
    # the kept pass really was the source: the same maps straight from the entry
    for a, b in zip(kept, R.label_map(entry, labels, c["L"])):
        assert torch.equal(a, b)
    # pre_mask == labelling by hand; the masked-out points still occlude (alpha is the full scene's)
    pre = torch.rand(labels.numel(), generator=torch.Generator().manual_seed(3)) < 0.6
    by_hand = torch.where(pre.to(gpu_device), labels, torch.full_like(labels, -1))
    with torch.no_grad():
        masked = query.render_label_map(cam, model, PIPE, bg, 0, labels, c["L"], pre_mask=pre.to(gpu_device))
        hand = query.render_label_map(cam, model, PIPE, bg, 0, by_hand, c["L"])
    for a, b in zip(masked, hand):
        assert torch.equal(a, b)
    assert torch.equal(masked.alpha, kept.alpha) and not torch.equal(masked.label, kept.label)


def test_render_label_map_of_a_small_model_and_grad_inputs(gpu_device, kept_cache):
    from opengaussian_amd import query
    R = kept_cache
    cap = _cap()
    c = lc.capacity_case(cap - 1, 7)
    assert c["labels"].numel() <= R.TINY_MAX_P
    model, cam = _model_of(c["sc"], gpu_device), c["cam"].to(gpu_device)
    bg = torch.zeros(3, device=gpu_device)
    labels = c["labels"].to(gpu_device)
    # such a pass takes the tiny path and keeps nothing unless the streaming path is forced
    sc = c["sc"]
    tiny_before = R.PASS_STATS["tiny"]
    _, nothing = _fresh_pass(sc, c["cam"], gpu_device, force_streaming=False)
    assert nothing is None and R.PASS_STATS["tiny"] == tiny_before + 1
    with torch.no_grad():
        got = query.render_label_map(cam, model, PIPE, bg, 0, labels, c["L"])
    assert R.PASS_STATS["tiny"] == tiny_before + 1
    s = types.SimpleNamespace(means3D=model.get_xyz, opacities=model.get_opacity, scales=model.get_scaling,
                              rotations=model.get_rotation)
    s.to = lambda dev: s
    (_, _, _, alpha), kept = _fresh_pass(s, c["cam"], gpu_device)
    for a, b in zip(got, R.label_map(kept, labels, c["L"])):
        assert torch.equal(a, b)
    assert torch.equal(got.alpha, alpha[0]) and len(torch.unique(got.label)) > cap // 4
    # forward only
    model._xyz.requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward only"):
        query.render_label_map(cam, model, PIPE, bg, 0, labels, c["L"])
    with torch.no_grad():
        again = query.render_label_map(cam, model, PIPE, bg, 0, labels, c["L"])
    assert torch.equal(again.label, got.label)
    with pytest.raises(ValueError):
        query.render_label_map(cam, model, PIPE, bg, 0, labels[:-1], c["L"])


# ---- click -> leaf -> object ---------------------------------------------------------------------------------------------------------
def test_click_to_leaf_to_object(gpu_device):
    """a click on a planted blob gives the blob's leaf, and render_queries draws the same object from it as from the leaf id"""
    from opengaussian_amd import query
    from tests import query_cases as qc
    from tests.golden import render_cases as rc
    s = qc.query_scene()
    Ww, Hh, f = qc.SCENE["W"], qc.SCENE["H"], qc.SCENE["f"]
    g = torch.Generator().manual_seed(77)
    n, leaf_id, cx, cy, z = 200, 7, 30.0, 40.0, 1.5
    leaf = s["leaf"].clone()
    leaf[leaf == leaf_id] = 8
    rows = torch.randperm(leaf.numel(), generator=g)[:n]
    px = cx + (torch.rand(n, generator=g) - 0.5) * 8
    py = cy + (torch.rand(n, generator=g) - 0.5) * 8
    p = s["params"]
    p["_xyz"][rows] = torch.stack([(px + 0.5 - Ww / 2) * z / f, (py + 0.5 - Hh / 2) * z / f, torch.full((n,), z)], dim=1)
    p["_scaling"][rows] = torch.log(torch.tensor(0.02))
    p["_opacity"][rows] = 3.0
    leaf[rows] = leaf_id
    model = rc.TinyModel(p, gpu_device, requires_grad=False)
    cam, bg, leaf = s["cam"].to(gpu_device), s["bg"].to(gpu_device), leaf.to(gpu_device)
    with torch.no_grad():
        lm = query.render_label_map(cam, model, PIPE, bg, 0, leaf, 13)
        clicks = torch.tensor([[int(cx), int(cy)], [int(cx) + 1, int(cy) - 1]], device=gpu_device)
        for radius in (0, 2):
            ids = query.labels_at_pixels(lm, clicks, radius)
            assert ids.dtype == torch.int64 and ids.tolist() == [leaf_id, leaf_id], (radius, ids.tolist())
        kw = dict(root_num=4, leaf_num=3, post_process=False)
        by_click = query.render_queries(cam, model, PIPE, bg, 0, leaf, [ids[0:1]], **kw)
        by_id = query.render_queries(cam, model, PIPE, bg, 0, leaf, [torch.tensor([leaf_id], device=gpu_device)], **kw)
    assert by_click.kept == [True] and by_id.kept == [True] and by_click.counts == by_id.counts
    assert torch.equal(by_click.images[0], by_id.images[0]) and torch.equal(by_click.silhouettes[0], by_id.silhouettes[0])
    # the object's silhouette covers the click
    assert float(by_click.silhouettes[0][0, int(cy), int(cx)]) > 0.5
