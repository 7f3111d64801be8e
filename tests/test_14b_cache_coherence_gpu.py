"""GPU: every version-keyed cache against every raw-pointer writer of the library ("the version contract").

Four pieces of state decide "nothing changed" from ``(data_ptr, torch's _version)``: the key of ``rasterizer.KEPT_PASSES``, that key
plus the background tensor for ``rasterizer.KEPT_IMAGES``, ``rasterizer._tiled_bg`` and ``pose.CameraPose``.  torch moves the counter
for its own in-place ops; ``FusedAdam``, ``ShardedAdam``, the k-means centre updates and the densification statistics write through
``data_ptr()`` and move it with ``_lib.mark_written``.  Held here:

  A  the table of section 3b, row by row: what a call wrote moved, what it only read did not; FusedAdam moves what torch's Adam moves
  B  a kept pass goes stale when FusedAdam steps the parameter render() sees as a detached alias (hand-set grad, momentum alone)
  C  the same for a kept image; and for its background tensor
  D  the tiled background of a fused pass follows a stepped background
  E  CameraPose re-evaluates after its delta was stepped
  F  autograd's saved-tensor check fires after a FusedAdam step as after a torch.optim.Adam step
  G  a kept pass owns its radii: writing into what render() returned reaches neither later hits nor their gradients
  H  a 12-channel re-blend with features that require grad raises in its forward

Every image comparison is bit for bit against the same library with the caches switched off (that path is held to the float64
oracle by test_10 / test_12); the one tolerance is test_14's for the feature gradient of a re-blend."""
import types

import pytest
import torch
from torch import nn

from opengaussian_amd.synthetic import make_camera
from tests import helpers
from tests.test_14_kept_pass_gpu import ReferenceShapedGaussians, kept  # noqa: F401  (kept: the fixture)

pytestmark = pytest.mark.gpu

# just above the 1024-Gaussian tiny-pass limit: the streaming path runs, the only one that keeps a pass
P, W, H, F = 1100, 64, 48, 60.0
# the same scene through a wider lens: it fills the middle of the image, the border is background (the float64 oracle finds 957
# of the 3072 pixels untouched by any Gaussian, the four corners among them)
F_WIDE = 40.0
PIPE = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
RENDER_KEYS = ("render", "alpha", "depth", "silhouette", "ins_feat", "radii", "visibility_filter")
_SCENE = helpers.lazy(lambda: helpers.tiny_scene(P, W, H, F))


def _scene(dev, wide=False):
    sc, cam = _SCENE()
    return sc, (make_camera(W, H, F_WIDE, F_WIDE) if wide else cam).to(dev)


def _fused_adam(params, lr=0.05):
    from opengaussian_amd.optim import FusedAdam
    return FusedAdam([{"params": [p], "lr": lr} for p in params], lr=0.0, eps=1e-15)


def _versions(tensors):
    return {k: t._version for k, t in tensors.items()}


def _moved(tensors, before):
    return {k: t._version != before[k] for k, t in tensors.items()}


# ---- A: the table ---------------------------------------------------------------------------------------------------------------
def _case_sharded_adam(dev, R):
    from opengaussian_amd import dp
    opt = dp.ShardedAdam([("a", (5,)), ("b", (3, 2))], {"a": 0.05, "b": 0.01}, dev)
    opt.load({"a": torch.arange(5.0, device=dev), "b": torch.ones(3, 2, device=dev)})
    grad = torch.ones(5, device=dev)
    opt.params["a"].grad = grad                                     # "b" has no gradient: skipped, like torch's Adam
    written = {"my_param": opt.my_param, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}
    return written, {"grad": grad}, opt.step


def _case_sharded_adam_views(dev, R):
    """the parameter views move with `flat`, through torch's own copy (pinned: it held before the helper existed)"""
    _, read, step = _case_sharded_adam(dev, R)
    opt = step.__self__
    return {"params[a]": opt.params["a"], "params[a].detach()": opt.params["a"].detach(), "flat": opt.flat}, read, step


def _km(dev, k=3, d=6, N=64):
    g = torch.Generator().manual_seed(7)
    feat = torch.rand(N, d, generator=g).to(dev)
    return feat, feat[:k].clone(), torch.rand(N, generator=g).to(dev) + 0.5


def _case_kmeans_lloyd(dev, R):
    from opengaussian_amd import kmeans
    feat, centers, _ = _km(dev)
    return {"centers": centers}, {"feat": feat}, lambda: kmeans.lloyd(feat, centers, 2, nchunks=1)


def _case_kmeans_lloyd_sharded(dev, R):
    from opengaussian_amd import kmeans
    feat, centers, _ = _km(dev)
    return {"centers": centers}, {"feat": feat}, lambda: kmeans.lloyd_sharded(feat, centers, 2, nchunks=1)


def _case_kmeans_wide_update(dev, R):
    from opengaussian_amd import kmeans
    feat, centers, weights = _km(dev)
    ids = (torch.arange(feat.shape[0], device=dev) % 3).to(torch.int32)     # already what the kernel reads: no copy is made
    return {"centers": centers}, {"feat": feat, "ids": ids, "weights": weights}, \
        lambda: kmeans.wide_update(feat, ids, centers, "l2", weights)


def _case_kmeans_wide_lloyd(dev, R):
    from opengaussian_amd import kmeans
    feat, centers, weights = _km(dev)
    return {"centers": centers}, {"feat": feat, "weights": weights}, lambda: kmeans.wide_lloyd(feat, centers, 2, "l2", weights)


def _case_kmeans_assign(dev, R):
    """the read-only entry points: nothing the caller holds moves"""
    from opengaussian_amd import kmeans
    feat, centers, _ = _km(dev)

    def call():
        kmeans.assign(feat, centers)
        kmeans.wide_assign(feat, centers)
    return {}, {"feat": feat, "centers": centers}, call


def _densify_state(dev, N=8):
    from opengaussian_amd import densify
    g = torch.Generator().manual_seed(3)
    state = densify.DensifyState(None, torch.zeros(N, 1, device=dev), torch.zeros(N, 1, device=dev), torch.zeros(N, device=dev))
    grad = torch.randn(N, 3, generator=g).to(dev)
    radii = (torch.arange(N, dtype=torch.int32) % 3).to(dev)               # some zero (not visible), some not
    return densify, state, grad, radii


def _case_densify_stats_radii(dev, R):
    densify, state, grad, radii = _densify_state(dev)
    written = {"xyz_gradient_accum": state.xyz_gradient_accum, "denom": state.denom, "max_radii2D": state.max_radii2D}
    return written, {"viewspace_grad": grad, "radii": radii}, lambda: densify.add_densification_stats(state, grad, radii=radii)


def _case_densify_stats_filter(dev, R):
    """without `radii` the kernel leaves max_radii2D alone: it is not marked"""
    densify, state, grad, radii = _densify_state(dev)
    vis = (radii > 0).to(torch.uint8)
    written = {"xyz_gradient_accum": state.xyz_gradient_accum, "denom": state.denom}
    return written, {"viewspace_grad": grad, "update_filter": vis, "max_radii2D": state.max_radii2D}, \
        lambda: densify.add_densification_stats(state, grad, vis)


def _kept_entry(dev, R):
    sc, cam = _scene(dev)
    rs = helpers.settings_for(cam, (0.1, 0.2, 0.3), 3, dev)
    with torch.no_grad():
        R.rasterize_fused(sc.means3D.to(dev), torch.zeros(P, 3, device=dev), sc.opacities.to(dev), sc.shs.to(dev),
                          sc.ins_feat.to(dev), rs, scales=sc.scales.to(dev), rotations=sc.rotations.to(dev),
                          detach_extra_from_geometry=False, frozen_key=("table", ("v", 0), None))
    (entry,) = R.KEPT_PASSES.slots.values()
    return entry


def _case_label_votes_out(dev, R):
    entry = _kept_entry(dev, R)
    labels = (torch.arange(H * W, dtype=torch.int32, device=dev) % 4).reshape(H, W)
    rows = torch.arange(P, dtype=torch.int32, device=dev) % 5
    out = torch.zeros(5, 5, dtype=torch.int64, device=dev)
    return {"out": out}, {"pixel_labels": labels, "rows": rows}, lambda: R.label_votes(entry, labels, 4, rows=rows, num_rows=5, out=out)


def _case_feature_votes_out(dev, R):
    entry = _kept_entry(dev, R)
    feats = torch.rand(2, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
    rows = torch.arange(P, dtype=torch.int32, device=dev) % 5
    out = torch.zeros(5, 3, dtype=torch.int64, device=dev)
    return {"out": out}, {"features": feats, "rows": rows}, lambda: R.feature_votes(entry, feats, rows=rows, num_rows=5, out=out)


def _case_sh_rebuild_out(dev, R):
    from opengaussian_amd import dp
    ex = dp.ShGradExchange(8, 16, dev)
    g = torch.Generator().manual_seed(9)
    means, campos = torch.randn(8, 3, generator=g).to(dev), torch.zeros(1, 3, device=dev)
    ex.gather_async(torch.randn(8, 3, generator=g).to(dev))
    out = torch.zeros(8, 16, 3, device=dev)
    return {"out": out}, {"means3D": means, "campos_all": campos}, lambda: ex.rebuild(means, campos, 3, out=out)


TABLE = {f.__name__[len("_case_"):]: f for f in (
    _case_sharded_adam, _case_sharded_adam_views, _case_kmeans_lloyd, _case_kmeans_lloyd_sharded, _case_kmeans_wide_update,
    _case_kmeans_wide_lloyd, _case_kmeans_assign, _case_densify_stats_radii, _case_densify_stats_filter, _case_label_votes_out,
    _case_feature_votes_out, _case_sh_rebuild_out)}


@pytest.mark.parametrize("entry_point", sorted(TABLE))
def test_a_call_moves_the_version_of_what_it_wrote_and_of_nothing_else(kept, gpu_device, entry_point):
    written, read, call = TABLE[entry_point](gpu_device, kept)
    values = {k: t.clone() for k, t in written.items()}
    w0, r0 = _versions(written), _versions(read)
    call()
    print(entry_point, "written:", _moved(written, w0), "read:", _moved(read, r0))
    for k, t in written.items():
        assert not torch.equal(t, values[k]), f"{k}: the case must make the call write it"
    assert _moved(written, w0) == {k: True for k in written}
    assert _moved(read, r0) == {k: False for k in read}


def test_fused_adam_moves_the_versions_torch_adam_moves(gpu_device):
    """Three groups; the last one's parameter has no gradient: not stepped, nothing of it moves.  The moments exist after a first
    step of either optimizer; the second step is the one compared."""
    dev = gpu_device

    def moved_by(make):
        g = torch.Generator().manual_seed(11)
        ps = [nn.Parameter(torch.randn(5, generator=g).to(dev)) for _ in range(3)]
        opt = make(ps)
        grads = [torch.randn(5, generator=g).to(dev) for _ in range(2)]
        for p, gr in zip(ps, grads):
            p.grad = gr
        opt.step()
        tensors = {}
        for i, p in enumerate(ps):
            tensors[f"p{i}"], tensors[f"p{i}.detach()"] = p, p.detach()
            for k, t in opt.state[p].items():
                tensors[f"p{i}.{k}"] = t
        for i, gr in enumerate(grads):
            tensors[f"p{i}.grad"] = gr
        before = _versions(tensors)
        opt.step()
        assert len(opt.state[ps[2]]) == 0
        return _moved(tensors, before)

    adam = lambda **kw: (lambda ps: torch.optim.Adam([{"params": [p], "lr": 0.05} for p in ps], lr=0.0, eps=1e-15, **kw))
    # the reference is torch's single-tensor implementation, whose every update is an in-place op on the tensor itself.  The
    # foreach implementation (the default on a GPU) updates exp_avg with torch._foreach_lerp_, which on torch 2.10 leaves the
    # version counters alone although it writes (measured here: exp_avg False, everything else as below): FusedAdam must move
    # whatever that path moves as well, and is not excused from marking exp_avg by it
    want = moved_by(adam(foreach=False))
    default = moved_by(adam())
    got = moved_by(_fused_adam)
    print("torch.optim.Adam(foreach=False):", want)
    print("torch.optim.Adam():             ", default)
    print("FusedAdam:                      ", got)
    stepped = {f"p{i}{s}": True for i in range(2) for s in ("", ".detach()", ".step", ".exp_avg", ".exp_avg_sq")}
    assert want == {**stepped, "p0.grad": False, "p1.grad": False, "p2": False, "p2.detach()": False}      # what the test assumes of torch
    assert got == want
    assert all(got[k] for k, m in default.items() if m) and default.keys() == got.keys()


# ---- B, C: kept passes and kept images under the project's own optimizer --------------------------------------------------------
def _model_with_stepped(attr, dev, mode):
    """A stage >= 1 model: every geometry / appearance attribute detached; `attr` is the detached alias of a Parameter that a
    FusedAdam still holds (train.py replaces the attributes by `param.detach()`, the optimizer keeps the Parameters)."""
    sc, cam = _scene(dev)
    pc = ReferenceShapedGaussians(sc, dev)
    param = nn.Parameter(getattr(pc, attr).clone())
    setattr(pc, attr, param.detach())
    opt = _fused_adam([param])
    param.grad = torch.ones_like(param)
    if mode == "momentum_only":
        # zero_grad(set_to_none=False) after one real step: the gradient is all zero, Adam's momentum still moves the parameter
        opt.step()
        param.grad.zero_()
    return pc, cam, param, opt


def _assert_same(out, ref, keys):
    for k in keys:
        if ref[k] is None:
            assert out[k] is None, k
        else:
            assert torch.equal(out[k], ref[k]), k


@pytest.mark.parametrize("mode", ["hand_set_grad", "momentum_only"])
@pytest.mark.parametrize("attr", ["_xyz", "_opacity"])
def test_a_fused_adam_step_makes_the_kept_pass_stale(kept, gpu_device, attr, mode):
    from opengaussian_amd.renderer import render
    R, dev = kept, gpu_device
    pc, cam, param, opt = _model_with_stepped(attr, dev, mode)
    bg = torch.tensor([0.2, 0.1, 0.3], device=dev)
    call = lambda: render(cam, pc, PIPE, bg, iteration=40000, rescale=False)
    before = R.PASS_STATS["reblend"]
    call()
    assert R.KEPT_PASSES.stats["admitted"] == 1 and R.PASS_STATS["reblend"] == before
    out0 = call()
    assert R.PASS_STATS["reblend"] == before + 1 and R.KEPT_PASSES.stats["stale"] == 0
    old = getattr(pc, attr).clone()
    opt.step()
    assert not torch.equal(getattr(pc, attr), old)                    # the alias render() reads moved by value
    out1 = call()
    print(attr, mode, R.KEPT_PASSES.stats, "reblends", R.PASS_STATS["reblend"] - before)
    assert R.KEPT_PASSES.stats["stale"] == 1 and R.PASS_STATS["reblend"] == before + 1
    R.KEPT_PASSES, on = R.KeptPasses(budget_bytes=0), R.KEPT_PASSES
    ref = call()
    R.KEPT_PASSES = on
    _assert_same(out1, ref, RENDER_KEYS)
    assert not torch.equal(out1["render"], out0["render"])


@pytest.fixture()
def kept_images(kept):
    saved, kept.KEPT_IMAGES = kept.KEPT_IMAGES, kept.KeptImages(budget_bytes=1 << 30)
    yield kept
    kept.KEPT_IMAGES = saved


def _passes(R):
    return sum(R.PASS_STATS[k] for k in ("blocking", "deferred", "tiny", "reblend"))


@pytest.mark.parametrize("mode", ["hand_set_grad", "momentum_only"])
@pytest.mark.parametrize("attr", ["_xyz", "_opacity"])
def test_a_fused_adam_step_makes_the_kept_image_stale(kept_images, gpu_device, attr, mode):
    from opengaussian_amd.renderer import render
    R, dev = kept_images, gpu_device
    pc, cam, param, opt = _model_with_stepped(attr, dev, mode)
    bg = torch.tensor([0.2, 0.1, 0.3], device=dev)
    call = lambda: render(cam, pc, PIPE, bg, iteration=60000, rescale=False, render_feat_map=False)
    n0 = _passes(R)
    call()
    assert R.KEPT_IMAGES.stats["admitted"] == 1 and _passes(R) == n0 + 1
    out0 = call()
    assert R.KEPT_IMAGES.stats["hits"] == 1 and _passes(R) == n0 + 1          # no pass was launched
    old = getattr(pc, attr).clone()
    opt.step()
    assert not torch.equal(getattr(pc, attr), old)
    out1 = call()
    print(attr, mode, R.KEPT_IMAGES.stats, "passes", _passes(R) - n0)
    assert R.KEPT_IMAGES.stats["stale"] == 1 and R.KEPT_IMAGES.stats["hits"] == 1 and _passes(R) == n0 + 2
    R.KEPT_IMAGES, on = R.KeptImages(budget_bytes=0), R.KEPT_IMAGES
    ref = call()
    R.KEPT_IMAGES = on
    _assert_same(out1, ref, RENDER_KEYS)
    assert not torch.equal(out1["render"], out0["render"])


def test_a_fused_adam_step_of_the_background_makes_the_kept_image_stale(kept_images, gpu_device):
    from opengaussian_amd.renderer import render
    R, dev = kept_images, gpu_device
    sc, cam = _scene(dev, wide=True)
    pc = ReferenceShapedGaussians(sc, dev)
    bg = nn.Parameter(torch.tensor([0.2, 0.1, 0.3], device=dev))
    opt = _fused_adam([bg])
    bg.grad = torch.ones_like(bg)
    call = lambda: render(cam, pc, PIPE, bg.detach(), iteration=60000, rescale=False, render_feat_map=False)
    n0 = _passes(R)
    out0 = call()
    call()
    assert R.KEPT_IMAGES.stats["hits"] == 1 and _passes(R) == n0 + 1
    empty = out0["alpha"][0] == 0                                      # pixels no Gaussian reaches
    assert bool(empty[0, 0]) and int(empty.sum()) > 100
    assert torch.equal(out0["render"][:, empty], bg.detach()[:, None].expand(3, int(empty.sum())))
    old = bg.detach().clone()
    opt.step()
    new = bg.detach().clone()
    assert not torch.equal(new, old)
    out1 = call()
    print(R.KEPT_IMAGES.stats, "passes", _passes(R) - n0, "bg", old.tolist(), "->", new.tolist())
    assert R.KEPT_IMAGES.stats["stale"] == 1 and _passes(R) == n0 + 2          # a real pass
    assert torch.equal(out1["alpha"], out0["alpha"])
    assert torch.equal(out1["render"][:, empty], new[:, None].expand(3, int(empty.sum())))


# ---- D: the tiled background ----------------------------------------------------------------------------------------------------
def test_the_tiled_background_follows_a_fused_adam_step(gpu_device):
    from opengaussian_amd import rasterizer as R
    dev = gpu_device
    sc, cam = _scene(dev, wide=True)
    bg = nn.Parameter(torch.tensor([0.2, 0.1, 0.3], device=dev))
    opt = _fused_adam([bg])
    bg.grad = torch.ones_like(bg)
    alias = bg.detach()
    args = (sc.means3D.to(dev), torch.zeros(P, 3, device=dev), sc.opacities.to(dev), sc.shs.to(dev), sc.ins_feat.to(dev))

    def call():
        rs = helpers.settings_for(cam, alias, 3, dev)
        assert rs.bg.data_ptr() == alias.data_ptr() and rs.bg.shape == (3,)     # the pass is handed the 3-wide tensor itself
        with torch.no_grad():
            return R.rasterize_fused(*args, rs, scales=sc.scales.to(dev), rotations=sc.rotations.to(dev),
                                     detach_extra_from_geometry=False)

    color0, _, _, alpha0 = call()
    assert color0.shape == (9, H, W)
    empty = alpha0[0] == 0
    n = int(empty.sum())
    assert bool(empty[0, 0]) and n > 100
    old = alias.clone()
    assert torch.equal(color0[:, empty], old.repeat(3)[:, None].expand(9, n))
    opt.step()
    new = alias.clone()
    assert not torch.equal(new, old)
    color1, _, _, alpha1 = call()
    print("bg", old.tolist(), "->", new.tolist(), "corner pixel", color1[:, 0, 0].tolist())
    assert torch.equal(alpha1, alpha0)
    assert torch.equal(color1[:, empty], new.repeat(3)[:, None].expand(9, n))


# ---- E: a camera pose stepped between two reads ---------------------------------------------------------------------------------
def test_camera_pose_reevaluates_after_a_fused_adam_step(gpu_device):
    from opengaussian_amd.pose import CameraPose
    dev = gpu_device
    _, base = _scene(dev)
    pose = CameraPose(base)
    opt = _fused_adam(list(pose.parameters()), lr=0.01)
    view0 = pose.world_view_transform.detach().clone()                # one evaluation serves each of the three tensors once
    pose.delta.grad = torch.tensor([1.0, -1.0, 1.0, -1.0, 1.0, -1.0], device=dev)
    opt.step()
    assert float(pose.delta.detach().abs().min()) > 0
    full, centre = pose.full_proj_transform, pose.camera_center
    fresh = CameraPose(base, delta=pose.delta)
    assert torch.equal(fresh.delta.detach(), pose.delta.detach())
    assert torch.equal(full, fresh.full_proj_transform) and torch.equal(centre, fresh.camera_center)
    assert torch.equal(pose.world_view_transform, fresh.world_view_transform)
    assert not torch.equal(pose.world_view_transform.detach(), view0)


# ---- F: autograd's saved-tensor check -------------------------------------------------------------------------------------------
def test_backward_through_a_stepped_saved_tensor_raises_as_with_torch_adam(gpu_device):
    dev = gpu_device

    def run(make):
        p = nn.Parameter(torch.arange(1.0, 6.0, device=dev))
        opt = make([p])
        y = (p * p).sum()                                             # saves p
        p.grad = torch.ones_like(p)
        opt.step()
        with pytest.raises(Exception) as err:
            y.backward()
        return err

    want = run(lambda ps: torch.optim.Adam(ps, lr=0.05, eps=1e-15))
    got = run(_fused_adam)
    print("torch.optim.Adam:", want.type.__name__, "| FusedAdam:", got.type.__name__)
    assert got.type is want.type is RuntimeError
    assert "modified by an inplace operation" in str(want.value) and "modified by an inplace operation" in str(got.value)


# ---- G: the kept radii ----------------------------------------------------------------------------------------------------------
def test_a_kept_pass_owns_its_radii(kept, gpu_device):
    from opengaussian_amd.renderer import render
    R, dev = kept, gpu_device
    sc, cam = _scene(dev)
    pc = ReferenceShapedGaussians(sc, dev)
    bg = torch.tensor([0.2, 0.1, 0.3], device=dev)
    gF = torch.randn(6, H, W, generator=torch.Generator().manual_seed(4)).to(dev)

    def step():
        out = render(cam, pc, PIPE, bg, iteration=40000, rescale=False)
        pc._ins_feat.grad = None
        (out["ins_feat"] * gF).sum().backward()
        return out, pc._ins_feat.grad.clone()

    before = R.PASS_STATS["reblend"]
    admitting, _ = step()
    hit1, _ = step()
    assert R.KEPT_PASSES.stats["admitted"] == 1 and R.PASS_STATS["reblend"] == before + 1
    assert int((hit1["radii"] > 0).sum()) > P // 2
    hit1["radii"].zero_()                                             # a caller that writes into what it was given ...
    admitting["radii"].zero_()                                        # ... also into what the admitting call returned
    hit2, g2 = step()
    hit3, _ = step()
    assert R.PASS_STATS["reblend"] == before + 3
    R.KEPT_PASSES, on = R.KeptPasses(budget_bytes=0), R.KEPT_PASSES
    ref, gref = step()
    R.KEPT_PASSES = on
    assert R.PASS_STATS["reblend"] == before + 3
    print("radii > 0:", int((hit2["radii"] > 0).sum()), "cache off:", int((ref["radii"] > 0).sum()),
          "max |grad - grad off|:", float((g2 - gref).abs().max()), "of", float(gref.abs().max()))
    assert torch.equal(hit2["radii"], ref["radii"]) and torch.equal(hit2["visibility_filter"], ref["visibility_filter"])
    assert float(gref.abs().max()) > 0
    torch.testing.assert_close(g2, gref, rtol=1e-6, atol=1e-9)        # test_14's bar for a re-blend's feature gradient
    assert hit2["radii"].data_ptr() != hit3["radii"].data_ptr()       # both alive: two tensors, not two aliases of the entry's
    assert torch.equal(hit3["radii"], ref["radii"])


# ---- H: the channel check of a re-blend -----------------------------------------------------------------------------------------
def test_a_twelve_channel_reblend_with_grad_raises_in_its_forward(kept, gpu_device):
    R, dev = kept, gpu_device
    sc, cam = _scene(dev)
    rs = helpers.settings_for(cam, (0.1, 0.2, 0.3), 3, dev)
    feats = torch.rand(P, 9, generator=torch.Generator().manual_seed(6)).to(dev)
    key = ("cam0", ("v", 0), None)

    def call(f):
        return R.rasterize_fused(sc.means3D.to(dev), torch.zeros(P, 3, device=dev), sc.opacities.to(dev), sc.shs.to(dev), f, rs,
                                 scales=sc.scales.to(dev), rotations=sc.rotations.to(dev), detach_extra_from_geometry=False,
                                 frozen_key=key)

    with torch.no_grad():
        color = call(feats)[0]
    assert color.shape == (12, H, W) and R.KEPT_PASSES.stats["admitted"] == 1
    before = R.PASS_STATS["reblend"]
    with pytest.raises(RuntimeError, match="forward-only"):
        call(feats.clone().requires_grad_())
    assert R.KEPT_PASSES.stats["hits"] == 1 and R.PASS_STATS["reblend"] == before       # the kept pass was found; nothing was launched
    with torch.no_grad():
        again = call(feats)[0]                                        # without grad the 12-channel re-blend still serves
    assert R.PASS_STATS["reblend"] == before + 1 and torch.equal(again, color)
