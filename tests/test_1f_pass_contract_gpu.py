"""GPU: what code outside opengaussian_amd/rasterizer.py reads from the two autograd functions of a pass, pinned.

_RasterizeGaussians (activated inputs) and _RasterizeModel (raw parameters) run the same pass; tests, scripts and the
benchmark reach into their autograd nodes.  On rasterize_fused and rasterize_model, 6 extra channels, M = 4, on the tiny
(P = 8, 32 x 32) and the streaming path (the same scene with TINY_MAX_P = 0):

  * the saved_tensors layout: 13 tensors for a tiny pass, 18 for a streaming one, none for P = 0; [11] is the returned radii;
  * the attributes of the node and their values; the size of the hosted gradient record from the requires_grad flags;
  * what a call adds to PASS_STATS, forward and backward;
  * the two functions give the same four outputs, bit for bit;
  * the hosted record is handed over once on the raw path: two backwards over a retained graph, hosting on and off;
  * a camera leaf through the raw path; a 12-channel pass whose camera trains is rejected by both before any launch.
"""
import contextlib
import functools

import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

BG = (0.1, 0.2, 0.3)               # 3-wide: tiled over the 9 channels by both functions
M = 4                              # stored SH coefficients, active degree 1
KINDS = ("fused", "model")
PATHS = ("tiny", "streaming")
ATTRS = ("P", "Cn", "num_rendered", "tiny", "bwd_tmp", "bwd_clear_bytes", "full_binning", "num_groups", "geom_channels",
         "raster_settings", "pose_like")


@functools.lru_cache(maxsize=None)
def _scene(P, W, H):
    """(scene, camera, raw parameters) on the host, built once: log-scales, logits, quaternions of norm 0.5 .. 2"""
    sc, cam = helpers.tiny_scene(P, W, H, 30.0, seed=1500 + P)
    g = torch.Generator().manual_seed(P)
    op = sc.opacities.clamp(1e-4, 1 - 1e-4)
    raw = {"features_dc": sc.shs[:, :1].contiguous(), "features_rest": sc.shs[:, 1:M].contiguous(),
           "opacity": torch.log(op / (1 - op)), "scaling": torch.log(sc.scales),
           "rotation": sc.rotations * (0.5 + 1.5 * torch.rand(P, 1, generator=g))}
    return sc, cam, raw


@contextlib.contextmanager
def _path(path):
    from opengaussian_amd import rasterizer as R
    saved = R.TINY_MAX_P
    if path == "streaming":
        R.TINY_MAX_P = 0
    try:
        yield
    finally:
        R.TINY_MAX_P = saved


@contextlib.contextmanager
def _hosted(on):
    from opengaussian_amd import rasterizer as R
    saved, R.HOST_BWD_CLEAR = R.HOST_BWD_CLEAR, on
    try:
        yield
    finally:
        R.HOST_BWD_CLEAR = saved


def _forward(kind, dev, P=8, W=32, H=32, train="all", extra_channels=6, rs=None):
    """one pass through the facade -> (outputs, leaves).  train: "all", "extra" (the extra features alone) or "none".
    The activated inputs of the fused pass are activate_model's outputs of the raw parameters the model pass gets."""
    from opengaussian_amd import rasterizer as R
    sc, cam, raw = _scene(P, W, H)
    if rs is None:
        rs = helpers.settings_for(cam, BG, 1, dev)
    leaf = lambda t, on=(train == "all"): t.detach().clone().to(dev).requires_grad_(on)
    feat = torch.cat([sc.ins_feat, sc.ins_feat[:, :3]], 1)[:, :extra_channels].contiguous()
    L = dict(means3D=leaf(sc.means3D), means2D=leaf(torch.zeros(P, 3)), extra=leaf(feat, train != "none"))
    r = {k: v.to(dev) for k, v in raw.items()}
    order = ("features_dc", "features_rest", "opacity", "scaling", "rotation")
    if kind == "model":
        L.update({k: leaf(r[k]) for k in order})
        out = R.rasterize_model(L["means3D"], L["means2D"], *[L[k] for k in order], rs, extra_feats=L["extra"])
    else:
        scales, rots, opac, shs = R.activate_model(*[r[k] for k in order])
        L.update(opacities=leaf(opac), shs=leaf(shs), scales=leaf(scales), rotations=leaf(rots))
        out = R.rasterize_fused(L["means3D"], L["means2D"], L["opacities"], L["shs"], L["extra"], rs, scales=L["scales"],
                                rotations=L["rotations"])
    return out, L


def _upstream(out, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(out[i].shape, generator=g).to(dev) for i in (0, 2, 3)]


# ---- saved layout, attributes, PASS_STATS ----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", KINDS)
def test_saved_layout_attributes_and_pass_stats(gpu_device, kind, path):
    from opengaussian_amd import rasterizer as R
    dev = gpu_device
    tiny = path == "tiny"
    before = dict(R.PASS_STATS)
    with _path(path):
        out, L = _forward(kind, dev)
    color, radii, depth, alpha = out
    fn = color.grad_fn
    delta = {k: R.PASS_STATS[k] - before[k] for k in before}
    print(f"{kind} {path}: PASS_STATS delta {delta}, num_rendered {fn.num_rendered}, bwd_clear_bytes {fn.bwd_clear_bytes}")

    # PASS_STATS of the forward
    assert delta["tiny"] == (1 if tiny else 0)
    assert delta["raw_model"] == (1 if kind == "model" else 0)
    assert delta["blocking"] + delta["deferred"] == (0 if tiny else 1)
    assert delta["tiny_rerendered_for_backward"] == 0 and delta["reblend"] == 0

    # outputs: separate tensors, radii outside the graph
    assert color.shape == (9, 32, 32) and depth.shape == (1, 32, 32) and alpha.shape == (1, 32, 32) and radii.shape == (8,)
    assert len({t.untyped_storage().data_ptr() for t in (color, depth, alpha)}) == 3
    assert radii.dtype is torch.int32 and not radii.requires_grad
    assert int((radii > 0).sum()) > 0

    # saved layout
    saved = fn.saved_tensors
    assert len(saved) == (13 if tiny else 18)
    assert saved[11].dtype is torch.int32 and saved[11].data_ptr() == radii.data_ptr()
    assert saved[12].data_ptr() == alpha.data_ptr()
    assert saved[0].shape == (8, 3) and saved[7].numel() == 9                  # means3D first, the tiled background eighth
    for i in (8, 9):
        assert saved[i].numel() == 16
    assert saved[10].numel() == 3
    if not tiny:
        assert saved[13].dtype is torch.uint8 and saved[14].dtype is torch.uint8 and saved[15].dtype is torch.int32
        assert saved[16].dtype is torch.uint8 and saved[17].dtype is torch.uint8

    # attributes of the node
    for name in ATTRS:
        assert hasattr(fn, name), name
    assert fn.P == 8 and fn.Cn == 9 and fn.num_groups == 1 and fn.geom_channels == 3
    assert fn.tiny is tiny
    assert (fn.num_rendered == -1) if tiny else (fn.num_rendered > 0)
    assert fn.full_binning is bool(R.FULL_BINNING) and fn.pose_like is None
    assert fn.raster_settings.image_width == 32
    if kind == "model":
        assert fn.M == M and not hasattr(fn, "sh_rgb_sink")
    else:
        assert not hasattr(fn, "M") and fn.sh_rgb_sink is None
    assert (fn.bwd_tmp is not None) == ((not tiny) and R.HOST_BWD_CLEAR)
    assert fn.bwd_clear_bytes == (8 * 128 if fn.bwd_tmp is not None else 0)

    # backward: a tiny pass re-renders, once, and then knows its num_rendered
    before = dict(R.PASS_STATS)
    torch.autograd.backward([color, depth, alpha], _upstream(out, dev))
    assert R.PASS_STATS["tiny_rerendered_for_backward"] - before["tiny_rerendered_for_backward"] == (1 if tiny else 0)
    assert R.PASS_STATS["tiny"] == before["tiny"] and R.PASS_STATS["raw_model"] == before["raw_model"]
    assert fn.num_rendered >= 0 and fn.bwd_tmp is None
    for k, v in L.items():
        assert v.grad is not None and v.grad.shape == v.shape and torch.isfinite(v.grad).all(), k


@pytest.mark.parametrize("hosted", [True, False], ids=["hosted", "backward_fill"])
@pytest.mark.parametrize("kind", KINDS)
def test_hosted_record_size_follows_the_requires_grad_flags(gpu_device, kind, hosted):
    dev = gpu_device
    for train, stride in (("all", 128), ("extra", 64)):
        with _path("streaming"), _hosted(hosted):
            out, _ = _forward(kind, dev, train=train)
        fn = out[0].grad_fn
        assert (fn.bwd_tmp is not None) == hosted, train
        assert fn.bwd_clear_bytes == (8 * stride if hosted else 0), train
    with _path("tiny"), _hosted(hosted):
        out, _ = _forward(kind, dev, train="extra")
    assert out[0].grad_fn.bwd_tmp is None and out[0].grad_fn.bwd_clear_bytes == 0


@pytest.mark.parametrize("kind", KINDS)
def test_an_empty_scene_saves_nothing_and_gives_zero_images(gpu_device, kind):
    from opengaussian_amd import rasterizer as R
    before = dict(R.PASS_STATS)
    out, _ = _forward(kind, gpu_device, P=0)
    fn = out[0].grad_fn
    assert len(fn.saved_tensors) == 0 and fn.num_rendered == 0 and fn.P == 0 and fn.tiny is False and fn.bwd_tmp is None
    assert out[1].shape == (0,) and out[0].shape[1:] == (32, 32)
    for t in (out[0], out[2], out[3]):
        assert float(t.detach().abs().max()) == 0.0
    assert R.PASS_STATS == before                                      # nothing launched, nothing counted
    out[0].sum().backward()                                            # every gradient None: nothing to do


# ---- the two functions agree ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_model_and_fused_outputs_are_bit_identical(gpu_device, path):
    with _path(path), torch.no_grad():
        out_model, _ = _forward("model", gpu_device, train="none")
        out_fused, _ = _forward("fused", gpu_device, train="none")
    assert int((out_model[1] > 0).sum()) > 0
    for name, x, y in zip(("colour", "radii", "depth", "alpha"), out_model, out_fused):
        assert torch.equal(x, y), f"{name} differs between rasterize_model and rasterize_fused on the {path} path"


# ---- record hand-over on the raw path -------------------------------------------------------------------------------------
def _two_backwards(dev, hosted):
    with _hosted(hosted):
        out, L = _forward("model", dev, P=300, W=48, H=32)
        fn = out[0].grad_fn
        assert fn.tiny is False and (fn.bwd_tmp is not None) == hosted
        up = _upstream(out, dev, seed=3)
        res = []
        for i in range(2):
            for v in L.values():
                v.grad = None
            torch.autograd.backward([out[0], out[2], out[3]], up, retain_graph=i == 0)
            assert fn.bwd_tmp is None and fn.bwd_clear_bytes == 0           # used once: the second backward fills its own
            res.append({k: v.grad.clone() for k, v in L.items()})
    return res


def test_raw_path_hands_the_hosted_record_over_once(gpu_device):
    sets = _two_backwards(gpu_device, True) + _two_backwards(gpu_device, False)
    assert float(sets[0]["means3D"].abs().max()) > 0 and float(sets[0]["rotation"].abs().max()) > 0
    for i, other in enumerate(sets[1:], 1):
        for k, g in sets[0].items():
            assert torch.equal(g, other[k]), f"gradient set {i}: {k} differs from the first backward with the hosted clear"


# ---- camera leaf ----------------------------------------------------------------------------------------------------------
def test_camera_leaf_through_the_raw_path_and_forward_only_channels(gpu_device):
    from opengaussian_amd import rasterizer as R
    dev = gpu_device
    _, cam, _ = _scene(300, 48, 32)
    rs = helpers.settings_for(cam, BG, 1, dev)
    view = rs.viewmatrix.detach().clone().requires_grad_(True)
    rs = rs._replace(viewmatrix=view)
    out, L = _forward("model", dev, P=300, W=48, H=32, rs=rs)
    fn = out[0].grad_fn
    assert fn.tiny is False and fn.pose_like is not None and len(fn.pose_like) == 3
    assert fn.bwd_clear_bytes == (300 * 128 if R.HOST_BWD_CLEAR else 0)
    torch.autograd.backward([out[0], out[2], out[3]], _upstream(out, dev, seed=5))
    assert view.grad is not None and view.grad.shape == view.shape and view.grad.dtype is view.dtype
    assert torch.isfinite(view.grad).all() and float(view.grad.abs().max()) > 0
    assert L["means3D"].grad is not None
    # 12 channels have no backward: with nothing but the camera training, both functions say so before anything is launched
    before = dict(R.PASS_STATS)
    for kind in KINDS:
        with pytest.raises(RuntimeError, match="forward-only"):
            _forward(kind, dev, P=300, W=48, H=32, train="none", extra_channels=9, rs=rs)
    assert R.PASS_STATS == before
