"""GPU: the rasterizer against the CPU oracle under GENERAL camera poses.

Every other oracle-parity test renders through the identity camera with fx == fy, under which most of what the kernels do
with the camera is multiplied by zero or one: the view matrix' rotation block and translation, the off-diagonal entries of
the projection matrix, the camera centre of the SH view direction, the distinction between focal_x and focal_y, and (the
scenes stop short of it) the +-1.3 x tanfov clamp of tx/tz, ty/tz with the gradient it zeroes.  Here the camera is rotated
(quarter turns and half turns as signed permutation matrices, exact in fp32; two general axis-angle rotations that leave
no matrix entry at zero or one), translated by the size of the scene, fx != fy, and the image is 150 x 90 (no multiple of
16).  helpers.posed_scene draws the scene in the camera frame and moves it to the world frame, so the posed camera sees
what the identity camera saw.

What entitles these tests to trust the oracle under such a camera is in tests/test_oracle_raster.py (test_posed_*).
Bars: the suite's -- radii, sorted keys, point lists and tile ranges bit-exact, images IMG_TOL modulo the documented
threshold flips, every gradient family GRAD_TOL of the family maximum against float64 autograd plus the per-row ruler."""
import types

import numpy as np
import pytest
import torch

from tests import helpers
from tests.test_10_raster_gpu import GRAD_TOL, IMG_TOL, _grad_check

pytestmark = pytest.mark.gpu

W, H, FX, FY = 150, 90, 120.0, 85.0
TANX, TANY = helpers.tanfovs(W, H, FX, FY)
POSE_NAMES = list(helpers.POSES)
# P on each geometry path: tiny_geometry_kernel (<= 256, tiny=True), small_geometry_kernel (257 .. 1024), preprocess_kernel
SIZES = [(200, True), (900, False), (1500, False)]
MODES = ["sh3", "sh0_cov", "rgb3_modifier", "feat6_cov"]


def _mode_of(pose, P):
    """colour / covariance input mode of a (pose, size) case: every mode meets every geometry path and every kind of pose"""
    return MODES[(POSE_NAMES.index(pose) + [s[0] for s in SIZES].index(P)) % len(MODES)]


def _inputs(sc, cam, mode):
    """(oracle inputs, sh_degree, background, scale_modifier)"""
    if mode == "sh3":
        return helpers.oracle_inputs(sc, cam, use_sh=True), 3, (0.1, 0.2, 0.3), 1.0
    if mode == "sh0_cov":
        return helpers.oracle_inputs(sc, cam, use_sh=True, use_cov=True), 0, (0.3, 0.0, 0.2), 1.0
    if mode == "rgb3_modifier":
        return helpers.oracle_inputs(sc, cam, use_sh=False), 3, (0.0, 0.4, 0.1), 0.7
    assert mode == "feat6_cov"
    return helpers.oracle_inputs(sc, cam, use_cov=True, feat=sc.ins_feat), 3, (0.0,) * 6, 1.0


def _oracle_forward(inp, sh_degree, bg, scale_modifier=1.0):
    from oracle import raster_oracle as ro
    return ro.render_forward(W=W, H=H, tanfovx=TANX, tanfovy=TANY, bg=np.array(bg, np.float32), sh_degree=sh_degree,
                             scale_modifier=scale_modifier, **inp)


def _assert_images(color, depth, alpha, ref, tag):
    n = lambda t: t.detach().cpu().numpy()
    try:
        helpers.assert_close_modulo_threshold_flips(n(color), ref["color"], IMG_TOL)
        helpers.assert_close_modulo_threshold_flips(n(alpha), ref["alpha"], IMG_TOL)
        helpers.assert_close_modulo_threshold_flips(n(depth), ref["depth"], IMG_TOL * 10, flip_tol=4e-2)
    except AssertionError as e:
        raise AssertionError(f"{tag}: {e}") from None


def _forward_check(inp, cam, sh_degree, bg, scale_modifier, dev, tiny, tag):
    """integers bit-exact (the tiny pass keeps no binning state: radii only), images at the bars of
    test_10::test_random_configurations_forward_parity"""
    ref = _oracle_forward(inp, sh_degree, bg, scale_modifier)
    assert (ref["geom"].radii > 0).sum() > 0.5 * len(ref["geom"].radii), f"{tag}: the posed camera does not see the scene"
    (color, radii, depth, alpha), _ = helpers.hip_forward(inp, cam, bg, sh_degree, dev, requires_grad=True, tiny=tiny,
                                                          scale_modifier=scale_modifier)
    assert bool(color.grad_fn.tiny) == tiny, tag
    np.testing.assert_array_equal(radii.cpu().numpy(), ref["geom"].radii, err_msg=tag)
    if not tiny:
        keys, ranges, _ncontrib, plist = helpers.hip_export_binning(color)
        np.testing.assert_array_equal(keys, ref["binning"].keys_sorted, err_msg=tag)
        np.testing.assert_array_equal(plist, ref["binning"].point_list, err_msg=tag)
        np.testing.assert_array_equal(ranges, ref["binning"].ranges, err_msg=tag)
    _assert_images(color, depth, alpha, ref, tag)
    return ref


@pytest.mark.parametrize("P,tiny", SIZES)
@pytest.mark.parametrize("pose", POSE_NAMES)
def test_posed_forward_parity(gpu_device, pose, P, tiny):
    R, t = helpers.POSES[pose]
    mode = _mode_of(pose, P)
    sc, cam = helpers.posed_scene(P, W, H, FX, FY, R, t, seed=100 + P)
    inp, sh_degree, bg, mod = _inputs(sc, cam, mode)
    _forward_check(inp, cam, sh_degree, bg, mod, gpu_device, tiny, f"{pose} P={P} {mode}")


@pytest.mark.parametrize("P,tiny", SIZES)
@pytest.mark.parametrize("pose", POSE_NAMES)
def test_posed_backward_parity(gpu_device, pose, P, tiny):
    """every gradient family, means2D included, against float64 autograd through the oracle: GRAD_TOL of the family maximum and
    the per-row ruler.  dL/dscales is left out under scale_modifier != 1 (the reference's scale gradient omits the modifier
    factor, Appendix A.5(v)); rotations carry the geometry there."""
    R, t = helpers.POSES[pose]
    mode = _mode_of(pose, P)
    sc, cam = helpers.posed_scene(P, W, H, FX, FY, R, t, seed=200 + P)
    inp, sh_degree, bg, mod = _inputs(sc, cam, mode)
    errs = _grad_check(inp, cam, W, H, FX, gpu_device, sh_degree=sh_degree, bg=bg, seed=P, fy=FY, scale_modifier=mod, tiny=tiny,
                       row_ruler=True, skip=("scales",) if mod != 1.0 else ())
    print(f"posed backward {pose} P={P} {mode}:", {k: f"{e:.1e}" for k, e in errs.items()})
    want = {"means3D", "opacities", "means2D"} | ({"cov3D_precomp"} if "cov" in mode else {"rotations"}) | \
           ({"shs"} if mode.startswith("sh") else {"colors_precomp"})
    assert want <= set(errs), (sorted(want), sorted(errs))
    for k, e in errs.items():
        assert e < GRAD_TOL, f"{pose} P={P} {mode}: {k}: relative error {e} (all: {errs})"


@pytest.mark.parametrize("pose,mode", [("general", "sh3"), ("quarter_y", "feat6_cov"), ("general_b", "rgb3_modifier")])
def test_posed_clamped_gaussians_forward_and_backward(gpu_device, pose, mode):
    """A tenth of the centres at (1.35 .. 1.75) x tanfov in x, in y and in both, both signs, with footprints that reach the image:
    the +-1.3 x tanfov clamp of tx/tz, ty/tz is active on Gaussians that are blended, and x_grad_mul / y_grad_mul zero their
    dtx / dty.  Their gradients are a few per cent of the family maximum (dL/dcov3D: below one per cent), so the clamped rows are
    also held to GRAD_TOL of THEIR OWN maximum, per family."""
    R, t = helpers.POSES[pose]
    P = 1500
    sc, cam = helpers.posed_scene(P, W, H, FX, FY, R, t, seed=31, beyond_clamp=0.1)
    inp, sh_degree, bg, mod = _inputs(sc, cam, mode)
    ref = _forward_check(inp, cam, sh_degree, bg, mod, gpu_device, False, f"clamp {pose} {mode}")
    # which rows are clamped AND blended, from the oracle alone (float64 view space: the centres are >= 0.05 x tanfov from the limit)
    Xc = inp["means3D"].astype(np.float64) @ np.asarray(R).T + np.asarray(t)[None]
    cx, cy = np.abs(Xc[:, 0] / Xc[:, 2]) > 1.3 * TANX, np.abs(Xc[:, 1] / Xc[:, 2]) > 1.3 * TANY
    listed = np.zeros(P, bool)
    listed[ref["binning"].point_list] = True
    seen = (ref["geom"].radii > 0) & (ref["geom"].tiles_touched > 0) & listed
    kinds = {"x": cx & ~cy & seen, "y": cy & ~cx & seen, "xy": cx & cy & seen}
    rows = np.nonzero((cx | cy) & seen)[0]
    tiles = int(ref["geom"].tiles_touched[rows].sum())
    print(f"clamp {pose} {mode}: {len(rows)} clamped visible Gaussians touch {tiles} tiles", {k: int(v.sum()) for k, v in kinds.items()})
    assert len(rows) >= 20 and all(int(v.sum()) >= 3 for v in kinds.values())
    errs = _grad_check(inp, cam, W, H, FX, gpu_device, sh_degree=sh_degree, bg=bg, seed=3, fy=FY, scale_modifier=mod,
                       row_ruler=True, skip=("scales",) if mod != 1.0 else (), rows={"clamped": rows})
    print(f"clamp {pose} {mode}:", {k: f"{e:.1e}" for k, e in errs.items()})
    assert "means3D[clamped]" in errs
    for k, e in errs.items():
        assert e < GRAD_TOL, f"clamp {pose} {mode}: {k}: relative error {e} (all: {errs})"


@pytest.mark.parametrize("pose", POSE_NAMES)
def test_posed_mark_visible(gpu_device, pose):
    """markVisible == the oracle's near-plane test pvz > 0.2 (Appendix A.1 step 1: fp32, left to right, no contraction), with
    centres within a few ulps of the plane on both sides, bit for bit; and == the float64 sign away from the plane."""
    from opengaussian_amd.rasterizer import GaussianRasterizer
    R, t = helpers.POSES[pose]
    sc, cam = helpers.posed_scene(4000, W, H, FX, FY, R, t, seed=5)
    g = torch.Generator().manual_seed(17)
    Xc = sc.means3D.double() @ torch.tensor(R).t() + torch.tensor(t, dtype=torch.float64)[None]
    Xc[:2000, 2] = 0.2 + (torch.rand(2000, generator=g, dtype=torch.float64) * 2 - 1) * 2e-6        # a few ulps of the terms
    Xc[2000:3000, 2] = 0.2 + (torch.rand(1000, generator=g, dtype=torch.float64) * 2 - 1) * 1e-2
    Xw = ((Xc - torch.tensor(t, dtype=torch.float64)[None]) @ torch.tensor(R)).float()
    F = np.float32
    V = cam.world_view_transform.numpy().astype(F).reshape(16)
    x, y, z = (Xw.numpy()[:, i] for i in range(3))
    pvz = V[2] * x + V[6] * y + V[10] * z + V[14]
    want = pvz > F(0.2)
    assert 500 < int(want[:2000].sum()) < 1500, "the probe rows do not straddle the near plane"
    got = GaussianRasterizer(helpers.settings_for(cam, (0, 0, 0), 3, gpu_device)).markVisible(Xw.to(gpu_device)).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    pvz64 = (Xw.double().numpy() @ np.asarray(R).T + np.asarray(t)[None])[:, 2]
    far = np.abs(pvz64 - 0.2) > 1e-5
    assert far.sum() > 1900
    np.testing.assert_array_equal(got[far], pvz64[far] > 0.2)


def test_posed_fused_pass(gpu_device):
    """rasterize_fused (RGB from SH + 6 feature channels, one pass) under a general pose: images and every gradient against the
    oracle's two passes (RGB with every family; features with gradient to the features only -- the default
    detach_extra_from_geometry, as in test_12)."""
    from oracle import raster_oracle as ro
    from opengaussian_amd.rasterizer import rasterize_fused
    dev = gpu_device
    R, t = helpers.POSES["general"]
    P = 1500
    sc, cam = helpers.posed_scene(P, W, H, FX, FY, R, t, seed=41)
    bg = (0.1, 0.2, 0.3)
    inpA = helpers.oracle_inputs(sc, cam, use_sh=True)
    inpB = helpers.oracle_inputs(sc, cam, feat=sc.ins_feat)
    refA, refB = _oracle_forward(inpA, 3, bg), _oracle_forward(inpB, 3, bg * 2)
    leaves = {k: getattr(sc, k).to(dev).clone().requires_grad_(True)
              for k in ("means3D", "scales", "rotations", "opacities", "shs", "ins_feat")}
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    color, radii, depth, alpha = rasterize_fused(leaves["means3D"], m2, leaves["opacities"], leaves["shs"], leaves["ins_feat"],
                                                 helpers.settings_for(cam, bg, 3, dev), scales=leaves["scales"],
                                                 rotations=leaves["rotations"])
    assert color.shape == (9, H, W)
    np.testing.assert_array_equal(radii.cpu().numpy(), refA["geom"].radii)
    keys, ranges, _n, plist = helpers.hip_export_binning(color)
    np.testing.assert_array_equal(keys, refA["binning"].keys_sorted)
    np.testing.assert_array_equal(plist, refA["binning"].point_list)
    np.testing.assert_array_equal(ranges, refA["binning"].ranges)
    _assert_images(color[:3], depth, alpha, refA, "fused RGB")
    _assert_images(color[3:], depth, alpha, refB, "fused features")
    rng = np.random.default_rng(9)
    gC, gD, gA = rng.standard_normal((9, H, W)), rng.standard_normal((1, H, W)), rng.standard_normal((1, H, W))
    td = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    torch.autograd.backward([color, depth, alpha], [td(gC), td(gD), td(gA)])
    zero1 = np.zeros((1, H, W))
    backA = lambda **kw: ro.render_backward_f64(inpA, refA["binning"], W, H, TANX, TANY, np.array(bg, np.float64), gC[:3], gD, gA,
                                                sh_degree=3, **kw)
    backB = lambda **kw: ro.render_backward_f64(inpB, refB["binning"], W, H, TANX, TANY, np.array(bg * 2, np.float64), gC[3:],
                                                zero1, zero1, sh_degree=3, **kw)
    names = ("means3D", "scales", "rotations", "opacities", "shs", "means2D")
    both = lambda **kw: {**{k: v for k, v in backA(**kw).items() if k in names}, "ins_feat": backB(**kw)["colors_precomp"]}
    want, want32 = both(), helpers.lazy(lambda: both(dtype=torch.float32))
    got = {k: v.grad for k, v in leaves.items()} | {"means2D": m2.grad}
    errs = {}
    for k, w in want.items():
        gk = got[k].cpu().double().numpy().reshape(w.shape)
        w32 = lambda k=k, shape=w.shape: want32()[k].reshape(shape)
        errs[k] = helpers.assert_grads_close_modulo_threshold_flips(gk, w, GRAD_TOL, want_fp32=w32, what=f"fused {k}")
        helpers.assert_grad_family_close_modulo_threshold_flips(gk, w, GRAD_TOL, w32, what=f"fused {k}")
    print("posed fused:", {k: f"{e:.1e}" for k, e in errs.items()})
    assert all(e < GRAD_TOL for e in errs.values()), errs


def test_posed_grouped_pass(gpu_device):
    """rasterize_groups under a general pose: each group's images against the ORACLE's render of that subset (SH colours: the
    camera centre enters), radii against the oracle's."""
    from opengaussian_amd.rasterizer import rasterize_groups
    dev = gpu_device
    R, t = helpers.POSES["general_b"]
    P, G = 1800, 3
    sc, cam = helpers.posed_scene(P, W, H, FX, FY, R, t, seed=51)
    bg = (0.2, 0.1, 0.3)
    ids = torch.randint(-1, G, (P,), generator=torch.Generator().manual_seed(3))
    d = lambda a: a.to(dev)
    with torch.no_grad():
        color, radii, depth, alpha = rasterize_groups(d(sc.means3D), torch.zeros(P, 3, device=dev), d(sc.opacities), d(ids), G,
                                                      helpers.settings_for(cam, bg, 3, dev), shs=d(sc.shs), scales=d(sc.scales),
                                                      rotations=d(sc.rotations))
    assert color.shape == (G, 3, H, W)
    assert int((radii.cpu()[ids < 0] != 0).sum()) == 0
    inp = helpers.oracle_inputs(sc, cam, use_sh=True)
    for gi in range(G):
        mask = (ids == gi).numpy()
        sub = {k: (v[mask] if k in ("means3D", "opacities", "scales", "rotations", "shs") else v) for k, v in inp.items()}
        ref = _oracle_forward(sub, 3, bg)
        assert (ref["geom"].radii > 0).sum() > 200
        np.testing.assert_array_equal(radii.cpu().numpy()[mask], ref["geom"].radii, err_msg=f"group {gi}")
        _assert_images(color[gi], depth[gi], alpha[gi], ref, f"group {gi}")


def test_posed_kept_pass_is_bit_identical_to_a_full_pass(gpu_device):
    """test_14's bit-identity of the frozen-geometry re-blend, under a general pose"""
    from opengaussian_amd import rasterizer as Rz
    dev = gpu_device
    R, t = helpers.POSES["general"]
    P = 3000
    sc, cam = helpers.posed_scene(P, W, H, FX, FY, R, t, seed=61)
    sc, cam = sc.to(dev), cam.to(dev)
    m2 = torch.zeros(P, 3, device=dev)

    def fused(feats, key, bg):
        return Rz.rasterize_fused(sc.means3D, m2, sc.opacities, sc.shs, feats, helpers.settings_for(cam, bg, 3, dev),
                                  scales=sc.scales, rotations=sc.rotations, detach_extra_from_geometry=False, frozen_key=key)

    saved, Rz.KEPT_PASSES = Rz.KEPT_PASSES, Rz.KeptPasses(budget_bytes=1 << 30)
    try:
        f1 = torch.rand(P, 6, generator=torch.Generator().manual_seed(1)).to(dev)
        key = ("posed", ("v", 0), None)
        before = Rz.PASS_STATS["reblend"]
        miss = fused(sc.ins_feat, key, (0.1, 0.2, 0.3))
        assert Rz.KEPT_PASSES.stats["admitted"] == 1 and Rz.PASS_STATS["reblend"] == before
        hit = fused(sc.ins_feat, key, (0.1, 0.2, 0.3))
        assert Rz.PASS_STATS["reblend"] == before + 1
        full = fused(f1, None, (0.7, 0.0, 0.4))
        again = fused(f1, key, (0.7, 0.0, 0.4))
        assert Rz.PASS_STATS["reblend"] == before + 2
        for a, b, what in zip(miss + full, hit + again, ("color", "radii", "depth", "alpha") * 2):
            assert torch.equal(a, b), what
        assert int((full[1] > 0).sum()) > 0.5 * P
    finally:
        Rz.KEPT_PASSES = saved


def test_posed_render(gpu_device):
    """renderer.render() of a posed Camera: RGB and the 6-channel feature map against the oracle (no rescale draw)."""
    from opengaussian_amd.renderer import render
    from tests.test_11_render_gpu import FakeGaussians
    dev = gpu_device
    R, t = helpers.POSES["general"]
    P = 2500
    sc, cam = helpers.posed_scene(P, W, H, FX, FY, R, t, seed=71)
    bg = (0.2, 0.1, 0.3)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    pc = FakeGaussians(sc, dev)
    with torch.no_grad():
        out = render(cam.to(dev), pc, pipe, torch.tensor(bg, device=dev), iteration=1, rescale=False)
    feat = (torch.nn.functional.normalize(sc.ins_feat * 2 - 1, dim=1) + 1) / 2
    refA = _oracle_forward(helpers.oracle_inputs(sc, cam, use_sh=True), 3, bg)
    refB = _oracle_forward(helpers.oracle_inputs(sc, cam, feat=feat), 3, bg * 2)
    assert (refA["geom"].radii > 0).sum() > 0.5 * P
    np.testing.assert_array_equal(out["radii"].cpu().numpy(), refA["geom"].radii)
    assert torch.equal(out["visibility_filter"].cpu(), torch.from_numpy(refA["geom"].radii > 0))
    _assert_images(out["render"], out["depth"], out["alpha"], refA, "render RGB")
    _assert_images(out["ins_feat"], out["depth"], out["silhouette"], refB, "render ins_feat")
