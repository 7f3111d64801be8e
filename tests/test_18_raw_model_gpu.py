"""GPU: the rasterizer pass taken from the model's RAW parameters (include/ogs_model.h, rasterizer.rasterize_model).

  * ogs_model_activate against float64 torch, held to the larger of 4 ulp and twice the error of torch's own fp32 getters on the
    same inputs; the SH interleave exact; the edge rows (|q| = 0 and 1e-13, logits +-40, log-scale 100);
  * the raw pass == the existing pass fed with activate_model's outputs, bit for bit: images, radii, sorted keys, point list,
    tile ranges -- on the tiny, the small and the streaming geometry path, 3 and 9 channels, every SH layout;
  * raw-parameter gradients against float64 autograd through the oracle with the activations on top, and against the float64
    chain rule applied to the existing backward's gradients; exact zeros where they are owed; the g / eps rule;
  * render() with pipe.raw_model_pass on and off, and the calls that must not take the raw pass;
  * the argument errors of the new entry points.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import helpers
from tests import raw_model_restatement as rr

pytestmark = pytest.mark.gpu

W, H, FX, FY = 150, 90, 120.0, 85.0
TANX, TANY = helpers.tanfovs(W, H, FX, FY)
GRAD_TOL = 2e-4
SIZES = (200, 900, 1500)            # tiny_geometry_kernel, small_geometry_kernel, preprocess_kernel


def _raw_scene(P, seed, M=16):
    """posed scene (the general pose) as RAW parameters: log-scales, logits, quaternions of norm 0.3 .. 3, dc / rest split"""
    R, t = helpers.POSES["general"]
    sc, cam = helpers.posed_scene(P, W, H, FX, FY, R, t, seed=seed)
    g = torch.Generator().manual_seed(7000 + seed)
    op = sc.opacities.clamp(1e-4, 1 - 1e-4)
    raw = {"features_dc": sc.shs[:, :1].contiguous(), "features_rest": sc.shs[:, 1:M].contiguous() if M > 1 else None,
           "opacity": torch.log(op / (1 - op)), "scaling": torch.log(sc.scales),
           "rotation": sc.rotations * (0.3 + 2.7 * torch.rand(P, 1, generator=g))}
    return sc, cam, raw


def _dev(raw, dev, requires_grad=False):
    return {k: (None if v is None else v.to(dev).requires_grad_(requires_grad)) for k, v in raw.items()}


def _raw_args(r):
    return r["features_dc"], r["features_rest"], r["opacity"], r["scaling"], r["rotation"]


def _ulps(got, want64):
    """error of `got` (fp32) in units of the fp32 spacing at the float64 value (at least 2^-149: the spacing at zero is a
    denormal, which a process with flush-to-zero on -- other tests of the suite leave it on -- turns into 0)"""
    want64 = np.asarray(want64, np.float64)
    with np.errstate(over="ignore"):
        unit = np.maximum(np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64), 2.0 ** -149)
    return float((np.abs(np.asarray(got, np.float64) - want64) / unit).max()) if want64.size else 0.0


# ---- activations --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 4, 16])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 1500])
def test_activate_against_float64(gpu_device, P, M):
    from opengaussian_amd.rasterizer import activate_model
    g = torch.Generator().manual_seed(100 * P + M)
    raw = {"features_dc": torch.randn(P, 1, 3, generator=g), "features_rest": torch.randn(P, M - 1, 3, generator=g) if M > 1 else None,
           "opacity": torch.randn(P, 1, generator=g) * 4.0, "scaling": torch.randn(P, 3, generator=g) * 1.5 - 3.0,
           "rotation": torch.nn.functional.normalize(torch.randn(P, 4, generator=g)) * (0.3 + 2.7 * torch.rand(P, 1, generator=g))}
    d = _dev(raw, gpu_device)
    scales, rots, opac, shs = activate_model(*_raw_args(d))
    d64 = {k: (None if v is None else v.double()) for k, v in d.items()}
    want = rr.activate_torch(*_raw_args(d64))                       # float64 torch on the device
    torch32 = rr.activate_torch(*_raw_args(d))                      # torch's own fp32 getters
    n = lambda t_: t_.cpu().numpy()
    for name, got, w, t32 in zip(("scales", "rotations", "opacities"), (scales, rots, opac), want, torch32):
        e_kernel, e_torch = _ulps(n(got), n(w)), _ulps(n(t32), n(w))
        print(f"activate P={P} M={M} {name}: kernel {e_kernel:.2f} ulp, torch fp32 {e_torch:.2f} ulp")
        assert e_kernel <= max(4.0, 2.0 * e_torch), (name, e_kernel, e_torch)
    assert shs.shape == (P, M, 3) and torch.equal(shs, torch32[3]), "the SH interleave must be exact"


def test_activate_edge_rows_and_overflowing_scale(gpu_device):
    from opengaussian_amd import rasterizer as R
    dev = gpu_device
    sc, cam, raw = _raw_scene(300, seed=5)
    raw["rotation"][0] = 0.0
    raw["rotation"][1] = torch.tensor([0.6, 0.0, -0.8, 0.0]) * 1e-13
    raw["opacity"][2], raw["opacity"][3] = 40.0, -40.0
    raw["scaling"][4] = 100.0                                      # exp overflows
    d = _dev(raw, dev)
    scales, rots, opac, _ = R.activate_model(*_raw_args(d))
    want = rr.activate(*[None if v is None else v.numpy() for v in _raw_args(raw)])
    assert torch.all(rots[0] == 0)
    assert _ulps(rots[1].cpu().numpy(), want[1][1]) <= 4.0 and abs(float(rots[1].norm()) - 0.1) < 1e-6
    assert float(opac[2]) == 1.0 and _ulps(opac[3].cpu().numpy(), want[2][3]) <= 4.0 and float(opac[3]) > 0
    assert torch.isinf(scales[4]).all()
    # the pass itself: the radius guard gives the overflowing row radius 0 and the call succeeds, finite images
    rs = helpers.settings_for(cam, (0.1, 0.2, 0.3), 3, dev)
    color, radii, depth, alpha = R.rasterize_model(sc.means3D.to(dev), torch.zeros(300, 3, device=dev), *_raw_args(d), rs)
    assert int(radii[4]) == 0 and int((radii > 0).sum()) > 100
    assert torch.isfinite(color).all() and torch.isfinite(alpha).all() and torch.isfinite(depth).all()


# ---- raw pass == existing pass on activate_model's outputs, bit for bit ---------------------------------------------------
def _both_passes(dev, sc, cam, raw, Cn, deg, requires_grad=False, detach_extra=True):
    """-> (raw outputs, raw leaves, existing outputs, activated leaves)"""
    from opengaussian_amd import rasterizer as R
    P = sc.means3D.shape[0]
    rs = helpers.settings_for(cam, (0.1, 0.2, 0.3), deg, dev)
    leaf = lambda t_: t_.detach().clone().to(dev).requires_grad_(requires_grad)
    extra = sc.ins_feat[:, :Cn - 3].contiguous() if Cn > 3 else None
    r = {k: (None if v is None else leaf(v)) for k, v in raw.items()}
    r.update(means3D=leaf(sc.means3D), means2D=leaf(torch.zeros(P, 3)), extra=None if extra is None else leaf(extra))
    out_raw = R.rasterize_model(r["means3D"], r["means2D"], *_raw_args(r), rs, extra_feats=r["extra"],
                                detach_extra_from_geometry=detach_extra)
    scales, rots, opac, shs = R.activate_model(*_raw_args(r))
    a = dict(means3D=leaf(sc.means3D), means2D=leaf(torch.zeros(P, 3)), scales=leaf(scales), rotations=leaf(rots),
             opacities=leaf(opac), shs=leaf(shs), extra=None if extra is None else leaf(extra))
    if Cn == 3:
        empty = torch.Tensor([])
        out_act = R.rasterize_gaussians(a["means3D"], a["means2D"], a["shs"], empty, a["opacities"], a["scales"], a["rotations"],
                                        empty, rs)
    else:
        out_act = R.rasterize_fused(a["means3D"], a["means2D"], a["opacities"], a["shs"], a["extra"], rs, scales=a["scales"],
                                    rotations=a["rotations"], detach_extra_from_geometry=detach_extra)
    return out_raw, r, out_act, a


# (P, channels, M, active degree): every geometry path x both channel counts; active degree below the stored one; M = 1
BIT_CASES = [(200, 3, 16, 2), (200, 9, 1, 0), (900, 3, 9, 1), (900, 9, 16, 3), (1500, 3, 1, 0), (1500, 9, 16, 2),
             (1500, 3, 4, 0), (900, 3, 16, 0)]


@pytest.mark.parametrize("P,Cn,M,deg", BIT_CASES)
def test_raw_pass_is_bit_identical_to_the_existing_pass(gpu_device, P, Cn, M, deg):
    from opengaussian_amd import rasterizer as R
    sc, cam, raw = _raw_scene(P, seed=300 + P + Cn, M=M)
    with torch.no_grad():
        n0 = R.PASS_STATS["raw_model"], R.PASS_STATS["tiny"]
        out_raw, _, out_act, _ = _both_passes(gpu_device, sc, cam, raw, Cn, deg)
        assert R.PASS_STATS["raw_model"] == n0[0] + 1
        assert R.PASS_STATS["tiny"] - n0[1] == (2 if P <= R.TINY_MAX_P else 0)      # both took the same geometry path
    assert int((out_raw[1] > 0).sum()) > P // 2
    for name, x, y in zip(("colour", "radii", "depth", "alpha"), out_raw, out_act):
        assert torch.equal(x, y), f"{name} differs between the raw and the existing pass"
    # the binning state: the reference's full lists of both passes (the tiny path keeps none: its streaming re-run is exported)
    saved, R.TINY_MAX_P = R.TINY_MAX_P, 0
    try:
        with R.full_binning():
            out_raw, _, out_act, _ = _both_passes(gpu_device, sc, cam, raw, Cn, deg, requires_grad=True)
            b_raw, b_act = helpers.hip_export_binning(out_raw[0]), helpers.hip_export_binning(out_act[0])
    finally:
        R.TINY_MAX_P = saved
    for name, x, y in zip(("keys", "ranges", "n_contrib", "point list"), b_raw, b_act):
        np.testing.assert_array_equal(x, y, err_msg=name)
    assert len(b_raw[0]) > 0
    for x, y in zip(out_raw, out_act):
        assert torch.equal(x, y)


# ---- gradients -----------------------------------------------------------------------------------------------------------
def _upstream(Cn, seed, dev):
    g = np.random.default_rng(seed)
    gC, gD, gA = g.standard_normal((Cn, H, W)), g.standard_normal((1, H, W)) * 0.05, g.standard_normal((1, H, W))
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    return (gC, gD, gA), (t(gC), t(gD), t(gA))


def _raw_grads_of(r):
    g = lambda t_: None if t_ is None or t_.grad is None else t_.grad.detach().cpu().double().numpy()
    return {"_xyz": g(r["means3D"]), "means2D": g(r["means2D"]), "_features_dc": g(r["features_dc"]),
            "_features_rest": g(r["features_rest"]), "_opacity": g(r["opacity"]), "_scaling": g(r["scaling"]),
            "_rotation": g(r["rotation"]), "extra": g(r["extra"])}


def _chain(raw, g_act):
    """float64 chain rule over gradients w.r.t. the activated arrays (dict: scales, rotations, opacities, shs, means3D, means2D)"""
    c = rr.chain_rule(raw["scaling"].numpy(), raw["rotation"].numpy(), raw["opacity"].numpy(), g_act["scales"], g_act["rotations"],
                      g_act["opacities"], g_act["shs"])
    return {"_xyz": g_act["means3D"], "means2D": g_act["means2D"], "_features_dc": c["features_dc"],
            "_features_rest": c["features_rest"], "_opacity": c["opacity"], "_scaling": c["scaling"], "_rotation": c["rotation"]}


@pytest.mark.parametrize("P", SIZES)
def test_raw_gradients_against_the_float64_oracle(gpu_device, P):
    """SH pass, 16 stored coefficients, active degree 2.  The oracle differentiates the rasterizer in float64 on the activated
    arrays the device used (activate_model's, so both see one binning); the activations' chain rule follows in float64."""
    from oracle import raster_oracle as ro
    dev = gpu_device
    deg, bg = 2, (0.1, 0.2, 0.3)
    sc, cam, raw = _raw_scene(P, seed=500 + P)
    out_raw, r, out_act, a = _both_passes(dev, sc, cam, raw, 3, deg, requires_grad=True)
    (gC, gD, gA), up = _upstream(3, P, dev)
    torch.autograd.backward([out_raw[0], out_raw[2], out_raw[3]], list(up))
    got = _raw_grads_of(r)
    inp = dict(means3D=sc.means3D.numpy(), opacities=a["opacities"].detach().cpu().numpy(), scales=a["scales"].detach().cpu().numpy(),
               rotations=a["rotations"].detach().cpu().numpy(), shs=a["shs"].detach().cpu().numpy(),
               viewmatrix=cam.world_view_transform.numpy(), projmatrix=cam.full_proj_transform.numpy(),
               campos=cam.camera_center.numpy())
    ref = ro.render_forward(W=W, H=H, tanfovx=TANX, tanfovy=TANY, bg=np.array(bg, np.float32), sh_degree=deg, **inp)
    np.testing.assert_array_equal(out_raw[1].cpu().numpy(), ref["geom"].radii)
    back = lambda dtype: _chain(raw, ro.render_backward_f64(inp, ref["binning"], W, H, TANX, TANY, np.array(bg, np.float64), gC, gD,
                                                            gA, sh_degree=deg, dtype=dtype))
    want = back(torch.float64)
    want32 = helpers.lazy(lambda: back(torch.float32))
    for k, w in want.items():
        e = helpers.assert_grad_family_close_modulo_threshold_flips(got[k], w.reshape(got[k].shape), GRAD_TOL,
                                                                    lambda k=k: want32()[k], what=f"P={P} {k}")
        print(f"raw gradients vs oracle P={P} {k}: {e:.1e}")
    # rows above the active degree, and every row of a culled Gaussian: exact zeros
    assert np.all(got["_features_rest"][:, (deg + 1) ** 2 - 1:] == 0.0)
    culled = out_raw[1].cpu().numpy() == 0
    assert culled.any()
    for k in ("_xyz", "means2D", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        assert np.all(got[k][culled] == 0.0), k


@pytest.mark.parametrize("Cn", [3, 9])
@pytest.mark.parametrize("P", SIZES)
def test_raw_gradients_against_chain_rule_over_the_existing_backward(gpu_device, P, Cn):
    dev = gpu_device
    sc, cam, raw = _raw_scene(P, seed=600 + P + Cn, M=9)
    out_raw, r, out_act, a = _both_passes(dev, sc, cam, raw, Cn, 1, requires_grad=True)
    _, up = _upstream(Cn, P + Cn, dev)
    torch.autograd.backward([out_raw[0], out_raw[2], out_raw[3]], list(up))
    torch.autograd.backward([out_act[0], out_act[2], out_act[3]], list(up))
    got = _raw_grads_of(r)
    g_act = {k: a[k].grad.detach().cpu().double().numpy() for k in ("means3D", "means2D", "scales", "rotations", "opacities", "shs")}
    want = _chain(raw, g_act)
    for k, w in want.items():
        helpers.assert_grad_family_close(got[k], w.reshape(got[k].shape), GRAD_TOL, what=f"P={P} C={Cn} {k}")
    if Cn > 3:
        assert torch.equal(r["extra"].grad, a["extra"].grad)
    # untouched rows (visible, no gradient reached them) and culled rows: exact zeros, as the existing backward writes them
    idle = np.all(g_act["shs"].reshape(P, -1) == 0, axis=1) & np.all(g_act["scales"] == 0, axis=1) & (g_act["opacities"].reshape(-1) == 0)
    assert idle.any()
    for k in ("_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        assert np.all(got[k][idle] == 0.0), k
    assert np.all(got["_features_rest"][:, 3:] == 0.0)             # active degree 1 of 9 stored coefficients


def test_tiny_quaternion_row_follows_the_g_over_eps_rule(gpu_device):
    dev = gpu_device
    P = 200
    sc, cam, raw = _raw_scene(P, seed=77)
    with torch.no_grad():
        row = int(_both_passes(dev, sc, cam, raw, 3, 3)[0][1].argmax())          # a large footprint: it receives gradient
    raw["rotation"][row] = sc.rotations[row] * 1e-13
    out_raw, r, out_act, a = _both_passes(dev, sc, cam, raw, 3, 3, requires_grad=True)
    assert int(out_raw[1][row]) > 0
    _, up = _upstream(3, 3, dev)
    torch.autograd.backward([out_raw[0], out_raw[2], out_raw[3]], list(up))
    torch.autograd.backward([out_act[0], out_act[2], out_act[3]], list(up))
    g = a["rotations"].grad[row].double().cpu().numpy()
    assert np.abs(g).max() > 0
    got = r["rotation"].grad[row].double().cpu().numpy()
    assert np.abs(got - g / 1e-12).max() <= 1e-4 * np.abs(g / 1e-12).max(), (got, g / 1e-12)


def test_only_extra_feats_requiring_grad_runs_the_features_only_backward(gpu_device):
    from opengaussian_amd import rasterizer as R
    dev = gpu_device
    P = 1500
    sc, cam, raw = _raw_scene(P, seed=88)
    rs = helpers.settings_for(cam, (0.0, 0.0, 0.0), 3, dev)
    d = _dev(raw, dev)
    leaves = [sc.means3D.to(dev), torch.zeros(P, 3, device=dev), *_raw_args(d)]
    extra = sc.ins_feat.to(dev).requires_grad_(True)
    out = R.rasterize_model(*leaves, rs, extra_feats=extra)
    assert out[0].grad_fn.bwd_clear_bytes == P * 64                # the record of a features-only backward: the feature sums alone
    _, up = _upstream(9, 9, dev)
    out[0].backward(up[0])
    assert all(t_.grad is None for t_ in leaves if t_ is not None)
    scales, rots, opac, shs = R.activate_model(*_raw_args(d))
    extra2 = sc.ins_feat.to(dev).requires_grad_(True)
    out2 = R.rasterize_fused(leaves[0], leaves[1], opac, shs, extra2, rs, scales=scales, rotations=rots)
    out2[0].backward(up[0])
    assert torch.equal(out[0], out2[0]) and torch.equal(extra.grad, extra2.grad)


# ---- render() ------------------------------------------------------------------------------------------------------------
def _render_call(dev, raw_pass, kwargs, requires_grad=True, override=False):
    from opengaussian_amd import rasterizer as R
    from opengaussian_amd.renderer import render
    from tests.golden import render_cases as rc
    case = rc.build("stage1_norescale")
    pc = rc.TinyModel(case["params"], dev, requires_grad=requires_grad)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    if raw_pass is not None:
        pipe.raw_model_pass = raw_pass
    kw = dict(kwargs)
    if override:
        kw["override_color"] = torch.rand(pc._xyz.shape[0], 3, device=dev)
    n0 = R.PASS_STATS["raw_model"]
    torch.manual_seed(kw.pop("rng_seed", case["rng_seed"]))
    with (torch.enable_grad() if requires_grad else torch.no_grad()):
        out = render(case["cam"].to(dev), pc, pipe, case["bg"].to(dev), 1, **kw)
        if requires_grad:
            rc.fixed_loss(out).backward()
    return out, pc, R.PASS_STATS["raw_model"] - n0, case


def _radius_margin_ok(case):
    """rows whose float64 3 sqrt(lambda) (oracle's preprocess in float64 over float64 activations) is farther than 1e-4 from an integer"""
    from oracle import raster_oracle as ro
    p, cam = case["params"], case["cam"]
    Wc, Hc = int(cam.image_width), int(cam.image_height)
    scales, rots, opac, _ = rr.activate(p["_features_dc"].numpy(), None, p["_opacity"].numpy(), p["_scaling"].numpy(), p["_rotation"].numpy())
    t = lambda a_: torch.tensor(np.asarray(a_), dtype=torch.float64)
    import math
    tanx, tany = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    P = scales.shape[0]
    _, conic, _, _, _ = ro.preprocess_t(t(p["_xyz"]), torch.zeros(P, 3, dtype=torch.float64), t(opac), t(cam.world_view_transform),
                                        t(cam.full_proj_transform), t(cam.camera_center).reshape(3), Wc, Hc, tanx, tany,
                                        scales=t(scales), rotations=t(rots), colors_precomp=torch.zeros(P, 3, dtype=torch.float64))
    A, B, Cc = conic[:, 0].numpy(), conic[:, 1].numpy(), conic[:, 2].numpy()
    detc = A * Cc - B * B                                          # = 1 / det(cov2D)
    ca, cc, det = Cc / detc, A / detc, 1.0 / detc
    mid = 0.5 * (ca + cc)
    lam = mid + np.sqrt(np.maximum(0.1, mid * mid - det))
    v = 3.0 * np.sqrt(lam)
    return ~(np.abs(v - np.round(v)) <= 1e-4) | ~np.isfinite(v)


@pytest.mark.parametrize("call", ["stage0", "fused"])
def test_render_raw_model_pass_on_and_off(gpu_device, call):
    from tests.golden import render_cases as rc
    dev = gpu_device
    kwargs = dict(render_feat_map=False, rescale=False) if call == "stage0" else dict(render_feat_map=True, rescale=False)
    out_off, pc_off, n_off, case = _render_call(dev, False, kwargs)
    out_abs, _, n_abs, _ = _render_call(dev, None, kwargs)
    out_on, pc_on, n_on, _ = _render_call(dev, True, kwargs)
    assert n_off == 0 and n_abs == 0, "without the attribute (or with it off) the call takes the present path"
    assert n_on == 1
    assert list(out_on) == list(out_off)
    for k in rc.TENSOR_KEYS:
        if out_off[k] is None:
            assert out_on[k] is None, k
            continue
        assert torch.equal(out_off[k], out_abs[k])
        helpers.assert_close_modulo_threshold_flips(out_on[k].detach().cpu().numpy(), out_off[k].detach().cpu().numpy(),
                                                    tol=1e-3 if k == "depth" else 1e-4, flip_tol=4e-2 if k == "depth" else 4e-3)
    ok = _radius_margin_ok(case)
    assert (~ok).mean() <= 0.01, "the seeded scene leaves more than 1 % of its radii within 1e-4 of an integer"
    r_on, r_off = out_on["radii"].cpu().numpy(), out_off["radii"].cpu().numpy()
    np.testing.assert_array_equal(r_on[ok], r_off[ok])
    assert np.array_equal(out_on["visibility_filter"].cpu().numpy()[ok], (r_off > 0)[ok])
    fam_on = {n: getattr(pc_on, n).grad for n in rc.PARAM_NAMES}
    fam_off = {n: getattr(pc_off, n).grad for n in rc.PARAM_NAMES}
    fam_on["viewspace_points"], fam_off["viewspace_points"] = out_on["viewspace_points"].grad, out_off["viewspace_points"].grad
    assert fam_on["viewspace_points"] is not None
    for n, g_off in fam_off.items():
        if g_off is None:
            assert fam_on[n] is None, n
            continue
        helpers.assert_grad_family_close(fam_on[n].cpu().double().numpy(), g_off.cpu().double().numpy(), GRAD_TOL, what=f"{call} {n}")


def test_render_calls_that_must_not_take_the_raw_pass(gpu_device):
    from opengaussian_amd import rasterizer as R
    dev = gpu_device
    # seed 1: the coin says "rescale" (0.7576 > 0.5) and rescale=True lets it
    assert _render_call(dev, True, dict(rescale=True, rng_seed=1))[2] == 0
    assert _render_call(dev, True, dict(rescale=False, render_feat_map=False), override=True)[2] == 0
    # a fully detached model: the frozen-geometry caches serve the call (stage >= 1), not the raw pass
    R.clear_kept()
    assert R.KEPT_PASSES.enabled(dev)
    assert _render_call(dev, True, dict(rescale=False), requires_grad=False)[2] == 0
    assert _render_call(dev, True, dict(rescale=False, render_feat_map=False), requires_grad=False)[2] == 0
    R.clear_kept()


# ---- argument errors -------------------------------------------------------------------------------------------------------
def test_raw_entry_argument_errors(gpu_device):
    from opengaussian_amd import _lib
    from opengaussian_amd import rasterizer as R
    dev = gpu_device
    lib = _lib.lib()
    P = 300
    sc, cam, raw = _raw_scene(P, seed=9)
    d = _dev(raw, dev)
    rs = helpers.settings_for(cam, (0.0, 0.0, 0.0), 3, dev)
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    keep = [sc.means3D.to(dev), f(3), rs.viewmatrix.contiguous(), rs.projmatrix.contiguous(), rs.campos.contiguous(), f(3, H, W),
            f(1, H, W), f(1, H, W), torch.zeros(P, dtype=torch.int32, device=dev),
            torch.empty(int(lib.ogs_raster_geom_bytes(P, 3)), dtype=torch.uint8, device=dev),
            torch.empty(int(lib.ogs_raster_geom_tmp_bytes(P)), dtype=torch.uint8, device=dev)]

    def args():
        a = R._fwd_args(rs, P, 3, keep[0], None, None, None, None, None, None, keep[1], keep[2], keep[3], keep[4], keep[5], keep[6],
                        keep[7], keep[8], None, 1)
        a.sh_coeffs = 16
        a.geom_buffer, a.geom_tmp = keep[9].data_ptr(), keep[10].data_ptr()
        return a
    stream = torch.cuda.current_stream().cuda_stream
    n = C.c_int64(0)
    rm = R._raw_model_struct(*[d[k] for k in ("features_dc", "features_rest", "opacity", "scaling", "rotation")])
    a = args()
    assert lib.ogs_raster_forward_geometry_raw(C.byref(a), C.byref(rm), stream, C.byref(n)) == 0 and n.value > 0
    a = args()
    a.shs = d["features_dc"].data_ptr()
    assert lib.ogs_raster_forward_geometry_raw(C.byref(a), C.byref(rm), stream, C.byref(n)) == -1        # OGS_ERR_INVALID_ARG
    assert lib.ogs_raster_forward_tiny_raw(C.byref(a), C.byref(rm), stream) == -1
    assert b"must be NULL" in lib.ogs_last_error()
    a = args()
    no_rest = R._raw_model_struct(d["features_dc"], None, d["opacity"], d["scaling"], d["rotation"])
    assert lib.ogs_raster_forward_geometry_raw(C.byref(a), C.byref(no_rest), stream, C.byref(n)) == -1
    assert b"features_rest" in lib.ogs_last_error()
    b = _lib.OgsRasterBwdArgs()
    b.P, b.W, b.H, b.C, b.sh_coeffs = P, W, H, 3, 16
    assert lib.ogs_raster_backward_raw(C.byref(b), C.byref(no_rest), None, stream) == -1
    b.shs = d["features_dc"].data_ptr()
    assert lib.ogs_raster_backward_raw(C.byref(b), C.byref(rm), None, stream) == -1
    torch.cuda.synchronize()
