"""GPU: camera gradients of a pass (include/ogs_raster.h: dL_dviewmatrix, dL_dprojmatrix, dL_dcampos; csrc/pose_bwd.hip).

  1. parity through the C ABI against tests/pose_grad_restatement.py on the cases of tests/pose_grad_cases.py, at
     |got - ref| <= 2e-4 S per entry (S = the sum over the Gaussians of the magnitudes of their contributions);
  2. the never-read entries and campos without SH are exact zeros; canaries around the outputs and pose_tmp are untouched;
  3. asking for the camera gradients changes no per-Gaussian gradient;
  4. two complete runs give the same 35 floats bit for bit;
  5. the translation identity from device outputs alone, also past one chunk of the second launch;
  6. the facade: GaussianRasterizer, a pose-only pass, rasterize_model, the tiny path, render(), no pose kernel for constant
     cameras, no kept pass for a camera that trains;
  7. the route a user had (the se(3) delta applied to the scene in torch) gives the same six numbers;
  8. one small step against the gradient lowers the device's own loss.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import helpers
from tests import pose_grad_cases as pc
from tests import pose_grad_restatement as pr

pytestmark = pytest.mark.gpu

_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """the session cache of this file holds device state (the saved tensors of eleven passes): released when the file is done"""
    yield
    import gc
    _RUNS.clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _run(name, dev):
    """forward + ogs_raster_backward with the camera outputs of a case, once per session: (autograd node, results)"""
    if name not in _RUNS:
        c = pc.case(name)
        ctx, leaves, out = pc.device_forward(c, dev)
        _RUNS[name] = (ctx, pc.device_backward(c, ctx, dev, pose=True), out)
    return _RUNS[name][:2]


# ---- 1, 2: parity, exact zeros, canaries ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.PARITY_CASES)
def test_parity_through_the_c_abi(gpu_device, name):
    c = pc.case(name)
    ref = pc.reference(name)
    _, got = _run(name, gpu_device)
    assert got["rc"] == 0, got["error"]
    worst = pc.worst_error(got, ref)
    print(f"pose parity {name}: max |got - ref| / S =", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= pr.BAR, f"{name}: {k}: {v:.3e} of S"
    # never read by a pass: exact zeros, not small numbers
    assert (got["viewmatrix"][[3, 7, 11, 15]] == 0).all() and (got["projmatrix"][[2, 6, 10, 14]] == 0).all()
    assert not np.signbit(got["viewmatrix"][[3, 7, 11, 15]]).any() and not np.signbit(got["projmatrix"][[2, 6, 10, 14]]).any()
    if not c.spec.sh:
        assert (got["campos"] == 0).all()
    else:
        assert (got["campos"] != 0).all()
    assert got["canaries_intact"]


def _looking_away_case():
    """the `general` scene's camera-frame twin seen by a camera turned half round: every Gaussian behind it"""
    c = pc.case("general")
    W, H, fx, fy = pc.SMALL
    cam = helpers.general_camera(W, H, fx, fy, np.diag([-1.0, 1.0, -1.0]), (0.0, 0.0, 0.0))
    from opengaussian_amd.synthetic import make_scene
    sc = make_scene(300, W, H, fx, fy, seed=1, log_scale_mean=-3.0)
    return pc.Case("culled", pc.Spec(300), sc, cam, helpers.oracle_inputs(sc, cam), None, W, H, c.tanfovx, c.tanfovy, c.gC, c.gD,
                   c.gA, None)


def test_a_view_that_culls_everything_and_an_empty_scene_give_35_zeros(gpu_device):
    from opengaussian_amd import _lib
    dev = gpu_device
    c = _looking_away_case()
    ctx, _, out = pc.device_forward(c, dev)
    assert int((out[1] > 0).sum()) == 0 and ctx.num_rendered == 0
    got = pc.device_backward(c, ctx, dev, pose=True)
    assert got["rc"] == 0, got["error"]
    for k in ("viewmatrix", "projmatrix", "campos"):
        assert (got[k] == 0).all() and not np.signbit(got[k]).any(), k
    assert got["canaries_intact"]
    # P = 0: nothing to read, the 35 floats are still written
    lib = _lib.lib()
    b = _lib.OgsRasterBwdArgs()
    b.P, b.W, b.H, b.C = 0, 64, 48, 3
    buf, tmp, n_tmp = pc.pose_buffers(lib, b, 0, dev)
    assert lib.ogs_raster_backward(C.byref(b), torch.cuda.current_stream().cuda_stream) == 0, lib.ogs_last_error()
    torch.cuda.synchronize()
    got = pc.read_pose_buffers(buf, tmp, n_tmp)
    assert all((got[k] == 0).all() for k in ("viewmatrix", "projmatrix", "campos")) and got["canaries_intact"]


def test_argument_errors_come_before_any_launch(gpu_device):
    c = pc.case("general")
    ctx, _ = _run("general", gpu_device)
    for field in ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos", "pose_tmp"):
        got = pc.device_backward(c, ctx, gpu_device, pose=True, only={field: None})
        assert got["rc"] == -1 and "together" in got["error"], (field, got)           # OGS_ERR_INVALID_ARG
        assert all(np.isnan(got[k]).all() for k in ("means3D", "opacities", "shs")), "an output was written before the check"
    got = pc.device_backward(c, ctx, gpu_device, pose=True, only={"num_groups": 2})
    assert got["rc"] == -3 and "grouped" in got["error"]                                   # OGS_ERR_UNSUPPORTED
    assert np.isnan(got["means3D"]).all()
    got = pc.device_backward(c, ctx, gpu_device, pose=True, only={"scales": None})
    assert got["rc"] == -1 and np.isnan(got["means3D"]).all()


# ---- 3, 4 ---------------------------------------------------------------------------------------------------------------------
FAMILIES = ("means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")


@pytest.mark.parametrize("name", ["general_b", "rgb_clamp", "fused9", "cov"])
def test_pose_outputs_change_no_per_gaussian_gradient(gpu_device, name):
    c = pc.case(name)
    ctx, with_pose = _run(name, gpu_device)
    without = pc.device_backward(c, ctx, gpu_device, pose=False)
    assert without["rc"] == 0
    seen = [k for k in FAMILIES if k in without]
    assert len(seen) >= 5
    for k in seen:
        assert not np.isnan(without[k]).any(), k
        assert np.array_equal(with_pose[k], without[k]), k


def test_two_complete_runs_give_the_same_bits(gpu_device):
    name = "general_b"
    c = pc.case(name)
    _, first = _run(name, gpu_device)
    ctx2, _, _ = pc.device_forward(c, gpu_device)
    second = pc.device_backward(c, ctx2, gpu_device, pose=True)
    for k in ("viewmatrix", "projmatrix", "campos"):
        assert np.array_equal(first[k], second[k]), k
    # per-Gaussian families: the standard of test_90 (an fp64 record of float atomics, rounded once)
    for k in FAMILIES:
        if k in first:
            scale = np.abs(first[k]).max() + 1e-12
            assert np.abs(first[k] - second[k]).max() / scale < 1e-6, k


# ---- 5: the translation identity ------------------------------------------------------------------------------------------------
def _assert_translation_identity(inputs, got, tag):
    lhs, rhs, scale = pr.translation_identity(inputs["viewmatrix"], inputs["projmatrix"], got["viewmatrix"], got["projmatrix"],
                                              got["campos"], got["means3D"])
    err = np.abs(lhs - rhs) / scale
    print(f"translation identity {tag}: |lhs - rhs| / sum |dL/dmean| =", err)
    assert (err <= pr.BAR).all(), (tag, lhs, rhs, scale)


@pytest.mark.parametrize("name", pc.PARITY_CASES)
def test_translation_identity_on_the_parity_scenes(gpu_device, name):
    _, got = _run(name, gpu_device)
    _assert_translation_identity(pc.case(name).inputs, got, name)


def test_translation_identity_past_one_chunk_of_the_second_launch(gpu_device):
    """P = 256 chunk + 1: the second launch takes two steps, the second of one row that holds one Gaussian.  No oracle at this
    size: the identity ties the new outputs to dL/dmeans3D, which the suite tests on its own."""
    from opengaussian_amd import _lib
    chunk = int(_lib.lib().ogs_pose_partial_chunk())
    P = 256 * chunk + 1
    assert 256 < P <= 400_000, P
    W = H = 64
    f = 60.0
    R, t = helpers.POSES["general"]
    sc, cam = helpers.posed_scene(P, W, H, f, f, R, t, seed=21, log_scale_mean=-4.5)
    tanx, tany = helpers.tanfovs(W, H, f, f)
    g = torch.Generator().manual_seed(5)
    c = pc.Case("chunk", pc.Spec(P), sc, cam, helpers.oracle_inputs(sc, cam), None, W, H, tanx, tany,
                torch.randn(3, H, W, generator=g).numpy(), torch.randn(1, H, W, generator=g).numpy() * 0.1,
                torch.randn(1, H, W, generator=g).numpy(), None)
    ctx, _, out = pc.device_forward(c, gpu_device)
    got = pc.device_backward(c, ctx, gpu_device, pose=True)
    assert got["rc"] == 0 and got["canaries_intact"]
    # the Gaussian of the last row, alone in the second step, must be one that receives gradient
    assert np.abs(got["means3D"][-1]).max() > 0 or np.abs(got["means3D"][-257:]).max() > 0
    _assert_translation_identity(c.inputs, got, f"P={P}")
    assert (got["viewmatrix"][[3, 7, 11, 15]] == 0).all() and (got["projmatrix"][[2, 6, 10, 14]] == 0).all()


# ---- 6: the facade --------------------------------------------------------------------------------------------------------------
def _upstream(c, dev):
    td = lambda a: None if a is None else torch.tensor(a, dtype=torch.float32, device=dev)
    return td(c.gC), td(c.gD), td(c.gA)


def _backward(out, ups):
    color, _, depth, alpha = out
    pairs = [(color, ups[0])] + ([(depth, ups[1]), (alpha, ups[2])] if ups[1] is not None else [])
    torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs])


def _facade(c, dev, cam, requires_grad, tiny=False):
    from opengaussian_amd import rasterizer as R
    saved = R.TINY_MAX_P
    if not tiny:
        R.TINY_MAX_P = 0
    try:
        return helpers._hip_forward(c.inputs, cam, pc.BG, c.sh_degree, dev, requires_grad, False, c.spec.scale_modifier)
    finally:
        R.TINY_MAX_P = saved


def _close(a, b, rel=1e-5):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) <= rel * float(b.abs().max())


def test_camera_pose_gradient_is_the_chain_rule_of_the_c_abi_outputs(gpu_device):
    from opengaussian_amd import _lib
    from opengaussian_amd.pose import CameraPose
    dev = gpu_device
    name = "general_b"
    c = pc.case(name)
    _, got = _run(name, dev)
    want = pr.chain_to_delta(CameraPose(c.cam.to(dev)), got["viewmatrix"], got["projmatrix"], got["campos"])
    assert float(want.abs().min()) > 0
    # everything trains
    cp = CameraPose(c.cam.to(dev))
    out, leaves = _facade(c, dev, cp, True)
    _backward(out, _upstream(c, dev))
    assert _close(cp.delta.grad, want), (cp.delta.grad, want)
    for k in ("means3D", "opacities", "shs", "scales", "rotations"):
        assert np.array_equal(leaves[k].grad.cpu().numpy().reshape(got[k].shape), got[k]) or \
            np.abs(leaves[k].grad.cpu().numpy().reshape(got[k].shape) - got[k]).max() <= 1e-6 * np.abs(got[k]).max(), k
    # only the pose trains: the same six numbers, and no per-Gaussian kernel runs because no per-Gaussian output exists
    cp2 = CameraPose(c.cam.to(dev))
    out, leaves = _facade(c, dev, cp2, False)
    assert out[0].requires_grad
    _lib.prof_enable(1)
    try:
        _backward(out, _upstream(c, dev))
        torch.cuda.synchronize()
        prof = _lib.prof_collect()
    finally:
        _lib.prof_enable(0)
    assert _close(cp2.delta.grad, want), (cp2.delta.grad, want)
    assert all(t.grad is None for t in leaves.values() if t is not None)
    assert any(k.startswith("pose_partials_kernel") for k in prof) and "pose_fold_kernel" in prof, sorted(prof)
    assert not any(k.startswith("preprocess_backward_kernel") for k in prof), sorted(prof)
    assert any(k.startswith("blend_backward_kernel") for k in prof), sorted(prof)


def test_constant_cameras_launch_no_pose_kernel(gpu_device):
    from opengaussian_amd import _lib
    dev = gpu_device
    c = pc.case("general")
    _lib.prof_enable(1)
    try:
        out, _ = _facade(c, dev, c.cam, True)
        _backward(out, _upstream(c, dev))
        torch.cuda.synchronize()
        prof = _lib.prof_collect()
    finally:
        _lib.prof_enable(0)
    assert any(k.startswith("preprocess_backward_kernel") for k in prof), sorted(prof)
    assert not any(k.startswith("pose_") for k in prof), sorted(prof)
    # a camera that requires grad under no_grad is a constant too
    from opengaussian_amd.pose import CameraPose
    with torch.no_grad():
        out, _ = _facade(c, dev, CameraPose(c.cam.to(dev)), False)
    assert not out[0].requires_grad


def test_tiny_path(gpu_device):
    """P <= the tiny limit: two launches forward, the backward re-renders through the streaming path and the camera gradients
    come out of that"""
    dev = gpu_device
    c = pc.case("P255")
    rs_cam = types.SimpleNamespace(
        image_height=c.cam.image_height, image_width=c.cam.image_width, FoVx=c.cam.FoVx, FoVy=c.cam.FoVy,
        world_view_transform=c.cam.world_view_transform.to(dev).requires_grad_(True),
        full_proj_transform=c.cam.full_proj_transform.to(dev).requires_grad_(True),
        camera_center=c.cam.camera_center.to(dev).requires_grad_(True))
    out, _ = _facade(c, dev, rs_cam, False, tiny=True)
    assert out[0].grad_fn.tiny
    _backward(out, _upstream(c, dev))
    got = {"viewmatrix": rs_cam.world_view_transform.grad.cpu().numpy().reshape(16),
           "projmatrix": rs_cam.full_proj_transform.grad.cpu().numpy().reshape(16),
           "campos": rs_cam.camera_center.grad.cpu().numpy()}
    worst = pc.worst_error(got, pc.reference("P255"))
    assert max(worst.values()) <= pr.BAR, worst
    assert rs_cam.world_view_transform.grad.shape == (4, 4)


def _raw_of(sc, seed=3):
    g = torch.Generator().manual_seed(7100 + seed)
    op = sc.opacities.clamp(1e-4, 1 - 1e-4)
    return {"features_dc": sc.shs[:, :1].contiguous(), "features_rest": sc.shs[:, 1:].contiguous(),
            "opacity": torch.log(op / (1 - op)), "scaling": torch.log(sc.scales),
            "rotation": sc.rotations * (0.3 + 2.7 * torch.rand(sc.rotations.shape[0], 1, generator=g))}


@pytest.mark.parametrize("name", ["general", "P255"])
def test_raw_model_pass_equals_the_plain_pass(gpu_device, name):
    """rasterize_model (the raw instantiation of the first launch; P255: through the tiny path's re-render) against the plain pass
    fed with activate_model's outputs, per entry within the bar of the case's S"""
    from opengaussian_amd import rasterizer as R
    dev = gpu_device
    c = pc.case(name)
    raw = {k: v.to(dev) for k, v in _raw_of(c.scene).items()}
    ups = _upstream(c, dev)
    m3 = c.scene.means3D.to(dev)
    m2 = torch.zeros_like(m3)

    def cam_leaves():
        return (c.cam.world_view_transform.to(dev).requires_grad_(True), c.cam.full_proj_transform.to(dev).requires_grad_(True),
                c.cam.camera_center.to(dev).requires_grad_(True))

    def settings(leaves):
        return helpers.settings_for(c.cam, pc.BG, 3, dev)._replace(viewmatrix=leaves[0], projmatrix=leaves[1], campos=leaves[2])

    la = cam_leaves()
    out = R.rasterize_model(m3, m2, raw["features_dc"], raw["features_rest"], raw["opacity"], raw["scaling"], raw["rotation"],
                            settings(la))
    _backward(out, ups)
    scales, rotations, opacities, shs = R.activate_model(raw["features_dc"], raw["features_rest"], raw["opacity"], raw["scaling"],
                                                         raw["rotation"])
    lb = cam_leaves()
    out_b = R.GaussianRasterizer(settings(lb))(means3D=m3, means2D=m2, opacities=opacities, shs=shs, scales=scales,
                                               rotations=rotations)
    assert torch.equal(out[0], out_b[0])
    _backward(out_b, ups)
    ref = pc.reference(name)
    for k, a, b in zip(("viewmatrix", "projmatrix", "campos"), la, lb):
        d = np.abs(a.grad.double().cpu().numpy().reshape(-1) - b.grad.double().cpu().numpy().reshape(-1))
        assert b.grad.abs().max() > 0
        assert (d <= pr.BAR * ref.S[k]).all(), (k, d, ref.S[k])


class _Model:
    """what render() reads of the reference's GaussianModel"""

    def __init__(self, sc, dev, train_geometry):
        p = lambda t: t.to(dev).requires_grad_(train_geometry)
        self._xyz = p(sc.means3D)
        self._scaling = p(torch.log(sc.scales))
        self._rotation = p(sc.rotations)
        self._opacity = p(torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4)))
        self._features_dc = p(sc.shs[:, :1].contiguous())
        self._features_rest = p(sc.shs[:, 1:].contiguous())
        self._ins_feat = (sc.ins_feat.to(dev) * 2 - 1).requires_grad_(True)
        self.active_sh_degree = self.max_sh_degree = 3

    get_xyz = property(lambda s: s._xyz)
    get_scaling = property(lambda s: torch.exp(s._scaling))
    get_rotation = property(lambda s: torch.nn.functional.normalize(s._rotation))
    get_opacity = property(lambda s: torch.sigmoid(s._opacity))
    get_features = property(lambda s: torch.cat((s._features_dc, s._features_rest), dim=1))

    def get_ins_feat(self, origin=False):
        return torch.nn.functional.normalize(self._ins_feat, dim=1)


def test_render_trains_a_camera_pose_and_keeps_no_pass_of_it(gpu_device):
    from opengaussian_amd import rasterizer as R
    from opengaussian_amd.pose import CameraPose
    from opengaussian_amd.renderer import render
    dev = gpu_device
    c = pc.case("general_b")
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = torch.tensor(pc.BG, device=dev)
    gC = torch.tensor(c.gC, device=dev)

    def loss_of(out):
        return (out["render"] * gC).sum() + out["ins_feat"].sum() * 0.0

    # stage 0: everything trains, the pose with it.  Reference: the same call with a camera whose three tensors are leaves,
    # their gradients carried to the delta by torch
    cp = CameraPose(c.cam.to(dev))
    loss_of(render(cp, _Model(c.scene, dev, True), pipe, bg, 100, rescale=False)).backward()
    leaf = types.SimpleNamespace(
        image_height=c.H, image_width=c.W, FoVx=c.cam.FoVx, FoVy=c.cam.FoVy,
        world_view_transform=c.cam.world_view_transform.to(dev).requires_grad_(True),
        full_proj_transform=c.cam.full_proj_transform.to(dev).requires_grad_(True),
        camera_center=c.cam.camera_center.to(dev).requires_grad_(True))
    loss_of(render(leaf, _Model(c.scene, dev, True), pipe, bg, 100, rescale=False)).backward()
    want = pr.chain_to_delta(CameraPose(c.cam.to(dev)), leaf.world_view_transform.grad.cpu().numpy(),
                             leaf.full_proj_transform.grad.cpu().numpy(), leaf.camera_center.grad.cpu().numpy())
    assert float(want.abs().min()) > 0 and _close(cp.delta.grad, want), (cp.delta.grad, want)
    # stage >= 1: the model is frozen -- what the kept-pass cache lives on -- but the camera trains: every call is a full pass
    saved = R.KEPT_PASSES
    R.KEPT_PASSES = R.KeptPasses(budget_bytes=1 << 30)
    try:
        model = _Model(c.scene, dev, False)
        before = R.PASS_STATS["reblend"]
        grads = []
        for _ in range(2):
            cp.delta.grad = None
            loss_of(render(cp, model, pipe, bg, 40000, rescale=False)).backward()
            grads.append(cp.delta.grad.clone())
        assert R.PASS_STATS["reblend"] == before and R.KEPT_PASSES.stats["admitted"] == 0 and R.KEPT_PASSES.stats["hits"] == 0
        assert _close(grads[0], grads[1], 1e-6) and _close(grads[0], want, 1e-4)
        # the same model under a constant camera is kept as before
        constant = c.cam.to(dev)                  # one set of tensors: the key is made of their identities
        for _ in range(2):
            render(constant, model, pipe, bg, 40000, rescale=False)
        assert R.PASS_STATS["reblend"] == before + 1
    finally:
        R.KEPT_PASSES = saved


# ---- 7: the route a user had ----------------------------------------------------------------------------------------------------
def _quat_of_near_identity(Rm):
    w = torch.sqrt(1.0 + Rm[0, 0] + Rm[1, 1] + Rm[2, 2]) / 2
    return torch.stack([w, (Rm[2, 1] - Rm[1, 2]) / (4 * w), (Rm[0, 2] - Rm[2, 0]) / (4 * w), (Rm[1, 0] - Rm[0, 1]) / (4 * w)])


def _quat_mul(a, b):
    ar, ax, ay, az = a
    br, bx, by, bz = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return torch.stack([ar * br - ax * bx - ay * by - az * bz, ar * bx + ax * br + ay * bz - az * by,
                        ar * by - ax * bz + ay * br + az * bx, ar * bz + ax * by - ay * bx + az * br], dim=1)


def test_moving_the_camera_equals_moving_the_scene(gpu_device):
    """colors_precomp scene, delta = 0.  W2C = exp(delta) W2C_0 seen from the base camera is the scene moved by
    T = C2W_0 exp(delta) W2C_0: means T x, orientations R_T q -- P rigid transforms and quaternion products in torch, gradient back
    through [P, 3] and [P, 4].  The six numbers of the two routes agree within 2e-4 of the restatement's magnitude sums carried
    through the chain rule of the pose, sum over the entries of |d entry / d delta_k| S_entry."""
    from opengaussian_amd.pose import CameraPose, se3_exp
    dev = gpu_device
    name = "rgb_clamp"
    c = pc.case(name)
    ref = pc.reference(name)
    _, got = _run(name, dev)
    cp = CameraPose(c.cam.to(dev))
    g_pose = pr.chain_to_delta(cp, got["viewmatrix"], got["projmatrix"], got["campos"]).double().cpu().numpy()
    # the bound, in float64 on the host
    cpu = CameraPose(types.SimpleNamespace(world_view_transform=c.cam.world_view_transform.double(),
                                           full_proj_transform=c.cam.full_proj_transform.double(),
                                           camera_center=c.cam.camera_center.double()))
    J = torch.autograd.functional.jacobian(
        lambda d: torch.cat([(cpu._view0 + cpu._view0 @ (se3_exp(d).t() - torch.eye(4, dtype=d.dtype))).reshape(-1),
                             (cpu._full0 + cpu._view0 @ (se3_exp(d).t() - torch.eye(4, dtype=d.dtype)) @ cpu._proj).reshape(-1)]),
        torch.zeros(6, dtype=torch.float64)).numpy()
    bound = pr.BAR * (np.abs(J[:16]) * ref.S["viewmatrix"][:, None] + np.abs(J[16:]) * ref.S["projmatrix"][:, None]).sum(axis=0)
    # the moved scene through the existing backward
    delta = torch.zeros(6, device=dev, requires_grad=True)
    W2C = c.cam.world_view_transform.to(dev).t()
    from opengaussian_amd.pose import _mm
    T = _mm(_mm(torch.linalg.inv(W2C.double().cpu()).float().to(dev), se3_exp(delta)), W2C)
    t = lambda k: torch.tensor(c.inputs[k], device=dev)
    means = (t("means3D")[:, None, :] * T[:3, :3][None, :, :]).sum(2) + T[:3, 3][None]
    rots = _quat_mul(_quat_of_near_identity(T[:3, :3]), t("rotations"))
    from opengaussian_amd import rasterizer as R
    saved, R.TINY_MAX_P = R.TINY_MAX_P, 0
    try:
        out = R.GaussianRasterizer(helpers.settings_for(c.cam, pc.BG, 0, dev))(
            means3D=means, means2D=torch.zeros_like(means), opacities=t("opacities"), colors_precomp=t("colors_precomp"),
            scales=t("scales"), rotations=rots)
    finally:
        R.TINY_MAX_P = saved
    _backward(out, _upstream(c, dev))
    g_scene = delta.grad.double().cpu().numpy()
    print("delta gradient through the pose kernels:", g_pose, "through the moved scene:", g_scene, "bound:", bound)
    assert (np.abs(g_pose) > 0).all()
    assert (np.abs(g_pose - g_scene) <= bound).all(), (g_pose, g_scene, bound)


# ---- 8: descent ---------------------------------------------------------------------------------------------------------------
def test_one_step_against_the_gradient_lowers_the_loss(gpu_device):
    """photometric loss against the image of the true pose, from a pose off by 1 degree and 0.02 scene units"""
    from opengaussian_amd.pose import CameraPose
    dev = gpu_device
    c = pc.case("general_b")

    def image(cam, grad):
        out, _ = _facade(c, dev, cam, False)
        return out[0]

    with torch.no_grad():
        target = image(c.cam, False)
    axis = torch.tensor([0.5, -0.7, 0.5])
    off = torch.cat([axis / axis.norm() * np.deg2rad(1.0), torch.tensor([0.6, 0.0, -0.8]) * 0.02])
    cp = CameraPose(c.cam.to(dev), off)
    loss0 = ((image(cp, True) - target) ** 2).sum()
    loss0.backward()
    g = cp.delta.grad
    assert torch.isfinite(g).all() and float(g.norm()) > 0
    with torch.no_grad():
        cp.delta -= 1e-3 * g / g.norm()
        loss1 = ((image(cp, False) - target) ** 2).sum()
    print("descent: loss", float(loss0.detach()), "->", float(loss1))
    assert float(loss1) < float(loss0.detach())
