"""CPU: the reference of the camera-gradient tests, the conditions its cases must meet, and opengaussian_amd/pose.py.

  * the restatement (tests/pose_grad_restatement.py) against central differences of the float64 forward graph with the binning
    held fixed, on three entries of each array;
  * the case conditions of tests/pose_grad_cases.py, asserted so that a case cannot go soft: the fp32 evaluation of the graph is
    within 1e-5 S of the float64 one (no threshold flip decides a case), every entry a pass reads has S > 0, the clamp cases hold
    clamped Gaussians with non-zero contributions, and the translation identity holds in the restatement to 1e-9;
  * pose.se3_exp against helpers.rotation_matrix, the zero delta, the conventions against synthetic.make_camera;
  * the facade's argument plumbing around a stand-in for the autograd function, and its host-side errors.
"""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import pose_grad_cases as pc
from tests import pose_grad_restatement as pr


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["general", "rgb_clamp"])
def test_restatement_against_central_differences(name):
    c = pc.case(name)
    ref = pc.reference(name)
    rs = c.restatement()
    h = 1e-6
    picks = {"viewmatrix": (1, 6, 14), "projmatrix": (0, 7, 13), "campos": (0, 1, 2)}
    for arr, entries in picks.items():
        if c.spec.beyond_clamp and arr != "campos":
            # where the clamp is active the gradient is by definition NOT the derivative of the forward graph (the clamped
            # branch is detached): differences of the forward say nothing about those entries
            continue
        for k in entries:
            vals = []
            for sgn in (1.0, -1.0):
                V, M, Cp = rs.camera_rows()
                if arr == "viewmatrix":
                    V[k] += sgn * h
                elif arr == "projmatrix":
                    M[k] += sgn * h
                else:
                    Cp[:, k] += sgn * h
                with torch.no_grad():
                    vals.append(float(rs.loss(V, M, Cp)))
            fd = (vals[0] - vals[1]) / (2 * h)
            S = ref.S[arr][k]
            if arr == "campos" and not c.spec.sh:
                assert fd == 0.0 and ref.total[arr][k] == 0.0 and S == 0.0       # unused: exact zeros
                continue
            # truncation ~ h^2, and the rounding of two losses of size |L| divided by 2 h: |L| * 1e-16 / 1e-6
            assert abs(fd - ref.total[arr][k]) <= 1e-6 * S + 1e-9 * abs(ref.loss), (arr, k, fd, ref.total[arr][k], S)


def test_never_read_entries_have_no_gradient():
    ref = pc.reference("general")
    assert not ref.contrib["viewmatrix"][:, [3, 7, 11, 15]].any()
    assert not ref.contrib["projmatrix"][:, [2, 6, 10, 14]].any()


# ---- the cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.PARITY_CASES)
def test_case_conditions(name):
    c = pc.case(name)
    ref, ref32 = pc.reference(name), pc.reference(name, fp32=True)
    assert len(ref.used) > 0
    readable = {"viewmatrix": list(pr.VIEW_READ), "projmatrix": list(pr.PROJ_READ), "campos": [0, 1, 2] if c.spec.sh else []}
    fractions = {}
    for k, idx in readable.items():
        S = ref.S[k][idx]
        assert (S > 0).all(), f"{name}: {k} entries {np.array(idx)[S == 0]} receive nothing"
        frac = np.abs(ref32.total[k][idx] - ref.total[k][idx]) / S
        fractions[k] = (float(frac.max()) if len(idx) else 0.0, float((np.abs(ref.total[k][idx]) / S).min()) if len(idx) else 1.0)
        assert (frac <= 1e-5).all(), f"{name}: {k}: the fp32 evaluation leaves the float64 one by {frac.max():.2e} S"
    print(f"{name}: fp32 vs float64 as a fraction of S, and the worst cancellation total / S:", fractions)
    if not c.spec.sh:
        assert not ref.contrib["campos"].any()
    # the translation identity in float64
    lhs, rhs, scale = pr.translation_identity(c.inputs["viewmatrix"], c.inputs["projmatrix"], ref.total["viewmatrix"],
                                              ref.total["projmatrix"], ref.total["campos"], ref.means3D)
    assert (np.abs(lhs - rhs) <= 1e-9 * scale).all(), (name, lhs, rhs, scale)
    if c.spec.visible_first:
        # the last row (the edge the P = 255 / 256 / 257 cases are about) contributes to every array
        assert ref.used[-1] == c.spec.P - 1
        assert all(np.abs(ref.contrib[k][-1]).max() > 1e-6 * ref.S[k].max() for k in ("viewmatrix", "projmatrix", "campos")), name
    if name in pc.CLAMP_CASES:
        rows = pc.clamped_rows(c)
        pos = np.searchsorted(ref.used, rows)
        assert len(rows) >= 10 and (ref.used[pos] == rows).all()
        live = np.abs(ref.contrib["viewmatrix"][pos]).max(axis=1) > 0
        assert live.sum() >= 10, f"{name}: {int(live.sum())} clamped Gaussians with a non-zero contribution"


# ---- pose.py -----------------------------------------------------------------------------------------------------------------
def test_se3_exp_against_rodrigues():
    from opengaussian_amd.pose import se3_exp
    g = torch.Generator().manual_seed(11)
    for scale in (1.0, 1e-1, 5e-3, 1e-5):
        d = (torch.rand(6, generator=g, dtype=torch.float64) * 2 - 1) * scale
        E = se3_exp(d).numpy()
        w = d[:3].numpy()
        th = np.linalg.norm(w)
        assert np.abs(E[:3, :3] - helpers.rotation_matrix(w, th)).max() < 1e-14
        K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        Vm = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * (K @ K)
        assert np.abs(E[:3, 3] - Vm @ d[3:].numpy()).max() < 1e-12 * max(scale, 1e-3) + 1e-16
        assert (E[3] == np.array([0.0, 0.0, 0.0, 1.0])).all()
    assert torch.equal(se3_exp(torch.zeros(6)), torch.eye(4))
    # differentiable at zero and across the series threshold: the Jacobian at 0 is the generator basis
    J = torch.autograd.functional.jacobian(se3_exp, torch.zeros(6, dtype=torch.float64))
    assert torch.isfinite(J).all()
    assert J[2, 1, 0] == 1.0 and J[1, 2, 0] == -1.0 and J[0, 3, 3] == 1.0 and J[1, 3, 4] == 1.0 and J[2, 3, 5] == 1.0
    for th in (0.9e-2, 1.1e-2):                                  # either side of theta^2 = 1e-4
        d = torch.tensor([th, 0.0, 0.0, 0.1, 0.2, 0.3], dtype=torch.float64)
        Jn = torch.autograd.functional.jacobian(se3_exp, d)
        fd = (se3_exp(d + torch.eye(6, dtype=torch.float64)[1] * 1e-7) - se3_exp(d - torch.eye(6, dtype=torch.float64)[1] * 1e-7)) / 2e-7
        assert (Jn[:, :, 1] - fd).abs().max() < 1e-8
    with pytest.raises(RuntimeError):
        se3_exp(torch.zeros(7))


@pytest.mark.parametrize("pose", ["general", "quarter_y", "general_b"])
def test_camera_pose_zero_delta_and_conventions(pose):
    from opengaussian_amd.pose import CameraPose, se3_exp
    from opengaussian_amd.synthetic import make_camera
    W, H, fx, fy = pc.SMALL
    R, t = helpers.POSES[pose]
    base = helpers.general_camera(W, H, fx, fy, R, t)
    cp = CameraPose(base)
    assert [n for n, _ in cp.named_parameters()] == ["delta"] and cp.delta.shape == (6,)
    assert torch.equal(cp.world_view_transform, base.world_view_transform)
    assert torch.equal(cp.full_proj_transform, base.full_proj_transform)
    assert torch.equal(cp.camera_center, base.camera_center)
    assert cp.world_view_transform.requires_grad and cp.full_proj_transform.requires_grad and cp.camera_center.requires_grad
    assert cp.image_width == W and cp.image_height == H and cp.FoVx == base.FoVx and cp.FoVy == base.FoVy
    # a non-zero delta: W2C = exp(delta) @ W2C_base, and the three tensors are those make_camera builds for that W2C
    d = torch.tensor([0.21, -0.13, 0.08, 0.3, -0.2, 0.15])
    moved = CameraPose(base, d)
    w2c = se3_exp(d.double()) @ base.world_view_transform.double().t()
    want = make_camera(W, H, fx, fy, R=w2c[:3, :3].float(), t=w2c[:3, 3].float())
    assert (moved.world_view_transform - want.world_view_transform).abs().max() < 2e-6
    assert (moved.full_proj_transform - want.full_proj_transform).abs().max() < 2e-6 * want.full_proj_transform.abs().max()
    assert (moved.camera_center - want.camera_center).abs().max() < 5e-6
    assert torch.equal(moved.pose_matrix(), moved.world_view_transform.detach().t())
    with pytest.raises(RuntimeError):
        CameraPose(base, torch.zeros(5))


# ---- the facade around a stand-in -----------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def apply(self, *args):
        self.calls.append(args)
        return "out"


def test_facade_passes_camera_tensors_only_when_they_train(monkeypatch):
    from opengaussian_amd import rasterizer as R
    W, H, fx, fy = pc.SMALL
    cam = helpers.general_camera(W, H, fx, fy, *helpers.POSES["general"])
    rs = helpers.settings_for(cam, pc.BG, 3, "cpu")
    m = torch.zeros(4, 3)
    rec, rec_model = _Recorder(), _Recorder()
    monkeypatch.setattr(R, "_RasterizeGaussians", rec)
    monkeypatch.setattr(R, "_RasterizeModel", rec_model)
    e = torch.Tensor([])
    # a constant camera: the calls are the ones made before cameras could train, argument for argument
    R.rasterize_gaussians(m, m, e, m, m, m, m, e, rs)
    R.rasterize_fused(m, m, m, m, m, rs, scales=m, rotations=m)
    R.rasterize_model(m, m, m, m, m, m, m, rs)
    assert [len(a) for a in rec.calls] == [11, 11] and len(rec_model.calls[0]) == 10
    # a camera tensor that requires grad: the three tensors of the settings follow as the trailing inputs
    view = rs.viewmatrix.clone().requires_grad_(True)
    rs_t = rs._replace(viewmatrix=view)
    R.rasterize_gaussians(m, m, e, m, m, m, m, e, rs_t)
    R.rasterize_fused(m, m, m, m, m, rs_t, scales=m, rotations=m, frozen_key=("slot", "key", None))
    R.rasterize_model(m, m, m, m, m, m, m, rs_t)
    for a in rec.calls[2:]:
        assert len(a) == 18 and a[15] is view and a[16] is rs.projmatrix and a[17] is rs.campos
        assert a[11:15] == (None, 1, None, False)
    a = rec_model.calls[1]
    assert len(a) == 13 and a[10] is view and a[11] is rs.projmatrix and a[12] is rs.campos
    # ... and not under no_grad
    with torch.no_grad():
        R.rasterize_gaussians(m, m, e, m, m, m, m, e, rs_t)
    assert len(rec.calls[-1]) == 11


def test_facade_host_side_errors_and_record_size():
    from opengaussian_amd import rasterizer as R
    W, H, fx, fy = pc.SMALL
    cam = helpers.general_camera(W, H, fx, fy, *helpers.POSES["general"])
    rs = helpers.settings_for(cam, pc.BG, 3, "cpu")
    view = rs.viewmatrix.clone().requires_grad_(True)
    m = torch.zeros(4, 3)
    e = torch.Tensor([])
    # grouped passes are out of scope: refused before anything touches a device
    with pytest.raises(RuntimeError, match="grouped"):
        R._RasterizeGaussians.apply(m, m, e, m, m, m, m, e, rs, 0, None, torch.zeros(4, dtype=torch.int32), 2, None, False,
                                    view, rs.projmatrix, rs.campos)
    # there is no CPU path, with or without a camera that trains
    with pytest.raises(RuntimeError, match="GPU"):
        R._RasterizeGaussians.apply(m, m, e, m, m, m, m, e, rs, 0, None, None, 1, None, False, view, rs.projmatrix, rs.campos)
    # a pass whose only trainable inputs are the camera tensors needs the full record
    none = (False,) * 8
    assert R._grad_record_bytes(none, 10, 9, None, m, None, None, None, pose=True) == 10 * 128
    feat_only = (False, False, False, True, False, False, False, False)
    assert R._grad_record_bytes(feat_only, 10, 6, None, m, None, None, None) == 10 * 64
    assert R._grad_record_bytes(feat_only, 10, 6, None, m, None, None, None, pose=True) == 10 * 128


def test_struct_carries_the_pose_fields_last():
    from opengaussian_amd import _lib
    names = [f[0] for f in _lib.OgsRasterBwdArgs._fields_]
    assert names[-4:] == ["dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos", "pose_tmp"]
    assert names[-5] == "bwd_tmp_is_clear"
    assert "ogs_raster_backward_pose_tmp_bytes" in _lib.SIGNATURES and "ogs_pose_partial_chunk" in _lib.SIGNATURES
