"""Reference for the camera gradients of a pass (include/ogs_raster.h: dL_dviewmatrix, dL_dprojmatrix, dL_dcampos).

The float64 graph of the gradient oracle -- ``oracle.raster_oracle.preprocess_t`` + ``blend`` over a FIXED fp32 binning, as
``render_backward_f64`` builds it -- with the three camera arrays replaced by PER-GAUSSIAN COPIES as leaves: view [16, n],
projection [16, n], campos [n, 3].  ``preprocess_t`` only calls ``.reshape(16)`` on the matrices and indexes the result, and
``eval_sh_rgb_t`` only does ``campos[None, :]``, so two small stand-ins are enough and the oracle is used as it stands.

The gradient rows are then the per-Gaussian contributions c_g; their sum over g is the reference, and ``S = sum_g |c_g|`` per
entry is the scale every bar refers to: fp32 terms summed in fp64 can promise an error relative to the magnitude sum, not to a
total that cancels to a few 1e-3 of it.  In a ``colors_precomp`` pass autograd reports campos as unused: exact zeros.

The blend's skip decisions (alpha >= 1/255, T < 1e-4) are re-taken by ``blend`` in the dtype of the evaluation and are
constants of the gradient; ``dtype=torch.float32`` evaluates the same graph in fp32, as ``render_backward_f64`` offers.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

# entries of the two matrices a pass reads (storage order): the x, y, z rows of p_view; the hx, hy, hw rows
VIEW_READ = tuple(k for k in range(16) if k % 4 != 3)
PROJ_READ = tuple(k for k in range(16) if k % 4 != 2)
BAR = 2e-4          # the project's gradient bar (helpers.assert_grad_family_close), applied to the magnitude sum S


class _PerGaussianMatrix:
    """what preprocess_t sees as a camera matrix: ``.reshape(16)[k]`` is the [n] vector of entry k, one value per Gaussian"""

    def __init__(self, rows):
        self.rows = rows            # [16, n]

    def reshape(self, *shape):
        return self

    def __getitem__(self, k):
        return self.rows[k]


class _PerGaussianCampos:
    """what eval_sh_rgb_t sees as campos: ``campos[None, :]`` is the [n, 3] array of centres, one per Gaussian"""

    def __init__(self, rows):
        self.rows = rows            # [n, 3]

    def __getitem__(self, key):
        return self.rows


@dataclass
class PoseReference:
    used: np.ndarray            # [n] indices of the Gaussians that appear in a tile list
    contrib: dict               # "viewmatrix" [n, 16], "projmatrix" [n, 16], "campos" [n, 3]: c_g, float64
    total: dict                 # the same keys: sum over g
    S: dict                     # the same keys: sum over g of |c_g|
    means3D: np.ndarray         # [P, 3] dL/dmeans3D of the same graph (rows outside `used` zero)
    loss: float


class Restatement:
    """One pass: inputs (dict of numpy arrays as helpers.oracle_inputs builds them), the fp32 binning held fixed, the upstream
    gradients.  dL_ddepth / dL_dalpha may be None (zeros)."""

    def __init__(self, inputs, binning, W, H, tanfovx, tanfovy, bg, dL_dcolor, dL_ddepth=None, dL_dalpha=None,
                 scale_modifier=1.0, sh_degree=0):
        from oracle import raster_oracle as ro
        self.ro = ro
        self.inputs, self.W, self.H = inputs, int(W), int(H)
        self.tanfovx, self.tanfovy = float(tanfovx), float(tanfovy)
        self.bg, self.scale_modifier, self.sh_degree = np.asarray(bg, np.float64), float(scale_modifier), int(sh_degree)
        self.ups = (np.asarray(dL_dcolor, np.float64),
                    None if dL_ddepth is None else np.asarray(dL_ddepth, np.float64),
                    None if dL_dalpha is None else np.asarray(dL_dalpha, np.float64))
        P = np.asarray(inputs["means3D"]).shape[0]
        self.P = P
        # only the Gaussians of a tile list receive gradient; the graph is restricted to them (render_backward_f64 does the same)
        self.used = np.unique(np.asarray(binning.point_list).astype(np.int64))
        remap = np.full(P, -1, dtype=np.int64)
        remap[self.used] = np.arange(len(self.used))
        self.binning = ro.Binning(binning.num_rendered, binning.keys_sorted,
                                  remap[np.asarray(binning.point_list).astype(np.int64)], binning.ranges, binning.offsets)

    def camera_rows(self, dtype=torch.float64):
        """(view [16, n], projection [16, n], campos [n, 3]): the shared camera copied to every Gaussian"""
        n = len(self.used)
        t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
        V = t(self.inputs["viewmatrix"]).reshape(16, 1).expand(16, n).clone()
        M = t(self.inputs["projmatrix"]).reshape(16, 1).expand(16, n).clone()
        Cp = t(self.inputs["campos"]).reshape(1, 3).expand(n, 3).clone()
        return V, M, Cp

    def loss(self, V, M, Cp, dtype=torch.float64, means3D=None):
        """the pass' scalar loss as a function of per-Gaussian camera rows (and, optionally, of the means [n, 3])"""
        ro = self.ro
        t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
        sub = lambda k: None if self.inputs.get(k) is None else t(np.asarray(self.inputs[k])[self.used])
        m3 = sub("means3D") if means3D is None else means3D
        n = m3.shape[0]
        xy, conic, op, rgb, depth = ro.preprocess_t(
            m3, torch.zeros(n, 3, dtype=dtype), sub("opacities"), _PerGaussianMatrix(V), _PerGaussianMatrix(M),
            _PerGaussianCampos(Cp), self.W, self.H, self.tanfovx, self.tanfovy, sub("scales"), sub("rotations"),
            sub("cov3D_precomp"), sub("shs"), sub("colors_precomp"), self.scale_modifier, self.sh_degree)
        color, dmap, amap, _ = ro.blend(xy, conic, op, rgb, depth, self.binning.ranges, self.binning.point_list, self.W,
                                        self.H, t(self.bg))
        gC, gD, gA = self.ups
        out = (color * t(gC)).sum()
        if gD is not None:
            out = out + (dmap * t(gD)).sum()
        if gA is not None:
            out = out + (amap * t(gA)).sum()
        return out

    def reference(self, dtype=torch.float64) -> PoseReference:
        V, M, Cp = self.camera_rows(dtype)
        n = len(self.used)
        zero = PoseReference(self.used, {"viewmatrix": np.zeros((n, 16)), "projmatrix": np.zeros((n, 16)),
                                         "campos": np.zeros((n, 3))}, {}, {}, np.zeros((self.P, 3)), 0.0)
        if n:
            m3 = torch.tensor(np.asarray(self.inputs["means3D"])[self.used], dtype=dtype, requires_grad=True)
            for x in (V, M, Cp):
                x.requires_grad_(True)
            L = self.loss(V, M, Cp, dtype, m3)
            gV, gM, gC, gm = torch.autograd.grad(L, [V, M, Cp, m3], allow_unused=True)
            f = lambda g, shape: np.zeros(shape) if g is None else g.double().numpy()
            zero.contrib = {"viewmatrix": f(gV, (16, n)).T.copy(), "projmatrix": f(gM, (16, n)).T.copy(),
                            "campos": f(gC, (n, 3))}
            zero.means3D[self.used] = f(gm, (n, 3))
            zero.loss = float(L.detach())
        zero.total = {k: v.sum(axis=0) for k, v in zero.contrib.items()}
        zero.S = {k: np.abs(v).sum(axis=0) for k, v in zero.contrib.items()}
        return zero


def translation_identity(V, M, dV, dM, dC, dmeans):
    """Both sides of  sum_g dL/dmean_g[j] = sum_i V[4j+i] dL/dV[12+i] + sum_i M[4j+i] dL/dM[12+i] - dL/dcampos[j]  in float64,
    and the scale  sum_g |dL/dmean_g[j]|  per axis j: moving every mean by d is moving the two translations by W d and the
    centre by -d.  Returns (lhs [3], rhs [3], scale [3])."""
    V, M = np.asarray(V, np.float64).reshape(16), np.asarray(M, np.float64).reshape(16)
    dV, dM, dC = (np.asarray(a, np.float64).reshape(-1) for a in (dV, dM, dC))
    dmeans = np.asarray(dmeans, np.float64).reshape(-1, 3)
    lhs = dmeans.sum(axis=0)
    rhs = np.array([sum(V[4 * j + i] * dV[12 + i] for i in range(4)) + sum(M[4 * j + i] * dM[12 + i] for i in range(4)) - dC[j]
                    for j in range(3)])
    return lhs, rhs, np.abs(dmeans).sum(axis=0)


def chain_to_delta(pose_module, dV, dM, dC):
    """dL/d(delta) of a pose.CameraPose from the 35 partials: torch's chain rule through the module's three tensors, in the
    module's own dtype.  Returns a [6] tensor on the module's device."""
    outs = (pose_module.world_view_transform, pose_module.full_proj_transform, pose_module.camera_center)
    gs = [torch.as_tensor(np.asarray(g), dtype=o.dtype).reshape(o.shape).to(o.device) for g, o in zip((dV, dM, dC), outs)]
    return torch.autograd.grad(outs, [pose_module.delta], gs)[0]
