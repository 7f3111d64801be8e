"""A camera whose pose trains: an se(3) delta on top of a base camera, differentiable through the rasterizer.

The rasterizer returns the gradient of a pass with respect to the three camera arrays as its kernels read them
(include/ogs_raster.h: dL_dviewmatrix, dL_dprojmatrix, dL_dcampos); everything here is a few 4 x 4 torch operations in front of
that, and torch's autograd does the chain rule.  Conventions are those of the reference's scene/cameras.py:71-78 -- transposed
storage, ``full_proj = world_view @ projection``, the centre from the inverse of ``world_view`` -- so a ``CameraPose`` goes
wherever a camera goes:

    cam = CameraPose(view)                                   # stage 0 with noisy poses, or locating an image in a frozen model
    opt = torch.optim.Adam(cam.parameters(), lr=1e-3)
    loss_of(render(cam, gaussians, pipe, background, iteration)).backward()
    opt.step()
"""
from __future__ import annotations

import weakref

import torch
from torch import nn

_SMALL_ANGLE2 = 1e-4     # theta^2 below which the series are used: their first omitted term is theta^6 / 5040 < 2e-16
_CONSTANTS: dict = {}


def _mm(a, b):
    """a @ b for the 3 x 3 and 4 x 4 matrices of a pose, as a broadcast product and a sum: no BLAS call, no library workspace
    allocated in the caller's process for sixty-four multiplies"""
    return (a[:, :, None] * b[None, :, :]).sum(1)


def _mv(a, v):
    return (a * v[None, :]).sum(1)


def _constants(dtype, device):
    """per (dtype, device): the generators of so(3) [3, 3, 3] (K = sum_i omega_i G_i is the cross-product matrix), the series
    coefficients of A, B, C in (1, theta^2, theta^4), eye(3) and the last row of a rigid transform.  Built once: a pose is a
    handful of tiny kernels on a path that is all launch overhead."""
    key = (dtype, str(device))
    hit = _CONSTANTS.get(key)
    if hit is None:
        G = torch.zeros(3, 3, 3, dtype=torch.float64)
        G[0, 2, 1], G[0, 1, 2] = 1.0, -1.0
        G[1, 0, 2], G[1, 2, 0] = 1.0, -1.0
        G[2, 1, 0], G[2, 0, 1] = 1.0, -1.0
        series = torch.tensor([[1.0, -1.0 / 6.0, 1.0 / 120.0], [0.5, -1.0 / 24.0, 1.0 / 720.0],
                               [1.0 / 6.0, -1.0 / 120.0, 1.0 / 5040.0]], dtype=torch.float64)
        to = lambda t: t.to(device=device, dtype=dtype)
        hit = (to(G), to(series), to(torch.eye(3, dtype=torch.float64)), to(torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)))
        _CONSTANTS[key] = hit
    return hit


def se3_exp(delta: torch.Tensor) -> torch.Tensor:
    """exp of the twist ``delta = (omega[3], u[3])`` as a [4, 4] rigid transform [[R, t], [0, 1]]: R = I + A K + B K^2
    (Rodrigues), t = V u with V = I + B K + C K^2 (K the cross-product matrix of omega, theta = |omega|, A = sin theta / theta,
    B = (1 - cos theta) / theta^2, C = (theta - sin theta) / theta^3; the three as power series in theta^2 near zero, so the
    map and its derivative are finite at delta = 0).  A zero delta gives the exact identity."""
    if delta.shape != (6,):
        raise RuntimeError(f"se3_exp takes a 6-vector (omega, u), got {tuple(delta.shape)}")
    G, series, eye, last_row = _constants(delta.dtype, delta.device)
    w, u = delta[:3], delta[3:]
    t2 = (w * w).sum()
    small = t2 < _SMALL_ANGLE2
    t2s = torch.where(small, 1.0, t2)              # the closed forms never see theta = 0 (nor does their gradient)
    th = torch.sqrt(t2s)
    sin = torch.sin(th)
    closed = torch.stack([sin / th, (1.0 - torch.cos(th)) / t2s, (th - sin) / (t2s * th)])
    coef = torch.where(small, _mv(series, torch.stack([torch.ones_like(t2), t2, t2 * t2])), closed)
    K = (w[:, None, None] * G).sum(0)
    BK, K2 = coef[1] * K, _mm(K, K)
    R = eye + coef[0] * K + coef[1] * K2
    t = u + _mv(BK + coef[2] * K2, u)
    return torch.cat([torch.cat([R, t[:, None]], dim=1), last_row], dim=0)


def _forget(ref):
    pose = ref()
    if pose is not None:
        pose.__dict__.pop("_cycle", None)


class CameraPose(nn.Module):
    """``base`` seen from a pose moved by the trainable twist ``delta``: W2C = exp(delta) @ W2C_base (the delta lives in the
    camera frame: omega in radians, u in scene units).  ``world_view_transform``, ``full_proj_transform`` and ``camera_center``
    are rebuilt from ``delta`` on every access and carry its graph; every other attribute is the base camera's.  With a zero
    delta the three tensors equal the base camera's bit for bit: each is the base tensor plus a term that is exactly zero.
    The three tensors of one call share the graph of one ``se3_exp``: back-propagate through them together, as a pass does."""

    def __init__(self, base, delta: torch.Tensor | None = None):
        super().__init__()
        self.__dict__["_base"] = base              # not registered: the reference's Camera is a Module of its own
        W0 = base.world_view_transform.detach()
        if tuple(W0.shape) != (4, 4) or tuple(base.full_proj_transform.shape) != (4, 4):
            raise RuntimeError("CameraPose: the base camera's world_view_transform / full_proj_transform must be [4, 4]")
        init = torch.zeros(6, dtype=W0.dtype, device=W0.device) if delta is None else \
            delta.detach().to(device=W0.device, dtype=W0.dtype).clone()
        if init.shape != (6,):
            raise RuntimeError(f"CameraPose: delta must be a 6-vector, got {tuple(init.shape)}")
        self.delta = nn.Parameter(init)
        F0 = base.full_proj_transform.detach()
        proj = getattr(base, "projection_matrix", None)      # scene/cameras.py:73 keeps it (transposed); else full = view @ P
        if isinstance(proj, torch.Tensor) and tuple(proj.shape) == (4, 4):
            proj = proj.detach().to(device=W0.device, dtype=W0.dtype)
        else:
            proj = torch.linalg.solve(W0.double().cpu(), F0.double().cpu()).to(device=W0.device, dtype=W0.dtype)
        # C2W = C2W_base @ exp(delta)^-1: the centre moves by (rotation block of C2W_base) @ (-R^T t); inverted once, in float64
        c2w_rot = torch.linalg.inv(W0.double().cpu())[:3, :3].t().to(device=W0.device, dtype=W0.dtype)
        self.register_buffer("_c2w_rot", c2w_rot.contiguous(), persistent=False)
        self.register_buffer("_view0", W0.clone(), persistent=False)
        self.register_buffer("_full0", F0.to(W0.device).clone(), persistent=False)
        self.register_buffer("_center0", base.camera_center.detach().to(W0.device).clone(), persistent=False)
        self.register_buffer("_proj", proj.clone(), persistent=False)
        self.register_buffer("_eye4", torch.eye(4, dtype=W0.dtype, device=W0.device), persistent=False)

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(self.__dict__["_base"], name)

    def _compute(self):
        # world_view = W2C^T = W2C_base^T @ exp(delta)^T = view0 + view0 @ (exp(delta)^T - I); full_proj = world_view @ P;
        # centre = row 3 of the inverse of world_view, in closed form for the rigid delta: exp(delta)^-1 = [R^T | -R^T t]
        E = se3_exp(self.delta)
        step = _mm(self._view0, E.t() - self._eye4)
        view = self._view0 + step
        full = self._full0 + _mm(step, self._proj)
        center = self._center0 + _mv(self._c2w_rot, -_mv(E[:3, :3].t(), E[:3, 3]))
        if E.requires_grad:
            # the three share the graph of E: once a backward has run through it, nothing of this evaluation is handed out again
            ref = weakref.ref(self)
            E.register_hook(lambda g: _forget(ref))
        return view, full, center

    def _tensor(self, i) -> torch.Tensor:
        """Tensor i of (world_view, full_proj, centre).  One evaluation serves each of the three once -- render() reads each once
        per call, and an evaluation is ~40 tiny kernels forward and as many backward on a path that is all launch overhead --
        as long as delta and the grad mode are what they were and no backward has gone through it."""
        key = (self.delta._version, self.delta.data_ptr(), torch.is_grad_enabled())
        cyc = self.__dict__.get("_cycle")
        if cyc is None or cyc[0] != key or cyc[2][i]:
            cyc = self.__dict__["_cycle"] = [key, self._compute(), [False, False, False]]
        cyc[2][i] = True
        return cyc[1][i]

    @property
    def world_view_transform(self) -> torch.Tensor:
        return self._tensor(0)

    @property
    def full_proj_transform(self) -> torch.Tensor:
        return self._tensor(1)

    @property
    def camera_center(self) -> torch.Tensor:
        return self._tensor(2)

    def pose_matrix(self) -> torch.Tensor:
        """the current W2C [4, 4] (detached)"""
        return self.world_view_transform.detach().t().contiguous()
