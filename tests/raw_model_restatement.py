"""Float64 restatement of the raw-model pass' activations and of their chain rule (include/ogs_model.h,
csrc/ogs_model_act.h), independent of the device code: NumPy for the formulas as the issue states them, torch for the
reference's own activation functions (scene/gaussian_model.py:52-61: torch.exp, torch.sigmoid, F.normalize; :151-155: cat).
tests/test_raw_model_host.py holds the two against each other; the GPU tests use both as the float64 reference."""
from __future__ import annotations

import numpy as np
import torch

EPS = 1e-12      # F.normalize's eps

FAMILIES = ("features_dc", "features_rest", "scaling", "rotation", "opacity")


def activate(features_dc, features_rest, opacity, scaling, rotation):
    """-> scales [P,3], rotations [P,4], opacities [P,1], shs [P,M,3] in float64 (features_rest None or [P,0,3]: M = 1)."""
    f64 = lambda a: np.asarray(a, np.float64)
    dc, s, q, o = f64(features_dc), f64(scaling), f64(rotation), f64(opacity).reshape(-1, 1)
    n = np.sqrt((q * q).sum(axis=1, keepdims=True))
    shs = dc if features_rest is None or np.asarray(features_rest).size == 0 else np.concatenate([dc, f64(features_rest)], axis=1)
    return np.exp(s), q / np.maximum(n, EPS), 1.0 / (1.0 + np.exp(-o)), shs


def chain_rule(scaling, rotation, opacity, g_scales=None, g_rotations=None, g_opacities=None, g_shs=None):
    """Gradients w.r.t. the activated arrays -> gradients w.r.t. the raw parameters (dict over FAMILIES; None in, None out)."""
    f64 = lambda a: np.asarray(a, np.float64)
    out = dict.fromkeys(FAMILIES)
    if g_scales is not None:
        out["scaling"] = f64(g_scales) * np.exp(f64(scaling))
    if g_opacities is not None:
        sig = 1.0 / (1.0 + np.exp(-f64(opacity).reshape(-1, 1)))
        out["opacity"] = f64(g_opacities).reshape(-1, 1) * (sig * (1.0 - sig))
    if g_rotations is not None:
        q, g = f64(rotation), f64(g_rotations)
        n = np.sqrt((q * q).sum(axis=1, keepdims=True))
        qh = q / np.maximum(n, EPS)
        with np.errstate(divide="ignore", invalid="ignore"):
            inside = (g - qh * (qh * g).sum(axis=1, keepdims=True)) / n
        out["rotation"] = np.where(n >= EPS, inside, g / EPS)
    if g_shs is not None:
        g = f64(g_shs)
        out["features_dc"], out["features_rest"] = g[:, :1], g[:, 1:]
    return out


def activate_torch(features_dc, features_rest, opacity, scaling, rotation):
    """The reference's getters, on torch tensors of any float dtype (autograd runs through them)."""
    shs = features_dc if features_rest is None or features_rest.numel() == 0 else torch.cat((features_dc, features_rest), dim=1)
    return torch.exp(scaling), torch.nn.functional.normalize(rotation), torch.sigmoid(opacity), shs


def chain_rule_autograd(scaling, rotation, opacity, g_scales, g_rotations, g_opacities, dtype=torch.float64):
    """The same three chain rules through torch autograd over activate_torch (float64 by default)."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    s, q, o = t(scaling).requires_grad_(True), t(rotation).requires_grad_(True), t(opacity).reshape(-1, 1).requires_grad_(True)
    dc = torch.zeros(s.shape[0], 1, 3, dtype=dtype)
    scales, rots, opac, _ = activate_torch(dc, None, o, s, q)
    gs, gq, go = torch.autograd.grad([scales, rots, opac], [s, q, o],
                                     [t(g_scales), t(g_rotations), t(g_opacities).reshape(-1, 1)])
    return {"scaling": gs.double().numpy(), "rotation": gq.double().numpy(), "opacity": go.double().numpy()}
