"""CPU: the raw-model pass' chain rule restated in float64 equals torch autograd through the reference's activation functions;
render()'s eligibility rule for the raw pass over stand-in models; rasterize_model refuses CPU tensors; the new header's
symbols are declared in _lib.py."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import raw_model_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _raw_rows(P=64, seed=3):
    g = np.random.default_rng(seed)
    scaling = g.normal(-3.0, 1.0, (P, 3))
    q = g.standard_normal((P, 4))
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * g.uniform(0.3, 3.0, (P, 1))
    opacity = g.normal(0.0, 3.0, (P, 1))
    # the edges: |q| = 0, 1e-13 (below eps), exactly eps-ish from above; saturated logits
    q[0] = 0.0
    q[1] = np.array([0.6, 0.0, -0.8, 0.0]) * 1e-13
    q[2] = np.array([0.0, 1.0, 0.0, 0.0]) * 2e-12
    opacity[3], opacity[4] = 40.0, -40.0
    opacity[5], opacity[6] = 800.0, -800.0
    return scaling, q, opacity


def test_chain_rule_equals_autograd_through_reference_activations():
    scaling, q, opacity = _raw_rows()
    g = np.random.default_rng(11)
    gs, gq, go = g.standard_normal(scaling.shape), g.standard_normal(q.shape), g.standard_normal(opacity.shape)
    want = rr.chain_rule_autograd(scaling, q, opacity, gs, gq, go)
    got = rr.chain_rule(scaling, q, opacity, gs, gq, go)
    for k in ("scaling", "rotation", "opacity"):
        scale = np.abs(want[k]).max(axis=1, keepdims=True) + 1e-300
        assert (np.abs(got[k] - want[k]) / scale).max() < 1e-12, k
    # the clamp_min branch: g / eps, no projection; saturated sigmoids: an exact zero
    np.testing.assert_allclose(got["rotation"][:2], gq[:2] / 1e-12, rtol=1e-15)
    assert np.all(got["opacity"][5:7] == 0.0) and np.all(want["opacity"][5:7] == 0.0)
    assert abs(got["opacity"][3, 0]) < 1e-16 and abs(got["opacity"][4, 0]) < 1e-16


def test_activations_equal_reference_functions():
    scaling, q, opacity = _raw_rows()
    g = np.random.default_rng(5)
    dc, rest = g.standard_normal((64, 1, 3)), g.standard_normal((64, 8, 3))
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    want = rr.activate_torch(t(dc), t(rest), t(opacity), t(scaling), t(q))
    got = rr.activate(dc, rest, opacity, scaling, q)
    for a, b in zip(got, want):
        np.testing.assert_allclose(a, b.numpy(), rtol=1e-14, atol=0)
    assert rr.activate(dc, None, opacity, scaling, q)[3].shape == (64, 1, 3)
    sh_grads = rr.chain_rule(scaling, q, opacity, g_shs=got[3])
    assert np.array_equal(sh_grads["features_dc"], dc) and np.array_equal(sh_grads["features_rest"], rest)


class _Model:
    """stand-in for the reference's GaussianModel: the attributes render()'s eligibility rule looks at"""

    def __init__(self, device="meta", drop=None, own_xyz=True):
        mk = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)
        self._xyz, self._scaling, self._rotation, self._opacity = mk(5, 3), mk(5, 3), mk(5, 4), mk(5, 1)
        self._features_dc, self._features_rest = mk(5, 1, 3), mk(5, 15, 3)
        if drop:
            delattr(self, drop)
        self.get_xyz = self._xyz if own_xyz else mk(5, 3)


def _pipe(**kw):
    return types.SimpleNamespace(**{**dict(debug=False, compute_cov3D_python=False, convert_SHs_python=False), **kw})


def test_render_eligibility_rule():
    from opengaussian_amd.renderer import _raw_model_params
    cpu = _Model("cpu")
    # the switch is opt-in: the reference's PipelineParams has no such attribute
    assert _raw_model_params(cpu, _pipe(), cpu.get_xyz, None) is None
    assert _raw_model_params(cpu, _pipe(raw_model_pass=False), cpu.get_xyz, None) is None
    # CPU tensors never take it
    assert _raw_model_params(cpu, _pipe(raw_model_pass=True), cpu.get_xyz, None) is None

    class _Cuda(torch.Tensor):      # a CPU tensor that says it lives on the GPU: the rule is host logic
        is_cuda = True

    def on_gpu(m):
        for n in ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest"):
            if hasattr(m, n):
                own = getattr(m, n) is m.get_xyz
                setattr(m, n, getattr(m, n).as_subclass(_Cuda))
                if own:
                    m.get_xyz = getattr(m, n)
        return m

    on = _pipe(raw_model_pass=True)
    m = on_gpu(_Model("cpu"))
    got = _raw_model_params(m, on, m.get_xyz, None)
    assert got is not None and set(got) == {"_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest"}
    assert _raw_model_params(m, on, m.get_xyz, torch.zeros(5, 3)) is None                      # override_color
    for flag in ("debug", "compute_cov3D_python", "convert_SHs_python"):
        assert _raw_model_params(m, _pipe(raw_model_pass=True, **{flag: True}), m.get_xyz, None) is None, flag
    for name in ("_scaling", "_features_rest", "_opacity"):
        md = on_gpu(_Model("cpu", drop=name))
        assert _raw_model_params(md, on, md.get_xyz, None) is None, name                       # missing attribute
    other = on_gpu(_Model("cpu", own_xyz=False))
    assert _raw_model_params(other, on, other.get_xyz, None) is None                           # get_xyz is not _xyz
    half = on_gpu(_Model("cpu"))
    half._scaling = half._scaling.double().as_subclass(_Cuda)
    assert _raw_model_params(half, on, half.get_xyz, None) is None                             # not fp32


def test_rasterize_model_refuses_cpu_tensors():
    from opengaussian_amd.rasterizer import activate_model, rasterize_model
    from tests import helpers
    sc, cam = helpers.tiny_scene(16, 32, 32, 30.0)
    rs = helpers.settings_for(cam, (0, 0, 0), 3, "cpu")
    args = (sc.shs[:, :1].contiguous(), sc.shs[:, 1:].contiguous(), sc.opacities, torch.log(sc.scales), sc.rotations)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rasterize_model(sc.means3D, torch.zeros(16, 3), *args, rs)
    with pytest.raises(RuntimeError, match="no CPU path"):
        activate_model(*args)


def test_model_header_symbols_are_bound():
    from opengaussian_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ogs_model.h")).read()
    names = set(re.findall(r"^\s*int\s+(ogs_[a-z0-9_]+)\s*\(", hdr, re.M))
    assert names == {"ogs_raster_forward_geometry_raw", "ogs_raster_forward_tiny_raw", "ogs_raster_backward_raw",
                     "ogs_model_activate"}
    for n in names:
        assert n in _lib.SIGNATURES, n
    for cls, cname in ((_lib.OgsRawModel, "OgsRawModel"), (_lib.OgsRawModelGrads, "OgsRawModelGrads")):
        body = hdr.split(f"typedef struct {cname} {{")[1].split(f"}} {cname};")[0]
        fields = re.findall(r"float\*\s+([a-z_]+);", body)
        assert fields == [f[0] for f in cls._fields_], cname
