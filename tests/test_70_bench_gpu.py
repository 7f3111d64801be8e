"""GPU: a plain bench.py run (no --full) prints the headline alone, and --dump-outputs writes what its last timed step
computed -- checked against the same view rendered in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(gpu_device, tmp_path):
    from opengaussian_amd.rasterizer import rasterize_fused
    from opengaussian_amd.synthetic import make_scene, orbit_camera
    from tests import helpers
    steps, warmup = 3, 1
    out_dir = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "C2-100k-800", "--steps", str(steps),
           "--warmup", str(warmup), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    res = json.loads(lines[0])
    assert res["unit"] == "Mpix/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["steps"] == steps and res["value"] > 0 and res["ms_per_step"] > 0
    assert abs(res["value"] - 800 * 800 / (res["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * res["value"]
    assert not {"roofline", "kernels_ms_per_step", "kmeans", "stage1_pass", "frozen_rgb_call", "cpu_baseline",
                "extras"} & set(res), sorted(res)

    names = {"color", "depth", "alpha", "radii", "grad_means2D", "grad_means3D", "grad_scales", "grad_rotations",
             "grad_opacities", "grad_shs", "grad_ins_feat"}
    files = {f[:-4]: out_dir / f for f in os.listdir(out_dir)}
    assert set(files) == names
    assert sum(os.path.getsize(f) for f in files.values()) <= 64 << 20
    got = {k: np.load(f) for k, f in files.items()}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())

    # the last timed step rendered view (warmup + steps - 1) mod 8 of the seeded scene: re-render it here
    P, W, H, f = 100_000, 800, 800, 700.0
    sc = make_scene(P, W, H, f, f, seed=0).to(gpu_device)
    cam = orbit_camera(W, H, f, f, view_index=(warmup + steps - 1) % 8, num_views=8)
    leaves = {k: getattr(sc, k).clone().requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs",
                                                                     "ins_feat")}
    color, radii, depth, alpha = rasterize_fused(leaves["means3D"], torch.zeros(P, 3, device=gpu_device, requires_grad=True),
                                                 leaves["opacities"], leaves["shs"], leaves["ins_feat"],
                                                 helpers.settings_for(cam, (0.0, 0.0, 0.0), 3, gpu_device),
                                                 scales=leaves["scales"], rotations=leaves["rotations"])
    np.testing.assert_array_equal(got["radii"], radii.cpu().numpy().astype(np.float32))
    np.testing.assert_allclose(got["alpha"], alpha.detach().cpu().numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(got["depth"], depth.detach().cpu().numpy(), rtol=1e-6, atol=1e-6)
    assert got["color"].ndim == 1 and got["color"].size < color.numel()             # a fixed sample of the 9-channel image
    assert np.abs(got["grad_opacities"]).max() > 0
