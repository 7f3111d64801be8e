"""GPU: the per-tile depth sort of the render phase (binning.hip::tile_depth_sort_kernel) against the oracle's binning.

Ungrouped streaming passes (P > 1024) no longer sort the P Gaussians by depth: duplicate emits the pairs in Gaussian-index
order, the stable tile sort leaves each tile's list in id order, and one workgroup per tile sorts its list by (depth key, id).
Lists up to ogs_raster_tile_sort_capacity(0) entries are sorted by one wave, up to ogs_raster_tile_sort_capacity(1) by a
workgroup in LDS, longer ones by passes through global memory.  The
reference order (oracle.raster_oracle.bin_tiles: stable argsort of tile << 32 | depth bits over pairs emitted in id order)
must come out bit for bit, in the default (culled) binning mode and in full-binning mode (helpers.hip_export_binning checks
the culled list against the full one and returns the full one).

  * one tile of 40 000 entries (the global-memory path, several chunks, 20 000 pairs of equal depths); in the full list its
    edge neighbours get 5 000 - 7 600 entries (global-memory path, two chunks) and its corner neighbours 650 - 1 450 (LDS);
  * list lengths 1 and 2 (the early exits), around the one-wave limit (capacity level 0) and the LDS limit (level 1), and
    LDS limit + 1 entries of ONE depth (no digit differs: the list stays in id order), each in a scene whose other Gaussians are culled (behind the camera):
    they pass through the index-order scan and duplicate with zero tiles.

Bars: radii, sorted keys, point list and tile ranges bit-exact; images at the suite's IMG_TOL."""
import numpy as np
import pytest
import torch

from opengaussian_amd.synthetic import make_camera, make_scene
from tests import helpers
from tests.test_10_raster_gpu import IMG_TOL

pytestmark = pytest.mark.gpu

W, H, F = 64, 48, 60.0
TILE_11 = 1 * ((W + 15) // 16) + 1          # tile (1, 1)


def _tile_scene(n_vis, n_culled, px_lo, px_hi, seed, equal_depth=False):
    """n_vis Gaussians whose pixel centres fall in [px_lo, px_hi)^2 (identity camera, f = F), opacity 0.3, z = 2 + 6 U with
    z[1::2] = z[0::2] (equal_depth: one z for all), plus n_culled Gaussians behind the camera at random indices."""
    P = n_vis + n_culled
    sc = make_scene(P, W, H, F, F, seed=seed, log_scale_mean=-6.0, log_scale_std=0.3)
    g = torch.Generator().manual_seed(1000 + seed)
    z = 2.0 + 6.0 * torch.rand(n_vis, generator=g)
    z[1::2] = z[0::2][: z[1::2].shape[0]]
    if equal_depth:
        z[:] = z[0]
    px = px_lo + (px_hi - px_lo) * torch.rand(n_vis, generator=g)
    py = px_lo + (px_hi - px_lo) * torch.rand(n_vis, generator=g)
    # pixel centre = f x / z + (W - 1) / 2 for the identity camera
    vis_means = torch.stack([(px - (W - 1) / 2) * z / F, (py - (H - 1) / 2) * z / F, z], dim=1)
    means = torch.empty(P, 3)
    culled = torch.randperm(P, generator=g)[:n_culled]
    is_vis = torch.ones(P, dtype=torch.bool)
    is_vis[culled] = False
    means[is_vis] = vis_means
    means[~is_vis] = torch.tensor([0.0, 0.0, -1.0])
    sc.means3D = means.contiguous()
    sc.opacities[:] = 0.3
    return sc, make_camera(W, H, F, F)


def _check_against_oracle(sc, cam, dev):
    from oracle import raster_oracle as ro
    inp = helpers.oracle_inputs(sc, cam, use_sh=True)
    bg = (0.2, 0.1, 0.3)
    ref = ro.render_forward(W=W, H=H, tanfovx=W / (2 * F), tanfovy=H / (2 * F), bg=np.array(bg, np.float32), sh_degree=3,
                            **inp)
    (color, radii, depth, alpha), _ = helpers.hip_forward(inp, cam, bg, 3, dev, requires_grad=True)
    keys, ranges, ncontrib, plist = helpers.hip_export_binning(color)
    np.testing.assert_array_equal(radii.cpu().numpy(), ref["geom"].radii)
    assert len(keys) == ref["binning"].num_rendered
    np.testing.assert_array_equal(keys, ref["binning"].keys_sorted)
    np.testing.assert_array_equal(plist, ref["binning"].point_list)
    np.testing.assert_array_equal(ranges, ref["binning"].ranges)
    helpers.assert_close_modulo_threshold_flips(color.detach().cpu().numpy(), ref["color"], IMG_TOL)
    helpers.assert_close_modulo_threshold_flips(alpha.detach().cpu().numpy(), ref["alpha"], IMG_TOL)
    return ref, ranges


def _capacity(level=1):
    """level 0: longest list one wave sorts alone; 1: longest list a workgroup sorts in LDS"""
    from opengaussian_amd import _lib
    return int(_lib.lib().ogs_raster_tile_sort_capacity(level))


def test_one_tile_with_40000_entries(gpu_device):
    n = 40_000
    sc, cam = _tile_scene(n, 0, 16.0, 32.0, seed=18)
    ref, ranges = _check_against_oracle(sc, cam, gpu_device)
    assert int((ref["geom"].radii > 0).sum()) == n
    lens = (ranges[:, 1] - ranges[:, 0]).astype(np.int64)
    assert lens[TILE_11] == n and n > 2 * _capacity(), (lens[TILE_11], _capacity())
    # the long list really holds equal-depth neighbours ordered by id
    r0, r1 = ranges[TILE_11]
    d = ref["geom"].depth[ref["binning"].point_list[r0:r1]]
    assert int((np.diff(d) == 0).sum()) > 10_000
    # neighbours on both paths (full list)
    cap = _capacity()
    assert int((lens > cap).sum()) >= 3 and int(((lens > 256) & (lens <= cap)).sum()) >= 2, lens


@pytest.mark.parametrize("case", ["1", "2", "wave-1", "wave", "wave+1", "cap-1", "cap", "cap+1", "cap+1_one_depth"])
def test_list_length_boundaries(gpu_device, case):
    cap, wave = _capacity(1), _capacity(0)
    n = {"1": 1, "2": 2, "wave-1": wave - 1, "wave": wave, "wave+1": wave + 1, "cap-1": cap - 1, "cap": cap, "cap+1": cap + 1,
         "cap+1_one_depth": cap + 1}[case]
    # centres in [20, 28)^2 px with radius 2: every Gaussian touches tile (1, 1) alone, the list has exactly n entries
    sc, cam = _tile_scene(n, 1500, 20.0, 28.0, seed=n, equal_depth=case.endswith("one_depth"))
    ref, ranges = _check_against_oracle(sc, cam, gpu_device)
    lens = (ranges[:, 1] - ranges[:, 0]).astype(np.int64)
    assert lens[TILE_11] == n and int(lens.sum()) == n, lens
    assert int((ref["geom"].radii > 0).sum()) == n
