"""GPU: the per-Gaussian passes the ungrouped streaming path (P > 1024) no longer runs on their own.

  * the gradient-record clear: the forward blend zeroes OgsRasterFwdArgs.bwd_clear on its way and ogs_raster_backward, told so by
    OgsRasterBwdArgs.bwd_tmp_is_clear, skips its fill (tests 1 and 2);
  * the scan of tiles_touched: preprocess leaves one sum per 256-Gaussian workgroup, one small launch makes them offsets and
    num_rendered, duplicate scans its own 256 counts.  A full-binning pass keeps the scan over the P Gaussians, so
    helpers.hip_export_binning -- which holds the default pass' list against the full pass' one, entry by entry -- compares the
    two schemes with each other before the full list is compared with the oracle.

Bars: cleared ranges exactly zero and their guards untouched; gradients with the hosted clear bit-identical to those with the
backward's own fill; keys, point lists, ranges and num_rendered exact against oracle.raster_oracle."""
import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

GUARD = 4096
BG = (0.2, 0.1, 0.3)


def _render_with_clear(sc, cam, dev, stride):
    """One forward through the C ABI (the facade's own argument block and two-phase sequence) with bwd_clear pointing into the
    middle of a NaN-filled tensor; returns (cleared words, front guard, back guard, NaN bit pattern, num_rendered)."""
    from opengaussian_amd import _lib
    from opengaussian_amd import rasterizer as R
    P, W, H = sc.means3D.shape[0], cam.image_width, cam.image_height
    rs = helpers.settings_for(cam, BG, 3, dev)
    t = lambda x: x.to(dev).contiguous()
    m3, shs, opac, scl, rot = t(sc.means3D), t(sc.shs), t(sc.opacities), t(sc.scales), t(sc.rotations)
    out = (torch.empty(3, H, W, device=dev), torch.empty(1, H, W, device=dev), torch.empty(1, H, W, device=dev),
           torch.empty(P, dtype=torch.int32, device=dev))
    view, proj, campos = (R._f32c(x.to(dev)) for x in (rs.viewmatrix, rs.projmatrix, rs.campos))
    a = R._fwd_args(rs, P, 3, m3, shs, None, opac, scl, rot, None, rs.bg, view, proj, campos, *out, None, 1)
    nbytes = P * stride
    buf = torch.full(((2 * GUARD + nbytes) // 4,), float("nan"), dtype=torch.float32, device=dev)
    a.bwd_clear, a.bwd_clear_bytes = buf.data_ptr() + GUARD, nbytes
    keep = R._streaming_render(a, dev, _lib.lib(), False)
    torch.cuda.synchronize()
    words = buf.view(torch.int32)
    g = GUARD // 4
    nan_bits = int(torch.tensor(float("nan")).view(torch.int32))
    return words[g:g + nbytes // 4], words[:g], words[g + nbytes // 4:], nan_bits, keep[-1]


@pytest.mark.parametrize("P,W,H,stride", [(1025, 16, 16, 128), (1025, 48, 32, 128), (1025, 1920, 1080, 128),
                                          (1025, 1920, 1080, 64), (1300, 17, 17, 128)])
def test_forward_blend_clears_the_range_it_is_given_and_nothing_else(gpu_device, P, W, H, stride):
    """Workgroup b of the forward blend zeroes slice b of the range: one tile for the whole range, 6 tiles, nearly as many
    workgroups as 16-byte units (8160 / 8200), more workgroups than units (8160 / 4100: empty slices), partial tiles with mostly
    empty lists.  Both ways of sizing the render phase (blocking first pass, deferred second pass)."""
    from opengaussian_amd import rasterizer as R
    sc, cam = helpers.tiny_scene(P, W, H, 0.9 * max(W, H), seed=190 + P + W)
    R._LAST_NUM_RENDERED.pop((P, W, H, 1), None)
    st0 = dict(R.PASS_STATS)
    for sized in ("blocking", "deferred"):
        mid, front, back, nan_bits, D = _render_with_clear(sc, cam, gpu_device, stride)
        assert D > 0 and mid.numel() == P * stride // 4
        assert int((mid != 0).sum()) == 0, (sized, int((mid != 0).sum()))
        assert bool((front == nan_bits).all()) and bool((back == nan_bits).all()), sized
    assert R.PASS_STATS["blocking"] == st0["blocking"] + 1 and R.PASS_STATS["deferred"] == st0["deferred"] + 1


def test_camera_that_sees_nothing_clears_the_range_and_gives_zero_gradients(gpu_device):
    """num_rendered = 0: the blocking pass has no list to walk (stand-alone blend), the deferred pass walks empty lists; the range is
    zero after either, and a backward through autograd returns all-zero gradients."""
    from opengaussian_amd import rasterizer as R
    P, W, H = 1025, 48, 32
    sc, cam = helpers.tiny_scene(P, W, H, 40.0, seed=191)
    sc.means3D[:, 2] = -sc.means3D[:, 2].abs() - 1.0
    R._LAST_NUM_RENDERED.pop((P, W, H, 1), None)
    for sized in ("blocking", "deferred"):
        mid, front, back, nan_bits, D = _render_with_clear(sc, cam, gpu_device, 128)
        assert D == 0 and int((mid != 0).sum()) == 0, sized
        assert bool((front == nan_bits).all()) and bool((back == nan_bits).all()), sized
    inp = helpers.oracle_inputs(sc, cam, use_sh=True)
    for sized in ("deferred", "deferred"):
        junk = torch.full((P * 32,), float("nan"), device=gpu_device)      # what the allocator hands out next is not zero
        del junk
        (c, r, d, a), leaves = helpers.hip_forward(inp, cam, BG, 3, gpu_device, requires_grad=True)
        assert c.grad_fn.num_rendered == 0
        (c.sum() + a.sum()).backward()
        for k, v in leaves.items():
            if v is not None and v.grad is not None:
                assert float(v.grad.abs().max()) == 0.0, k


def _autograd_pass(sc, cam, dev, fused, hosted, backwards=1, seed=0):
    """forward + `backwards` backward calls through the facade; returns the list (one per backward) of gradient dicts"""
    from opengaussian_amd import rasterizer as R
    P, W, H = sc.means3D.shape[0], cam.image_width, cam.image_height
    rs = helpers.settings_for(cam, BG, 3, dev)
    leaf = lambda x: x.to(dev).clone().requires_grad_(True)
    L = dict(means3D=leaf(sc.means3D), means2D=torch.zeros(P, 3, device=dev, requires_grad=True), opacities=leaf(sc.opacities),
             shs=leaf(sc.shs), scales=leaf(sc.scales), rotations=leaf(sc.rotations))
    saved = R.HOST_BWD_CLEAR
    R.HOST_BWD_CLEAR = hosted
    try:
        if fused:
            L["feat"] = leaf(sc.ins_feat[:, :6])
            c, r, d, a = R.rasterize_fused(L["means3D"], L["means2D"], L["opacities"], L["shs"], L["feat"], rs, scales=L["scales"],
                                           rotations=L["rotations"])
        else:
            c, r, d, a = R.GaussianRasterizer(rs)(means3D=L["means3D"], means2D=L["means2D"], opacities=L["opacities"],
                                                  shs=L["shs"], scales=L["scales"], rotations=L["rotations"])
        assert (c.grad_fn.bwd_tmp is not None) == hosted
        g = torch.Generator().manual_seed(seed)
        gC, gA = torch.randn(c.shape, generator=g).to(dev), torch.randn(a.shape, generator=g).to(dev)
        res = []
        for i in range(backwards):
            for v in L.values():
                v.grad = None
            torch.autograd.backward([c, a], [gC, gA], retain_graph=i + 1 < backwards)
            res.append({k: v.grad.clone() for k, v in L.items()})
    finally:
        R.HOST_BWD_CLEAR = saved
    return res


@pytest.mark.parametrize("fused", [True, False], ids=["C9_fused", "C3"])
def test_gradients_with_the_hosted_clear_equal_those_with_the_backward_fill(gpu_device, fused):
    """Hosting on against hosting off (the pointer withheld: the fill at the start of ogs_raster_backward), P = 1500 at 64 x 48:
    every gradient tensor bit-identical; two backwards over a retained graph give the same gradients both times (the second
    finds the record dirty and clears it itself)."""
    sc, cam = helpers.tiny_scene(1500, 64, 48, 60.0, seed=192)
    dev = gpu_device
    on = _autograd_pass(sc, cam, dev, fused, hosted=True, backwards=2)
    off = _autograd_pass(sc, cam, dev, fused, hosted=False)
    assert float(on[0]["means3D"].abs().max()) > 0.0 and float(on[0]["shs"].abs().max()) > 0.0
    for k in on[0]:
        assert torch.equal(on[0][k], off[0][k]), k
        assert torch.equal(on[0][k], on[1][k]), k


def test_a_forward_without_backward_leaves_the_next_pass_unharmed(gpu_device):
    """A pass whose backward ran dirties its record and frees it; a forward whose backward never runs takes a record and drops it;
    the next pass of the same size is handed one of those blocks by the caching allocator and must clear it itself."""
    sc, cam = helpers.tiny_scene(1500, 64, 48, 60.0, seed=193)
    dev = gpu_device
    want = _autograd_pass(sc, cam, dev, False, hosted=False)[0]
    first = _autograd_pass(sc, cam, dev, False, hosted=True)[0]            # leaves a dirty block behind
    inp = helpers.oracle_inputs(sc, cam, use_sh=True)
    out, _ = helpers.hip_forward(inp, cam, BG, 3, dev, requires_grad=True)      # never back-propagated
    del out
    got = _autograd_pass(sc, cam, dev, False, hosted=True)[0]
    for k in want:
        assert torch.equal(first[k], want[k]) and torch.equal(got[k], want[k]), k


# ---- offsets from block sums ------------------------------------------------------------------------------------------------

def _binning_against_oracle(sc, cam, dev, W, H, f):
    from oracle import raster_oracle as ro
    inp = helpers.oracle_inputs(sc, cam, use_sh=True)
    g = ro.preprocess(inp["means3D"], inp["opacities"], inp["viewmatrix"], inp["projmatrix"], inp["campos"], W, H, W / (2 * f),
                      H / (2 * f), scales=inp["scales"], rotations=inp["rotations"], shs=inp["shs"], sh_degree=3)
    b = ro.bin_tiles(g, W, H)
    (color, radii, depth, alpha), _ = helpers.hip_forward(inp, cam, BG, 3, dev, requires_grad=True)
    assert color.grad_fn.num_rendered == b.num_rendered
    keys, ranges, ncontrib, plist = helpers.hip_export_binning(color)
    np.testing.assert_array_equal(radii.cpu().numpy(), g.radii)
    np.testing.assert_array_equal(keys, b.keys_sorted)
    np.testing.assert_array_equal(plist, b.point_list)
    np.testing.assert_array_equal(ranges, b.ranges)
    return g, b


@pytest.mark.parametrize("P", [1025, 1280, 1281, 2049])
def test_offsets_from_block_sums_give_the_oracle_binning(gpu_device, P):
    """one Gaussian past four workgroups, five whole workgroups, one past five, one past eight"""
    W, H, f = 64, 48, 60.0
    sc, cam = helpers.tiny_scene(P, W, H, f, seed=194 + P, with_ties=True)
    g, b = _binning_against_oracle(sc, cam, gpu_device, W, H, f)
    assert b.num_rendered > P // 2


def test_offsets_when_the_first_three_workgroups_are_culled(gpu_device):
    W, H, f, P = 64, 48, 60.0, 1281
    sc, cam = helpers.tiny_scene(P, W, H, f, seed=195)
    sc.means3D[:768, 2] = -1.0                                                 # behind the camera: block sums of zero
    g, b = _binning_against_oracle(sc, cam, gpu_device, W, H, f)
    assert int(g.radii[:768].max()) == 0 and int((g.radii[768:] > 0).sum()) > 100


def test_offsets_with_a_footprint_wider_than_255_tiles(gpu_device):
    """the per-thread loop of duplicate_kernel starts at an offset it only knows after the workgroup's scan"""
    W, H, f, P = 4400, 32, 70.0, 1100
    sc, cam = helpers.tiny_scene(P, W, H, f, seed=196)
    sc.means3D[600] = torch.tensor([0.0, 0.0, 3.0])
    sc.scales[600] = 40.0
    sc.opacities[600] = 0.02
    g, b = _binning_against_oracle(sc, cam, gpu_device, W, H, f)
    assert int(g.rect_max[600, 0] - g.rect_min[600, 0]) > 255


def test_deferred_second_pass_with_another_camera_agrees_with_the_blocking_path(gpu_device):
    """The hint path reads num_rendered on the device and sizes its buffers from the previous pass: same images, radii and count
    as a blocking pass over the same inputs."""
    from opengaussian_amd import rasterizer as R
    W, H, f, P = 96, 64, 80.0, 2049
    sc, cam = helpers.tiny_scene(P, W, H, f, seed=197)
    cam2 = helpers.general_camera(W, H, f, f, helpers.rotation_matrix((0.1, 1.0, 0.2), 0.15), (0.3, -0.2, 0.5))
    i1, i2 = helpers.oracle_inputs(sc, cam, use_sh=True), helpers.oracle_inputs(sc, cam2, use_sh=True)
    key = (P, W, H, 1)
    R._LAST_NUM_RENDERED.pop(key, None)
    st0 = dict(R.PASS_STATS)
    helpers.hip_forward(i1, cam, BG, 3, gpu_device)
    (cd, rd, dd, ad), _ = helpers.hip_forward(i2, cam2, BG, 3, gpu_device, requires_grad=True)
    assert R.PASS_STATS["deferred"] == st0["deferred"] + 1
    R._LAST_NUM_RENDERED.pop(key, None)
    (cb, rb, db, ab), _ = helpers.hip_forward(i2, cam2, BG, 3, gpu_device, requires_grad=True)
    assert R.PASS_STATS["blocking"] == st0["blocking"] + 2
    assert cd.grad_fn.num_rendered == cb.grad_fn.num_rendered > 0
    assert torch.equal(cd, cb) and torch.equal(rd, rb) and torch.equal(dd, db) and torch.equal(ad, ab)
    kd, kb = helpers.hip_export_binning(cd), helpers.hip_export_binning(cb)
    for x, y in zip(kd, kb):
        np.testing.assert_array_equal(x, y)

