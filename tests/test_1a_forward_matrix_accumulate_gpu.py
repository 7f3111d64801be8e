"""GPU: (1) the self-test of the forward walk's accumulation as a matrix instruction; (2) regression tests of the chunked forward
kernel as it is, on a scene that reaches every path of its walk.

(1) The step of pack_blend_chunked_kernel adds w x (features, depth, 1) into the pixel's sums; per 4x4 block that is a rank-one
product, which one 4-block K = 1 fp32 MFMA computes (csrc/blend_fwd.hip: rank1_update).  A kernel built on it was bit-identical and
slower, so NO kernel uses it; ogs_selftest_mfma_rank1 keeps the finding checkable: a chain of N such MFMA
updates equals, bit for bit, the same chain as fmaf per element (random data, cancelling sums, denormal products and sums, w = 0
against finite features, a negative-zero accumulator), and the A / B / accumulator lane layout is the one written down beside
rank1_update.

(2) The scene, kept-pass and statistics tests run the kernels the library ships (one fmaf per channel), none of the code in (1):
  * a full pass equals the re-blend of its own kept pass (torch.equal) and the oracle's blend, n_contrib exact, for C = 3, 6, 9, 12
    on a 40 x 24 scene with a two-chunk tile, a two-sub-chunk quadrant, a short block list, pixels that saturate mid-list and an
    empty tile.  Oracle bars are the project's existing ones (test_10, test_12, test_17): colour and alpha 1e-4; depth 1e-3 with
    flip_tol 4e-2, because depth sums carry the view depth (2..6 here) where colour sums carry values below 1;
  * the statistics variant of the same kernel gives what the images give, at test_15's bars."""
import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

W, H, F = 40, 24, 40.0          # 3 x 2 tiles: the right column is 8 pixels wide, the bottom row 8 high; 40 % 16 = 8, 24 % 16 = 8
BG12 = (0.25, -0.5, 0.75, 0.1, 0.6, -0.2, 0.3, 0.9, -0.7, 0.45, 0.05, -0.35)


# ---- the instruction against fmaf ------------------------------------------------------------------------------------------
def _rank1(w, f, acc0, dev):
    from opengaussian_amd import _lib
    n = w.shape[0]
    wd, fd, ad = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev) for x in (w, f, acc0))
    out_m = torch.full((4, 16, 16), float("nan"), device=dev)
    out_f = torch.full((4, 16, 16), float("nan"), device=dev)
    _lib.check(_lib.lib().ogs_selftest_mfma_rank1(wd.data_ptr(), fd.data_ptr(), ad.data_ptr(), n, out_m.data_ptr(),
                                                  out_f.data_ptr(), 0), "selftest")
    torch.cuda.synchronize()
    return out_m.cpu().numpy(), out_f.cpu().numpy()


def _chains(n, rng):
    """name -> (w [n,64], f [n,64], acc0 [4,16,16]) fp32"""
    f32 = np.float32
    tiny = f32(2.0 ** -126)                                    # smallest normal
    cases = {}
    cases["random"] = (rng.random((n, 64)), rng.standard_normal((n, 64)) * 3, rng.standard_normal((4, 16, 16)))
    # cancelling sums: step 2k+1 takes back what step 2k added, with features of 24 significant bits
    w = rng.random((n, 64)).astype(f32)
    f = (rng.standard_normal((n, 64)) * 1000).astype(f32)
    w[1::2] = w[0:2 * (n // 2):2]
    f[1::2] = -f[0:2 * (n // 2):2]
    cases["cancelling"] = (w, f, rng.standard_normal((4, 16, 16)) * 1e-3)
    # denormal products (w * f below 2^-126) onto denormal and tiny-normal sums
    wd = (rng.random((n, 64)) * 2.0 ** -70).astype(f32)
    fd = ((rng.random((n, 64)) - 0.5) * 2.0 ** -60).astype(f32)
    cases["denormal"] = (wd, fd, (rng.standard_normal((4, 16, 16)) * 3).astype(f32) * tiny)
    cases["denormal_inputs"] = (np.full((n, 64), tiny / 4, f32), rng.standard_normal((n, 64)) * 2.0 ** 20,
                                np.zeros((4, 16, 16)))
    # w = 0 (idle, stopped, dummy and skipped lanes) against finite features of both signs, some of them huge
    fz = rng.standard_normal((n, 64)) * 1e30
    wz = rng.random((n, 64))
    wz[:, ::2] = 0.0
    wz[n // 2] = 0.0
    cases["zero_weight"] = (wz, fz, rng.standard_normal((4, 16, 16)))
    # -0.0 accumulators: +0 products must turn them into +0, -0 products must not
    wn = np.zeros((n, 64))
    wn[:, 16:32] = rng.random((n, 16)) * (np.arange(n)[:, None] >= n - 1)       # block 1 adds something in the last step
    fn = np.where(rng.random((n, 64)) < 0.5, -1.0, 1.0) * rng.random((n, 64))
    cases["negative_zero"] = (wn, fn, np.full((4, 16, 16), -0.0))
    return {k: tuple(np.ascontiguousarray(x, f32) for x in v) for k, v in cases.items()}


@pytest.mark.parametrize("steps", [1, 5, 300])
def test_mfma_chain_equals_the_fmaf_chain_bit_for_bit(gpu_device, steps):
    rng = np.random.default_rng(steps)
    for name, (w, f, acc0) in _chains(steps, rng).items():
        got_m, got_f = _rank1(w, f, acc0, gpu_device)
        assert not np.isnan(got_f).any() and not np.isnan(got_m).any(), name
        diff = got_m.view(np.uint32) != got_f.view(np.uint32)
        assert not diff.any(), (f"{name}, {steps} steps: {int(diff.sum())} of 1024 elements differ, first at "
                                f"{tuple(np.argwhere(diff)[0])}: mfma {got_m[diff][0]!r} fmaf {got_f[diff][0]!r}")
    # negative zero survives a chain of +0 * (-f) = -0 additions only; checked against the host's arithmetic for one step
    w = np.zeros((1, 64), np.float32)
    f = np.tile(np.where(np.arange(16) % 2 == 0, -2.0, 2.0).astype(np.float32), 4)[None]
    got_m, _ = _rank1(w, f, np.full((4, 16, 16), -0.0, np.float32), gpu_device)
    want = np.float32(-0.0) + np.float32(0.0) * f[0, :16]              # -0 + -0 = -0, -0 + +0 = +0
    assert np.array_equal(np.signbit(got_m), np.broadcast_to(np.signbit(want), (4, 16, 16)))


def test_mfma_lane_layout(gpu_device):
    """Exact small integers, asymmetric in block, pixel and channel: acc[b][i][j] = (16 b + i + 1) * (1000 + 64 b + 3 j), one step
    from a distinct start value per element -- a swapped A / B, a transposed accumulator or a wrong block would all show."""
    lane = np.arange(64)
    w = (lane + 1).astype(np.float32)[None]
    f = (1000 + 64 * (lane // 16) + 3 * (lane % 16)).astype(np.float32)[None]
    acc0 = np.arange(1024, dtype=np.float32).reshape(4, 16, 16) * 0.5
    b, i, j = np.meshgrid(np.arange(4), np.arange(16), np.arange(16), indexing="ij")
    want = acc0 + (16 * b + i + 1) * (1000 + 64 * b + 3 * j)
    got_m, got_f = _rank1(w, f, acc0, gpu_device)
    assert np.array_equal(got_f, want.astype(np.float32))
    assert np.array_equal(got_m, want.astype(np.float32))


# ---- the kernel on a scene that reaches every path of the walk ------------------------------------------------------------
def _place(n, x0, x1, y0, y1, sigma, op0, op1, g):
    """n Gaussians whose centres project into the pixel box [x0, x1] x [y0, y1], footprint ~sigma pixels, opacity in [op0, op1]"""
    z = torch.rand(n, generator=g) * 4.0 + 2.0
    px = torch.rand(n, generator=g) * (x1 - x0) + x0
    py = torch.rand(n, generator=g) * (y1 - y0) + y0
    means = torch.stack([(px - W / 2 + 0.5) * z / F, (py - H / 2 + 0.5) * z / F, z], dim=1)
    scales = (sigma * z / F)[:, None] * (0.7 + 0.6 * torch.rand(n, 3, generator=g))
    opac = torch.rand(n, 1, generator=g) * (op1 - op0) + op0
    return means, scales, opac


def _scene():
    from opengaussian_amd.synthetic import Scene, make_camera
    g = torch.Generator().manual_seed(1234)
    parts = [
        _place(300, 1.0, 14.0, 1.0, 14.0, 5.0, 0.005, 0.008, g),     # tile 0: > 256 faint entries, no pixel saturates: two chunks
        _place(110, 16.3, 18.6, 0.3, 7.2, 0.45, 0.03, 0.08, g),       # tile 1, top-left quadrant: > 64, on its left blocks only
        _place(140, 1.0, 14.0, 17.0, 22.5, 2.5, 0.85, 0.99, g),      # tile 3: opaque, pixels saturate a few entries in
        _place(50, 18.0, 28.0, 18.0, 22.0, 0.8, 0.2, 0.9, g),        # tile 4
        _place(100, 33.5, 38.0, 1.0, 9.0, 0.9, 0.05, 0.9, g),        # tile 2 (8 pixels wide); tile 5 stays empty
    ]
    means, scales, opac = (torch.cat([p[k] for p in parts]).contiguous() for k in range(3))
    P = means.shape[0]
    q = torch.randn(P, 4, generator=g)
    feat = torch.rand(P, 12, generator=g) * 2.0 - 0.5
    sc = Scene(means, scales, (q / q.norm(dim=1, keepdim=True)).contiguous(), opac, torch.zeros(P, 16, 3), feat.contiguous())
    return sc, make_camera(W, H, F, F)


@pytest.fixture(scope="module")
def ref():
    """the scene and the oracle's pass over it, once: 12 channels, the narrower passes are its leading channels"""
    from oracle import raster_oracle as ro
    sc, cam = _scene()
    inp = helpers.oracle_inputs(sc, cam, feat=sc.ins_feat)
    out = ro.render_forward(W=W, H=H, tanfovx=W / (2 * F), tanfovy=H / (2 * F), bg=np.array(BG12, np.float32), sh_degree=3, **inp)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sc, cam, out


def _pixel_reach(geom):
    """[P, H, W] bool in float64: Gaussian p gives pixel (y, x) alpha >= 1/255"""
    xy, con, op = geom.xy.astype(np.float64), geom.conic.astype(np.float64), geom.opacity.astype(np.float64)
    dx = xy[:, 0, None, None] - np.arange(W)[None, None, :]
    dy = xy[:, 1, None, None] - np.arange(H)[None, :, None]
    power = -0.5 * (con[:, 0, None, None] * dx * dx + con[:, 2, None, None] * dy * dy) - con[:, 1, None, None] * dx * dy
    return (power <= 0) & (op[:, None, None] * np.exp(np.minimum(power, 0)) >= 1 / 255.0) & (geom.radii[:, None, None] > 0)


def test_scene_reaches_every_path(ref):
    sc, cam, out = ref
    reach = _pixel_reach(out["geom"])
    per_block = lambda x, y, s: int(reach[:, y:y + s, x:x + s].any(axis=(1, 2)).sum())
    assert 650 <= sc.means3D.shape[0] <= 750
    assert per_block(0, 0, 16) > 256                                   # two chunks
    assert per_block(16, 0, 8) > 64                                    # two sub-chunks of a quadrant
    assert 4 * per_block(20, 0, 4) < per_block(16, 0, 4) and 4 * per_block(20, 4, 4) < per_block(16, 4, 4)   # a short block list
    assert per_block(32, 16, 8) == 0                                   # an empty tile
    n = out["n_contrib"]
    assert n[:16, :16].max() > 256                                     # the second chunk of tile 0 contributes
    # the stop path: in tile 3 pixels end on different entries, well before the tile's list does
    ranges = out["binning"].ranges
    assert 0 < n[16:, :16].max() < ranges[3, 1] - ranges[3, 0] and len(np.unique(n[16:, :16])) > 8
    assert float(out["alpha"][0, 16:, :16].max()) > 0.999 and float(out["alpha"][0, :8, :16].max()) < 0.99


def _direct_pass(sc, cam, Cn, dev, full):
    """an ungrouped pass through the library's two-phase forward, no autograd: images, radii and the exported binning"""
    from opengaussian_amd import _lib
    from opengaussian_amd import rasterizer as R
    rs = helpers.settings_for(cam, BG12[:Cn], 3, dev)
    t = lambda x: x.to(dev).contiguous()
    P = sc.means3D.shape[0]
    e = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float32, device=dev)
    color, depth, alpha, radii = e(Cn, H, W), e(1, H, W), e(1, H, W), torch.zeros(P, dtype=torch.int32, device=dev)
    keep = (t(sc.means3D), t(sc.ins_feat[:, :Cn]), t(sc.opacities), t(sc.scales), t(sc.rotations), rs.bg, rs.viewmatrix,
            rs.projmatrix, rs.campos)
    m3, cols, opac, scl, rot, bg, view, proj, campos = keep

    def run():
        a = R._fwd_args(rs, P, Cn, m3, None, cols, opac, scl, rot, None, bg, view, proj, campos, color, depth, alpha, radii, None, 1)
        bufs = R._streaming_render(a, dev, _lib.lib(), False)
        return helpers._export_binning_of(a, bufs[5], bufs[2], W, H, dev)

    if full:
        with R.full_binning():
            keys, ranges, ncontrib, raw = run()
    else:
        keys, ranges, ncontrib, raw = run()
    return color, depth, alpha, radii, ranges, ncontrib


def _kept_pair(sc, cam, Cn, dev):
    """(full pass that is admitted to the cache, its re-blend) through the facade, features only"""
    from opengaussian_amd import rasterizer as R
    saved, R.KEPT_PASSES = R.KEPT_PASSES, R.KeptPasses(budget_bytes=1 << 30)
    try:
        rs = helpers.settings_for(cam, BG12[:Cn], 3, dev)
        t = lambda x: x.to(dev).contiguous()
        args = (t(sc.means3D), torch.zeros(sc.means3D.shape[0], 3, device=dev), t(sc.opacities), None, t(sc.ins_feat[:, :Cn]), rs)
        kw = dict(scales=t(sc.scales), rotations=t(sc.rotations), detach_extra_from_geometry=False,
                  frozen_key=("cam", ("v", Cn), None))
        before = R.PASS_STATS["reblend"]
        with torch.no_grad():
            full = R.rasterize_fused(*args, **kw)
            assert R.KEPT_PASSES.stats["admitted"] == 1 and R.PASS_STATS["reblend"] == before
            again = R.rasterize_fused(*args, **kw)
            assert R.PASS_STATS["reblend"] == before + 1
        return full, again
    finally:
        R.KEPT_PASSES = saved


@pytest.mark.parametrize("Cn", [3, 6, 9, 12])
def test_full_pass_equals_its_reblend_and_the_oracle(gpu_device, ref, Cn):
    sc, cam, out = ref
    dev = gpu_device
    full, again = _kept_pair(sc, cam, Cn, dev)
    for a, b, what in zip(full, again, ("color", "radii", "depth", "alpha")):
        assert torch.equal(a, b), f"C={Cn}: {what} of the chunked pass != the re-blend of its kept streams"
    color, depth, alpha, radii, ranges, _ = _direct_pass(sc, cam, Cn, dev, full=False)
    for a, b, what in zip(full, (color, radii, depth, alpha), ("color", "radii", "depth", "alpha")):
        assert torch.equal(a, b), f"C={Cn}: {what} differs between the facade and the direct pass"
    lens = ranges[:, 1].astype(np.int64) - ranges[:, 0]
    assert lens[0] > 256 and lens[5] == 0, lens                         # tile 0's CULLED list spans two chunks; tile 5 is empty
    np.testing.assert_array_equal(radii.cpu().numpy(), out["geom"].radii)
    helpers.assert_close_modulo_threshold_flips(color.cpu().numpy(), out["color"][:Cn], 1e-4)
    helpers.assert_close_modulo_threshold_flips(alpha.cpu().numpy(), out["alpha"], 1e-4)
    helpers.assert_close_modulo_threshold_flips(depth.cpu().numpy(), out["depth"], 1e-3, flip_tol=4e-2)
    # n_contrib in the reference's convention (position in the tile's full list): the same pass over the full lists
    fcolor, fdepth, falpha, fradii, _, ncontrib = _direct_pass(sc, cam, Cn, dev, full=True)
    assert torch.equal(fcolor, color) and torch.equal(fdepth, depth) and torch.equal(falpha, alpha) and torch.equal(fradii, radii)
    np.testing.assert_array_equal(ncontrib, out["n_contrib"].astype(np.uint32))


@pytest.mark.parametrize("Cn", [3, 6, 9, 12])
def test_statistics_variant_matches_the_images(gpu_device, ref, Cn):
    """ogs_raster_forward_group_stats on the same scene at test_15's bars: exact counts and maximum alpha, feature sums within
    1e-5 relative + 1e-6 of a float64 sum over the images, the same bits on a second run."""
    from opengaussian_amd.rasterizer import rasterize_group_stats
    sc, cam, _ = ref
    dev = gpu_device
    rs = helpers.settings_for(cam, BG12[:Cn], 3, dev)
    t = lambda x: x.to(dev).contiguous()
    color, depth, alpha, radii_img, _, _ = _direct_pass(sc, cam, Cn, dev, full=False)
    L = 7
    labels = torch.randint(-1, L, (H, W), generator=torch.Generator().manual_seed(5), dtype=torch.int32).to(dev)
    ids = torch.zeros(sc.means3D.shape[0], dtype=torch.int32, device=dev)
    col = color.double().cpu().numpy()
    a = alpha[0].double().cpu().numpy()
    lab = labels.cpu().numpy()
    bucket = np.where((lab >= 0) & (lab < L), lab, L)
    for thr in (0.0, 0.8, 0.999):
        with torch.no_grad():
            run = lambda: rasterize_group_stats(t(sc.means3D), t(sc.opacities), ids, 1, labels, L, rs, t(sc.ins_feat[:, :Cn]),
                                                scales=t(sc.scales), rotations=t(sc.rotations), alpha_threshold=thr)
            max_alpha, count, fsum, radii = run()
            again = run()
        sel = a > thr
        want_count = np.bincount(bucket[sel], minlength=L + 1)
        want = np.stack([np.bincount(bucket[sel], weights=col[c][sel], minlength=L + 1) for c in range(Cn)], axis=1)
        assert np.array_equal(count.cpu().numpy()[0], want_count), thr
        assert torch.equal(max_alpha.cpu().view(torch.int32), alpha.amax().reshape(1).cpu().view(torch.int32)), thr
        err = np.abs(fsum.double().cpu().numpy()[0] - want) - 1e-5 * np.abs(want)
        assert err.max() <= 1e-6, f"C={Cn} thr={thr}: feat_sum off by {err.max()}"
        assert torch.equal(radii, radii_img)
        for x, y in zip((max_alpha, count, fsum), again):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                               y.view(torch.int32) if y.dtype == torch.float32 else y), f"C={Cn} thr={thr}: run to run"
