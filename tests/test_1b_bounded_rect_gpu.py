"""The tile rect duplicate_kernel expands is the reference rect cut down to the bounding box of the reach ellipse
(csrc/preprocess_fwd.hip, preprocess_one "8b"; DESIGN.md "Round 9").

The cut is only allowed to remove (Gaussian, tile) pairs the box test of duplicate_kernel would have dropped anyway, so everything
after the first pass of the tile sort -- lists, ranges, images, gradients -- and the reported num_rendered stay what they were.
helpers.hip_export_binning holds a default pass' list against the full-binning pass' list (reference rects, every pair tested)
filtered by the reach flag, entry by entry: a pair the cut lost but the test keeps shows up there.  Each GPU case below therefore
proves containment on its scene; the CPU case proves it for the numpy restatement of the two sides on a wider population.

Bars: keys, point lists, ranges, radii and num_rendered exact against oracle.raster_oracle; images and gradients of the default
pass bit-identical to those of `rasterizer.full_binning()`; emitted pairs <= num_rendered, and on the opacity scene <= a float64
cap the reference rects alone do not meet."""
import contextlib

import numpy as np
import pytest
import torch

from tests import bounded_rect_restatement as br
from tests import helpers

BG = (0.2, 0.1, 0.3)
K_THR_MARGIN = 0.01


def test_bound_contains_box_test_cpu():
    """numpy fp32 restatement of both sides: no tile of a reference rect passes the box test outside the emitted rect.  Ordinary
    blobs, needles of ratio 1e2..1e4 centred within 1.5 px of tile corners, needles of ratio up to 1e5 far off screen (their fp32
    determinant rounds to the wrong sign in a few per mille: no ellipse, the reference rect stays), huge off-screen blobs, and
    slivers of ratio up to 1e6; opacities uniform, near 1, within 5e-6 of the threshold opacity exp(-kThrMargin) / 255 and up to
    50 x above it."""
    rng = np.random.default_rng(11)
    W, H, N = 320, 240, 8000
    F = np.float32

    def opacities(n):
        c, u = rng.integers(0, 4, n), rng.uniform(0, 1, n)
        edge = np.exp(-K_THR_MARGIN) / 255
        return np.where(c == 0, u, np.where(c == 1, 0.99 + 0.01 * u,
                                            np.where(c == 2, edge * (1 + (u - 0.5) * 1e-5), edge * 50 ** u))).astype(F)

    uni = lambda lo, hi: rng.uniform(lo, hi, N).astype(F)
    corner = lambda n_tiles: (rng.integers(0, n_tiles + 1, N) * 16 - 0.5 + rng.uniform(-1.5, 1.5, N)).astype(F)
    cases = {
        "ordinary": (uni(-40, W + 40), uni(-40, H + 40), br.random_cov2d(rng, N, 0.3, 30, 1, 10)),
        "needles": (corner(W // 16), corner(H // 16), br.random_cov2d(rng, N, 5, 3000, 1e2, 1e4)),
        "needles far": (uni(-3000, 3000), uni(-3000, 3000), br.random_cov2d(rng, N, 50, 5000, 1e2, 1e5)),
        "huge": (uni(-20000, 20000), uni(-20000, 20000), br.random_cov2d(rng, N, 100, 30000, 1, 1e3)),
        "slivers": (uni(0, W), uni(0, H), br.random_cov2d(rng, N, 1, 300, 1, 1e6)),
    }
    for name, (px, py, cov) in cases.items():
        bad, ref, emitted, reach = br.containment_violations(px, py, *cov, opacities(N), W, H)
        print(f"{name}: reference pairs {ref}, emitted {emitted}, pass the box test {reach}, lost {bad}")
        assert bad == 0, name
        assert reach <= emitted < ref, name


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

def _forward(inp, cam, dev, full=False, requires_grad=True):
    """one pass through the facade; returns (outputs, leaves, (num_rendered, emitted pairs))"""
    from opengaussian_amd import rasterizer as R
    R._DEBUG_EMITTED = []
    try:
        with (R.full_binning() if full else contextlib.nullcontext()):
            out, leaves = helpers.hip_forward(inp, cam, BG, 3, dev, requires_grad=requires_grad)
        counts = R._DEBUG_EMITTED[-1]
    finally:
        R._DEBUG_EMITTED = None
    return out, leaves, counts


def _oracle(sc, cam, W, H, f):
    from oracle import raster_oracle as ro
    inp = helpers.oracle_inputs(sc, cam, use_sh=True)
    g = ro.preprocess(inp["means3D"], inp["opacities"], inp["viewmatrix"], inp["projmatrix"], inp["campos"], W, H, W / (2 * f),
                      H / (2 * f), scales=inp["scales"], rotations=inp["rotations"], shs=inp["shs"], sh_degree=3)
    return inp, g, ro.bin_tiles(g, W, H)


def _binning_and_gradients(sc, cam, dev, W, H, f, gradients=True):
    """The assertions every scene gets.  Returns (oracle geometry, oracle binning, emitted pairs)."""
    inp, g, b = _oracle(sc, cam, W, H, f)
    (color, radii, depth, alpha), leaves, (D, emitted) = _forward(inp, cam, dev)
    assert D == color.grad_fn.num_rendered == b.num_rendered
    assert emitted <= D
    keys, ranges, ncontrib, plist = helpers.hip_export_binning(color)          # default list == full list filtered by the flag
    np.testing.assert_array_equal(radii.cpu().numpy(), g.radii)
    np.testing.assert_array_equal(keys, b.keys_sorted)
    np.testing.assert_array_equal(plist, b.point_list)
    np.testing.assert_array_equal(ranges, b.ranges)
    kept = int(helpers.LAST_REACH_FLAGS[0].sum())
    assert kept <= emitted, "fewer pairs emitted than the box test keeps"
    print(f"num_rendered {D}, emitted {emitted}, kept by the box test {kept}")
    if gradients:
        gen = torch.Generator().manual_seed(5)
        gC, gA = torch.randn(color.shape, generator=gen).to(dev), torch.randn(alpha.shape, generator=gen).to(dev)
        torch.autograd.backward([color, alpha], [gC, gA])
        (cf, rf, df, af), leaves_f, (Df, ef) = _forward(inp, cam, dev, full=True)
        assert Df == D == ef, "a full-binning pass emits the reference rects"
        for x, y in ((color, cf), (radii, rf), (depth, df), (alpha, af)):
            assert torch.equal(x, y)
        torch.autograd.backward([cf, af], [gC, gA])
        some = 0
        for k, v in leaves.items():
            if v is None or v.grad is None:
                continue
            assert torch.equal(v.grad, leaves_f[k].grad), k
            some += int(float(v.grad.abs().max()) > 0.0)
        assert some >= 5
    return g, b, emitted


def _place(sc, rows, px, py, z, W, H, f):
    """centres of `rows` that project onto pixel coordinates (px, py) at depth z (identity camera, helpers.tiny_scene)"""
    z = torch.as_tensor(z, dtype=torch.float32)
    sc.means3D[rows, 0] = (torch.as_tensor(px, dtype=torch.float32) + 0.5 - W / 2) * z / f
    sc.means3D[rows, 1] = (torch.as_tensor(py, dtype=torch.float32) + 0.5 - H / 2) * z / f
    sc.means3D[rows, 2] = z


@pytest.mark.gpu
def test_needles_across_tile_corners(gpu_device):
    """P = 1281 (block sums of five workgroups and one Gaussian), 176 x 112.  Every other Gaussian is a needle: scale ratio
    1e2 .. 1e4, random rotation, centre within 1.5 px of a tile corner, so the major axis runs along tile diagonals and the box
    test's slack term decides pairs.  The extent has to cover that slack."""
    W, H, f, P = 176, 112, 130.0, 1281
    sc, cam = helpers.tiny_scene(P, W, H, f, seed=301)
    gen = torch.Generator().manual_seed(302)
    rows = torch.arange(0, P, 2)
    n = rows.numel()
    corner_x = torch.randint(0, W // 16 + 1, (n,), generator=gen) * 16 - 0.5 + (torch.rand(n, generator=gen) * 3 - 1.5)
    corner_y = torch.randint(0, H // 16 + 1, (n,), generator=gen) * 16 - 0.5 + (torch.rand(n, generator=gen) * 3 - 1.5)
    _place(sc, rows, corner_x, corner_y, torch.rand(n, generator=gen) * 6 + 2, W, H, f)
    major = torch.exp(torch.rand(n, generator=gen) * 4.0 - 3.0)                          # 0.05 .. 2.7 world units
    ratio = torch.exp(torch.rand(n, generator=gen) * (np.log(1e4) - np.log(1e2)) + np.log(1e2))
    sc.scales[rows] = torch.stack([major, major / ratio, major / ratio], dim=1)
    sc.opacities[rows] = torch.rand(n, 1, generator=gen) * 0.98 + 0.02
    g, b, emitted = _binning_and_gradients(sc, cam, gpu_device, W, H, f)
    assert emitted < b.num_rendered


def _opacity_scene():
    W, H, f, P = 176, 112, 130.0, 1281
    sc, cam = helpers.tiny_scene(P, W, H, f, seed=303)
    gen = torch.Generator().manual_seed(304)
    edge_lo, edge_hi = np.float32(np.exp(-K_THR_MARGIN) / 255), np.float32(np.exp(K_THR_MARGIN) / 255)
    ulps = lambda v: [np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(1))]
    values = np.array(ulps(edge_lo) + ulps(edge_hi) + [1 / 255, 0.02, 0.99, 1.0], dtype=np.float32)
    rows = torch.arange(P)
    z = torch.rand(P, generator=gen) * 2 + 3
    _place(sc, rows, 40 + torch.rand(P, generator=gen) * (W - 80), 40 + torch.rand(P, generator=gen) * (H - 80), z, W, H, f)
    sigma_px = torch.rand(P, generator=gen) * 6 + 6                     # radius 18 .. 36 px: at least 3 x 3 tiles inside the image
    sc.scales[:] = (sigma_px * z / f)[:, None]
    sc.opacities[:, 0] = torch.from_numpy(values[np.arange(P) % len(values)])
    sc.means3D[5::97, 2] = -1.0                                          # a few behind the camera
    return sc, cam, W, H, f


def _float64_cap(g):
    """Tiles of the reference rects hit by the float64 bounding box of the ellipse  power >= ln(1 / (255 opacity)) - kThrMargin,
    padded by 2 px.  An opacity below the threshold opacity has no such ellipse: the box of its centre point, padded the same way
    (one tile, up to four at a corner)."""
    vis = g.radii > 0
    A, B, Cc = (g.conic[vis, k].astype(np.float64) for k in range(3))
    t = np.maximum(2.0 * (np.log(255.0 * g.opacity[vis].astype(np.float64)) + K_THR_MARGIN), 0.0)
    det = A * Cc - B * B
    hx, hy = np.sqrt(t * Cc / det) + 2.0, np.sqrt(t * A / det) + 2.0
    px, py = g.xy[vis, 0].astype(np.float64), g.xy[vis, 1].astype(np.float64)
    x0 = np.maximum(g.rect_min[vis, 0], np.ceil((px - hx - 15.0) / 16.0))
    x1 = np.minimum(g.rect_max[vis, 0], np.floor((px + hx) / 16.0) + 1)
    y0 = np.maximum(g.rect_min[vis, 1], np.ceil((py - hy - 15.0) / 16.0))
    y1 = np.minimum(g.rect_max[vis, 1], np.floor((py + hy) / 16.0) + 1)
    return int((np.maximum(x1 - x0, 0) * np.maximum(y1 - y0, 0)).sum())


@pytest.mark.gpu
def test_opacity_edges(gpu_device):
    """Isotropic Gaussians of radius 18 .. 36 px with opacities exp(-/+ kThrMargin) / 255 and one ulp either side, 1 / 255, 0.02,
    0.99 and 1.0.  At exp(-kThrMargin) / 255 the threshold is zero: the ellipse is a point, and one ulp below there is none.
    The emitted count stays below the float64 cap; the reference rects alone would not (asserted: the cap is below num_rendered)."""
    sc, cam, W, H, f = _opacity_scene()
    g, b, emitted = _binning_and_gradients(sc, cam, gpu_device, W, H, f)
    w = g.rect_max - g.rect_min
    assert int((w[g.radii > 0] >= 3).all()), "every visible Gaussian's reference rect is at least 3 x 3 tiles"
    cap = _float64_cap(g)
    print(f"float64 cap {cap}")
    assert cap < b.num_rendered, "the scene must not meet the cap with the reference rects"
    assert emitted <= cap
    assert emitted < b.num_rendered


@pytest.mark.gpu
@pytest.mark.parametrize("culled_front", [False, True], ids=["mixed", "first_three_workgroups_culled"])
def test_borders_and_culled_workgroups(gpu_device, culled_front):
    """Centres up to four radii outside each image edge (the cut must clamp against the reference rect, whose ends the image
    clamps), a fifth of the Gaussians behind the camera; second case: the first three workgroups wholly culled (block sums of
    zero in both runs of sums)."""
    W, H, f, P = 176, 112, 130.0, 1281
    sc, cam = helpers.tiny_scene(P, W, H, f, seed=305)
    gen = torch.Generator().manual_seed(306)
    z = torch.rand(P, generator=gen) * 3 + 2
    sigma_px = torch.rand(P, generator=gen) * 10 + 2
    side = torch.randint(0, 4, (P,), generator=gen)
    out = torch.rand(P, generator=gen) * 4 * 3 * sigma_px                     # up to four radii outside
    along_x, along_y = torch.rand(P, generator=gen) * W, torch.rand(P, generator=gen) * H
    px = torch.where(side == 0, -out, torch.where(side == 1, W + out, along_x))
    py = torch.where(side == 2, -out, torch.where(side == 3, H + out, along_y))
    _place(sc, torch.arange(P), px, py, z, W, H, f)
    sc.scales[:] = (sigma_px * z / f)[:, None] * torch.exp(torch.randn(P, 3, generator=gen) * 0.5)
    sc.means3D[torch.rand(P, generator=gen) < 0.2, 2] = -1.0
    if culled_front:
        sc.means3D[:768, 2] = -1.0
    g, b, emitted = _binning_and_gradients(sc, cam, gpu_device, W, H, f, gradients=False)
    assert int((g.radii > 0).sum()) > 100 and b.num_rendered > 1000          # the scene itself: enough is drawn
    if culled_front:
        assert int(g.radii[:768].max()) == 0
    assert emitted < b.num_rendered


@pytest.mark.gpu
def test_rects_wider_than_255_tiles(gpu_device):
    """4112 x 32 (257 x 2 tiles).  duplicate_kernel flags the pairs of a rect wider than 255 tiles without a test (its per-thread
    path), so all of them are in the list, and the full-binning list has them too: such a rect is not cut, whatever the ellipse
    says.  Gaussian 600 covers the whole width at opacity 0.99; Gaussian 700 has the same reference rect at opacity 0.02, where the
    ellipse's box is about 212 tiles wide -- a cut there would lose 88 pairs of the list.  The per-thread path starts at an offset
    the workgroup only knows after its scan of the emitted counts of the small Gaussians in front."""
    W, H, f, P = 4112, 32, 70.0, 1100
    sc, cam = helpers.tiny_scene(P, W, H, f, seed=307)
    for row, op in ((600, 0.99), (700, 0.02)):
        sc.means3D[row] = torch.tensor([0.0, 0.0, 3.0])
        sc.scales[row] = 40.0
        sc.opacities[row] = op
    g, b, emitted = _binning_and_gradients(sc, cam, gpu_device, W, H, f, gradients=False)
    for row in (600, 700):
        assert int(g.rect_max[row, 0] - g.rect_min[row, 0]) > 255
    sigma = f * 40.0 / 3.0
    assert 2 * np.sqrt(2 * (np.log(255 * 0.02) + K_THR_MARGIN)) * sigma < 255 * 16 - 32      # the ellipse's box of 700 is narrower
    flags = helpers.LAST_REACH_FLAGS[0]
    assert int(flags[b.point_list == 700].sum()) == 2 * 257 == int(flags[b.point_list == 600].sum())
    assert 2 * 2 * 257 < emitted < b.num_rendered


@pytest.mark.gpu
def test_deferred_passes_and_capacity_overflow_read_the_emitted_count(gpu_device):
    """Second pass at one size: buffers sized from the hint, every binning kernel reads its key count on the device -- the
    emitted total, not the reported one.  Third pass: a forced capacity overflow (hint of 7), render phase redone with exact
    buffers.  Images, radii, lists and both counts equal the blocking pass'; num_rendered equals the oracle's."""
    from opengaussian_amd import rasterizer as R
    sc, cam, W, H, f = _opacity_scene()
    inp, g, b = _oracle(sc, cam, W, H, f)
    key = (sc.means3D.shape[0], W, H, 1)
    R._LAST_NUM_RENDERED.pop(key, None)
    st0 = dict(R.PASS_STATS)
    (c0, r0, d0, a0), _, n0 = _forward(inp, cam, gpu_device)
    (c1, r1, d1, a1), _, n1 = _forward(inp, cam, gpu_device)
    R._LAST_NUM_RENDERED[key].clear(); R._LAST_NUM_RENDERED[key].append(7)
    (c2, r2, d2, a2), _, n2 = _forward(inp, cam, gpu_device)
    assert {k: R.PASS_STATS[k] - st0[k] for k in ("blocking", "deferred", "overflow")} == {"blocking": 1, "deferred": 2, "overflow": 1}
    assert n0 == n1 == n2 and n0[0] == b.num_rendered and n0[1] < n0[0]
    for c, r, d, a in ((c1, r1, d1, a1), (c2, r2, d2, a2)):
        assert c.grad_fn.num_rendered == b.num_rendered
        assert torch.equal(c, c0) and torch.equal(r, r0) and torch.equal(d, d0) and torch.equal(a, a0)
    k0 = helpers.hip_export_binning(c0)
    np.testing.assert_array_equal(k0[0], b.keys_sorted)
    for cc in (c1, c2):
        for x, y in zip(k0, helpers.hip_export_binning(cc)):
            np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_block_sums_past_one_trip_of_the_offsets_kernel(gpu_device):
    """block_offsets_kernel takes 8192 workgroup sums per trip: P = 2 100 000 is 8204 workgroups, a second trip of 12 sums (a
    run that ends inside a thread's eight) that starts from the first trip's carry, in both runs of sums.  No oracle at this
    size: the full-binning pass, which scans the P counts instead, gives the reference -- same num_rendered, the default list
    equal to its list filtered by the reach flag (helpers.hip_export_binning), same images.  Nine in ten Gaussians are behind
    the camera, at random, so the lists stay short and every workgroup still has something to emit."""
    W, H, f, P = 64, 48, 60.0, 2_100_000
    sc, cam = helpers.tiny_scene(P, W, H, f, seed=308)
    sc.means3D[torch.rand(P, generator=torch.Generator().manual_seed(309)) < 0.9, 2] = -1.0
    inp = helpers.oracle_inputs(sc, cam, use_sh=True)
    (color, radii, depth, alpha), _, (D, emitted) = _forward(inp, cam, gpu_device)
    assert int((radii[-256 * 12:] > 0).sum()) > 100, "the second trip's workgroups emit something"
    keys, ranges, ncontrib, plist = helpers.hip_export_binning(color)
    assert len(keys) == D and 0 < emitted < D
    assert int(helpers.LAST_REACH_FLAGS[0].sum()) <= emitted
