"""GPU: the counting sort by tile of the default streaming pass (binning.hip: tile_count_kernel, tile_count_scan_kernel,
tile_place_kernel) and the tie order of the per-tile depth sort behind it, against the oracle's binning.

The pass cuts the emitted (Gaussian, tile) pairs into B chunks of a multiple of ogs_raster_tile_count_trip() pairs, counts
each chunk's pairs per tile in LDS, scans the table of counts and places every value at an LDS cursor of its tile -- in
whatever order the LDS atomics hand out.  tile_depth_sort_kernel therefore orders equal depths by id itself.  Every test holds
keys, point list and tile ranges bit for bit against oracle.raster_oracle.bin_tiles through helpers.hip_export_binning (which
also holds the culled list of the counting path against the full list of the radix path, and their images bit for bit).

ogs_raster_tile_count_debug forces B and reverses the walk of a chunk (ties then arrive in descending id order); both hooks are
process-wide and are handed back by the fixture.  64 x 48 images (12 tiles), scenes of tests/test_18: n Gaussians of radius 2
inside tile (1, 1) -- exactly n emitted pairs, one list -- or spread over nine tiles, plus Gaussians behind the camera."""
from collections import deque

import numpy as np
import pytest
import torch

from opengaussian_amd.synthetic import make_camera, make_scene
from tests import helpers
from tests.test_10_raster_gpu import IMG_TOL
from tests.test_18_tile_depth_order_gpu import F, H, TILE_11, W, _capacity, _tile_scene

pytestmark = pytest.mark.gpu

TILES = ((W + 15) // 16) * ((H + 15) // 16)
BG = (0.2, 0.1, 0.3)


def _lib():
    from opengaussian_amd import _lib
    return _lib.lib()


def _trip():
    return int(_lib().ogs_raster_tile_count_trip())


@pytest.fixture
def hooks():
    """set(force_blocks, reverse); the library's own choice and the forward walk come back afterwards"""
    lib = _lib()
    yield lambda force, reverse=0: lib.ogs_raster_tile_count_debug(1, 1, force, reverse)
    lib.ogs_raster_tile_count_debug(1, 1, 0, 0)


def _set_hint(P, w, h, hint):
    """hint None: the next pass at this size reads num_rendered back and sizes its render phase exactly; otherwise it is a
    deferred pass with the capacity int(1.25 hint) + 4096"""
    from opengaussian_amd import rasterizer as R
    key = (P, w, h, 1)
    if hint is None:
        R._LAST_NUM_RENDERED.pop(key, None)
    else:
        R._LAST_NUM_RENDERED[key] = deque([int(hint)], maxlen=R._HINT_WINDOW)


def _check(sc, cam, dev, hint=None, w=W, h=H, f=F, images=True):
    """One pass against the oracle; returns (oracle result, ranges, point list, (num_rendered, emitted pairs))"""
    from opengaussian_amd import rasterizer as R
    from oracle import raster_oracle as ro
    inp = helpers.oracle_inputs(sc, cam, use_sh=True)
    kw = dict(W=w, H=h, tanfovx=w / (2 * f), tanfovy=h / (2 * f), sh_degree=3, **inp)
    if images:
        ref = ro.render_forward(bg=np.array(BG, np.float32), **kw)
    else:
        g = ro.preprocess(**kw)
        ref = dict(geom=g, binning=ro.bin_tiles(g, w, h))
    _set_hint(sc.means3D.shape[0], w, h, hint)
    R._DEBUG_EMITTED = []
    try:
        (color, radii, depth, alpha), _ = helpers.hip_forward(inp, cam, BG, 3, dev, requires_grad=True)
        counts = R._DEBUG_EMITTED[0]
    finally:
        R._DEBUG_EMITTED = None
    keys, ranges, ncontrib, plist = helpers.hip_export_binning(color)
    np.testing.assert_array_equal(radii.cpu().numpy(), ref["geom"].radii)
    assert counts[0] == ref["binning"].num_rendered and len(keys) == ref["binning"].num_rendered
    np.testing.assert_array_equal(keys, ref["binning"].keys_sorted)
    np.testing.assert_array_equal(plist, ref["binning"].point_list)
    np.testing.assert_array_equal(ranges, ref["binning"].ranges)
    if images:
        helpers.assert_close_modulo_threshold_flips(color.detach().cpu().numpy(), ref["color"], IMG_TOL)
        helpers.assert_close_modulo_threshold_flips(alpha.detach().cpu().numpy(), ref["alpha"], IMG_TOL)
    return ref, ranges, plist, counts


def _blocks(D, tiles=TILES):
    """B of a pass with this list capacity under the hooks as they stand (0: the radix path)"""
    return int(_lib().ogs_raster_tile_count_debug(D, tiles, -1, -1))


def _spread_scene(n_vis, n_culled, seed, equal_depth=False):
    """centres in [4, 44)^2 px: nine of the twelve tiles, every one fed by every chunk"""
    return _tile_scene(n_vis, n_culled, 4.0, 44.0, seed=seed, equal_depth=equal_depth)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_emitted_count_around_a_multiple_of_chunk_and_trip(gpu_device, hooks, delta):
    """B = 2 and n = 2 trips + delta pairs, all in one tile: chunks of (trip - 1 | trip, trip) and, one above, of (2 trips, 1) pairs;
    the tile's list comes from every chunk"""
    hooks(2)
    n = 2 * _trip() + delta
    sc, cam = _tile_scene(n, 1500, 20.0, 28.0, seed=190 + delta)
    assert _blocks(n) == 2
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device)
    assert D == n and emitted == n, (D, emitted)
    assert int(ranges[TILE_11, 1]) - int(ranges[TILE_11, 0]) == n


@pytest.mark.parametrize("blocks", [1, 3, 0])
def test_spread_scene_one_chunk_several_chunks_and_the_default(gpu_device, hooks, blocks):
    """B = 1 (one chunk feeds every tile), B = 3 (every tile fed by every chunk, chunk ends inside the lists) and the library's
    own B (one chunk per trip here); pairs of equal depths throughout"""
    hooks(blocks)
    sc, cam = _spread_scene(20_000, 1200, seed=191)
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device)
    assert 6 * _trip() < emitted <= 9 * _trip(), emitted           # B = 3: chunks of three trips, the last one shorter
    want = blocks if blocks else min(-(-D // _trip()), D // TILES - 1)
    assert _blocks(D) == want and want >= 1, (_blocks(D), want)
    assert int(((ranges[:, 1] - ranges[:, 0]) > 0).sum()) >= 9


def test_emitted_count_below_the_chunk_count(gpu_device, hooks):
    """deferred pass with a capacity far above the list: B = 8 chunks, 5 emitted pairs -- chunk 0 holds them all, the other
    seven are empty"""
    hooks(8)
    sc, cam = _tile_scene(5, 1500, 20.0, 28.0, seed=192)
    assert _blocks(int(4000 * 1.25) + 4096) == 8
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device, hint=4000)
    assert D == 5 and emitted == 5


N_NEEDLES = 1100


def _needle_scene(n_after, seed):
    """N_NEEDLES thin Gaussians along the anti-diagonal x + y = -40 px, centred 28 px outside the image's top-left corner, then
    n_after ordinary Gaussians inside tile (1, 1).  A needle is 40 px long (sigma) and about 1 px thin: its 3-sigma rect and the
    bounding box of its reach ellipse cover tiles of the image, the ellipse itself (reach: 3 sigma of the thin axis, ~3.5 px)
    stays 28 px away from the corner pixel -- every pair a needle emits carries the drop key."""
    P = N_NEEDLES + n_after
    sc, cam = _tile_scene(P, 0, 20.0, 28.0, seed=seed)
    g = torch.Generator().manual_seed(7000 + seed)
    z = 4.0 + 0.5 * torch.rand(N_NEEDLES, generator=g)
    px = -20.0 + 2.0 * torch.rand(N_NEEDLES, generator=g)
    py = -20.0 + 2.0 * torch.rand(N_NEEDLES, generator=g)
    sc.means3D[:N_NEEDLES] = torch.stack([(px - (W - 1) / 2) * z / F, (py - (H - 1) / 2) * z / F, z], dim=1)
    sc.scales[:N_NEEDLES] = torch.stack([40.0 * z / F, 0.5 * z / F, 0.5 * z / F], dim=1)
    half = -np.pi / 8                                             # rotation by -45 degrees about z: the long axis along (1, -1)
    sc.rotations[:N_NEEDLES] = torch.tensor([np.cos(half), 0.0, 0.0, np.sin(half)], dtype=torch.float32)
    return sc, cam


def test_chunks_whose_pairs_are_all_dropped(gpu_device, hooks):
    """needles alone: pairs are emitted, none is kept (twelve empty ranges).  Then the same needles in front of 2048 ordinary
    Gaussians, B = one chunk per trip: the first chunk (at least) holds nothing but dropped pairs"""
    hooks(0)
    sc, cam = _needle_scene(0, seed=193)
    ref, ranges, plist, (D, needle_pairs) = _check(sc, cam, gpu_device)
    assert _blocks(D) >= 1 and needle_pairs >= _trip(), (D, needle_pairs)
    assert not helpers.LAST_REACH_FLAGS[0].any()                  # (the helper returns the FULL list; its flags say what was kept)
    n = needle_pairs + 2048
    want = -(-n // _trip())
    hooks(want)
    sc, cam = _needle_scene(2048, seed=193)
    ref, ranges, plist, (D, emitted) = _check(sc, cam, gpu_device)
    assert emitted == n and _blocks(D) == want, (emitted, n, _blocks(D), want)
    assert int(helpers.LAST_REACH_FLAGS[0].sum()) == 2048


def test_device_count_of_zero(gpu_device, hooks):
    """every Gaussian behind the camera, deferred pass: the kernels run with a device count of 0 and leave 12 empty ranges"""
    hooks(4)
    sc, cam = _tile_scene(0, 1500, 20.0, 28.0, seed=194)
    ref, ranges, plist, (D, emitted) = _check(sc, cam, gpu_device, hint=3000)
    assert D == 0 and emitted == 0 and len(plist) == 0 and not ranges.any()


def test_one_tile_fed_by_one_chunk_only(gpu_device, hooks):
    """B = 4: Gaussians of the first quarter of the ids sit in tile (1, 1), all others in tile (2, 2) -- tile (1, 1) is fed by
    chunk 0 alone, tile (2, 2) by every chunk"""
    hooks(4)
    n = 4 * _trip()
    sc, cam = _tile_scene(n, 0, 20.0, 28.0, seed=195)
    shift = 16.0 * sc.means3D[n // 4 - 64:, 2] / F
    sc.means3D[n // 4 - 64:, 0] += shift
    sc.means3D[n // 4 - 64:, 1] += shift
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device)
    assert _blocks(D) == 4 and emitted == n
    lens = (ranges[:, 1] - ranges[:, 0]).astype(np.int64)
    tile_22 = 2 * ((W + 15) // 16) + 2
    assert lens[TILE_11] == n // 4 - 64 and lens[tile_22] == n - lens[TILE_11], lens


@pytest.mark.parametrize("case", ["wave", "wave+1", "cap", "cap+1", "wave_one_depth", "cap+1_one_depth"])
def test_ties_in_descending_id_order_reach_every_sort_path(gpu_device, hooks, case):
    """chunks placed back to front: equal depths (pairs of neighbours, or the whole list) reach the depth sort with descending
    ids, in lists on both sides of the one-wave limit and of the LDS limit (B = 3: one trip per chunk)"""
    hooks(3, reverse=1)
    cap, wave = _capacity(1), _capacity(0)
    n = {"wave": wave, "wave+1": wave + 1, "cap": cap, "cap+1": cap + 1}[case.split("_")[0]]
    sc, cam = _tile_scene(n, 1500, 20.0, 28.0, seed=196 + n, equal_depth=case.endswith("one_depth"))
    ref, ranges, plist, (D, emitted) = _check(sc, cam, gpu_device)
    assert _blocks(D) == 3 and emitted == n
    r0, r1 = ranges[TILE_11]
    assert r1 - r0 == n
    d = ref["geom"].depth[plist[r0:r1]]
    assert int((np.diff(d) == 0).sum()) >= n // 2 - 1


def test_spread_scene_reversed_with_ties_across_chunks(gpu_device, hooks):
    """one depth for the whole scene, B = 5 (chunks of two trips, four of them hold pairs) walked backwards: every list is a
    single run of ties that crosses the chunk ends"""
    hooks(5, reverse=1)
    sc, cam = _spread_scene(20_000, 1200, seed=197, equal_depth=True)
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device)
    assert _blocks(D) == 5


def test_two_calls_give_the_same_point_list(gpu_device, hooks):
    hooks(0)
    sc, cam = _spread_scene(20_000, 1200, seed=198)
    _, ranges_a, plist_a, _ = _check(sc, cam, gpu_device)
    _, ranges_b, plist_b, _ = _check(sc, cam, gpu_device, hint=None)
    np.testing.assert_array_equal(plist_a, plist_b)
    np.testing.assert_array_equal(ranges_a, ranges_b)


def test_grid_past_the_lds_bound_takes_the_radix_path(gpu_device, hooks):
    """111 x 111 tiles = 12 321 > 12 288: the pass keeps the radix sort (B = 0) and matches the oracle's binning"""
    hooks(0)
    w = h = 16 * 111
    f = 900.0
    P = 1100
    sc = make_scene(P, w, h, f, f, seed=199, log_scale_mean=-3.5)
    cam = make_camera(w, h, f, f)
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device, w=w, h=h, f=f, images=False)
    tiles = 111 * 111
    assert D >= tiles, D                                          # the list alone would have had room for the table
    assert _blocks(D, tiles) == 0 and _blocks(D, 12288) >= 1


def test_deferred_capacity_below_the_emitted_count_ends_in_the_rerun(gpu_device, hooks):
    """hint 1 -> capacity 4097 < emitted pairs: duplicate stops at the capacity, the counting pass sorts what was written, the
    host sees num_rendered > capacity and renders again with exact buffers; image and lists are the oracle's"""
    from opengaussian_amd import rasterizer as R
    hooks(0)
    sc, cam = _spread_scene(6000, 1200, seed=200)
    before = R.PASS_STATS["overflow"]
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device, hint=1)
    assert R.PASS_STATS["overflow"] == before + 1
    assert emitted > int(1 * 1.25) + 4096, emitted
