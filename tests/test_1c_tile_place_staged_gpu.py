"""GPU: the placement of the counting sort by tile (binning.hip: tile_place_kernel) on a grid of place chunks x tile slices,
with each workgroup's pairs staged in LDS and written out as runs, against the oracle's binning.

A place chunk is G consecutive chunks of the B that tile_count_kernel counted, a slice ceil(tiles / S) consecutive tiles; a
workgroup whose pair count (known from the table) fits its staging words places into LDS and writes each tile's run with one
lane per entry, any other workgroup stores its pairs one by one as before.  ogs_raster_tile_place_debug forces G, S and the
staging words and reports (place chunks, slices, staging words) of a pass; every test asserts through it that the forced grid is
the one the pass took, and holds keys, point list and ranges bit for bit against oracle.raster_oracle.bin_tiles through
tests.test_19_tile_count_binning_gpu._check.  64 x 48 images (12 tiles), the scenes of tests/test_18 and tests/test_19."""
import ctypes

import numpy as np
import pytest

from opengaussian_amd.synthetic import make_camera, make_scene
from tests import helpers
from tests.test_18_tile_depth_order_gpu import TILE_11, _capacity, _tile_scene
from tests.test_19_tile_count_binning_gpu import TILES, _blocks, _check, _needle_scene, _spread_scene, _trip, hooks  # noqa: F401

pytestmark = pytest.mark.gpu

ROOMY = 27_000          # staging words: more than the six trips two chunks of the spread scene hold at B = 3, and than the pairs
                        # of all nine trips inside one half of the tiles; less than LDS has room for


def _lib():
    from opengaussian_amd import _lib
    return _lib.lib()


def _place(D, tiles, group=-1, slices=-1, stage=-1):
    """sets the hooks that are >= 0 and returns (place chunks, slices, staging words) of a pass of this capacity and grid"""
    chosen = (ctypes.c_int32 * 3)()
    assert _lib().ogs_raster_tile_place_debug(D, tiles, group, slices, stage, chosen) == 0
    return tuple(int(c) for c in chosen)


@pytest.fixture
def place():
    """set(group, slices, stage_words); the library's own choice comes back afterwards"""
    yield lambda group, slices, stage=0: _place(1, 1, group, slices, stage)
    _place(1, 1, 0, 0, 0)


def _took(D, tiles=TILES):
    return _place(D, tiles)


@pytest.mark.parametrize("group,chunks", [(1, 3), (2, 2), (3, 1), (5, 1)])
def test_groups_of_count_chunks(gpu_device, hooks, place, group, chunks):
    """B = 3 over 6-9 emitted trips: G = 1 (three place chunks), 2 (two rows and one row: the last group is shorter), 3 (one place
    chunk) and 5 > B (one place chunk); two slices (five and four of the nine tiles), every pair staged"""
    hooks(3)
    place(group, 2, ROOMY)
    sc, cam = _spread_scene(20_000, 1200, seed=191)
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device)
    assert 6 * _trip() < emitted <= 9 * _trip(), emitted
    assert _blocks(D) == 3 and _took(D) == (chunks, 2, ROOMY), (_blocks(D), _took(D))
    assert int(((ranges[:, 1] - ranges[:, 0]) > 0).sum()) >= 9


@pytest.mark.parametrize("slices", [1, 2, 5, 12, 13])
def test_slices_of_the_tiles(gpu_device, hooks, place, slices):
    """B = 3, G = 2 and S = 1, 2, 5 (slices of 3, 3, 3, 3 and 0 tiles: one is empty), 12 (one tile per slice) and 13 > tiles"""
    hooks(3)
    place(2, slices, ROOMY)
    sc, cam = _spread_scene(20_000, 1200, seed=191)
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device)
    assert _blocks(D) == 3 and _took(D) == (2, slices, ROOMY), (_blocks(D), _took(D))


@pytest.mark.parametrize("fit", ["exact", "one_below", "none"])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_staging_words_around_a_workgroups_pair_count(gpu_device, hooks, place, delta, fit):
    """one tile, n = 2 trips + delta pairs, B = 2, G = S = 1: workgroups of (trip, trip - 1), (trip, trip) and (2 trips, 1) pairs.
    Staging words = the larger count (it fits exactly: both stage), one below it (that workgroup stores its pairs one by one,
    the other -- unless it holds as many -- stages) and 1 (no workgroup stages, but for the one that holds a single pair)"""
    hooks(2)
    n = 2 * _trip() + delta
    largest = 2 * _trip() if delta > 0 else _trip()
    words = {"exact": largest, "one_below": largest - 1, "none": 1}[fit]
    place(1, 1, words)
    sc, cam = _tile_scene(n, 1500, 20.0, 28.0, seed=190 + delta)
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device)
    assert D == n and emitted == n, (D, emitted)
    assert _blocks(n) == 2 and _took(n) == (2, 1, words), (_blocks(n), _took(n))
    assert int(ranges[TILE_11, 1]) - int(ranges[TILE_11, 0]) == n


def test_staged_and_direct_workgroups_in_one_launch(gpu_device, hooks, place):
    """spread scene, B = 3, G = S = 1, staging words = the mean pair count of the three workgroups (the last chunk is shorter than
    the others): the largest workgroup stores its pairs one by one, the smallest stages"""
    hooks(3)
    sc, cam = _spread_scene(20_000, 1200, seed=191)
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device, images=False)
    kept = int(helpers.LAST_REACH_FLAGS[0].sum())
    trip = _trip()
    assert 6 * trip < emitted < 9 * trip, emitted                 # chunks of three trips; the last holds fewer pairs
    words = kept // 3
    place(1, 1, words)
    _check(sc, cam, gpu_device)
    assert _took(D) == (3, 1, words), _took(D)


def test_chunks_and_slices_whose_pairs_are_all_dropped(gpu_device, hooks, place):
    """G = 2, S = 2.  Needles alone: pairs are emitted, none is kept -- no workgroup has a pair to stage.  Then the same needles in
    front of 2048 ordinary Gaussians of tile (1, 1), one count chunk per trip: the first place chunk holds nothing but dropped
    pairs, the second slice (tiles 6..11) no pair at all"""
    hooks(0)
    place(2, 2)
    sc, cam = _needle_scene(0, seed=193)
    ref, ranges, plist, (D, needle_pairs) = _check(sc, cam, gpu_device)
    B = _blocks(D)
    assert B >= 1 and needle_pairs >= _trip(), (D, needle_pairs)
    assert _took(D)[:2] == (-(-B // 2), 2) and _took(D)[2] > 0, _took(D)
    assert not helpers.LAST_REACH_FLAGS[0].any()
    n = needle_pairs + 2048
    want = -(-n // _trip())
    hooks(want)
    sc, cam = _needle_scene(2048, seed=193)
    ref, ranges, plist, (D, emitted) = _check(sc, cam, gpu_device)
    assert emitted == n and _blocks(D) == want, (emitted, n, _blocks(D), want)
    assert _took(D)[:2] == (-(-want // 2), 2) and _took(D)[2] > 0, _took(D)
    assert int(helpers.LAST_REACH_FLAGS[0].sum()) == 2048


def test_emitted_count_below_the_chunk_count(gpu_device, hooks, place):
    """deferred pass with a capacity far above the list: B = 8, G = 4, S = 3 and 5 emitted pairs -- place chunk 0 holds them all,
    in slice 1 (tiles 4..7); the second place chunk is empty"""
    hooks(8)
    place(4, 3)
    sc, cam = _tile_scene(5, 1500, 20.0, 28.0, seed=192)
    cap = int(4000 * 1.25) + 4096
    assert _blocks(cap) == 8 and _took(cap)[:2] == (2, 3) and _took(cap)[2] > 0, _took(cap)
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device, hint=4000)
    assert D == 5 and emitted == 5


def test_device_count_of_zero(gpu_device, hooks, place):
    """every Gaussian behind the camera, deferred pass, B = 4, G = 2, S = 3: the workgroups of place chunk 0 still write their
    slices' ranges, all (0, 0), and kept = 0"""
    hooks(4)
    place(2, 3)
    sc, cam = _tile_scene(0, 1500, 20.0, 28.0, seed=194)
    cap = int(3000 * 1.25) + 4096
    assert _blocks(cap) == 4 and _took(cap)[:2] == (2, 3), _took(cap)
    ref, ranges, plist, (D, emitted) = _check(sc, cam, gpu_device, hint=3000)
    assert D == 0 and emitted == 0 and len(plist) == 0 and not ranges.any()


@pytest.mark.parametrize("case", ["wave", "wave+1", "cap+1", "wave_one_depth", "wave+1_one_depth", "cap+1_one_depth"])
def test_ties_in_descending_id_order_reach_every_sort_path(gpu_device, hooks, place, case):
    """B = 3, G = 2, S = 2, chunks walked back to front: staged runs of equal depths (pairs of neighbours, or the whole list) reach
    the depth sort with descending ids, in lists at and past the one-wave limit and past the LDS limit"""
    hooks(3, reverse=1)
    place(2, 2, ROOMY)
    cap, wave = _capacity(1), _capacity(0)
    n = {"wave": wave, "wave+1": wave + 1, "cap+1": cap + 1}[case.split("_")[0]]
    sc, cam = _tile_scene(n, 1500, 20.0, 28.0, seed=196 + n, equal_depth=case.endswith("one_depth"))
    ref, ranges, plist, (D, emitted) = _check(sc, cam, gpu_device)
    assert _blocks(D) == 3 and _took(D) == (2, 2, ROOMY) and emitted == n, (_blocks(D), _took(D), emitted)
    r0, r1 = ranges[TILE_11]
    assert r1 - r0 == n
    d = ref["geom"].depth[plist[r0:r1]]
    assert int((np.diff(d) == 0).sum()) >= n // 2 - 1


def test_spread_scene_reversed_with_ties_across_chunks(gpu_device, hooks, place):
    """one depth for the whole scene, B = 5, G = 2, S = 2, walked backwards: every list is a single run of ties made of the staged
    runs of three place chunks"""
    hooks(5, reverse=1)
    place(2, 2, ROOMY)
    sc, cam = _spread_scene(20_000, 1200, seed=197, equal_depth=True)
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device)
    assert _blocks(D) == 5 and _took(D) == (3, 2, ROOMY), (_blocks(D), _took(D))


def test_deferred_capacity_below_the_emitted_count_ends_in_the_rerun(gpu_device, hooks, place):
    """hint 1 -> capacity 4097 < emitted pairs, G = 2, S = 2: the pairs at or past the capacity are neither counted nor staged, the
    host sees num_rendered > capacity and renders again with exact buffers; image and lists are the oracle's"""
    from opengaussian_amd import rasterizer as R
    hooks(0)
    place(2, 2)
    sc, cam = _spread_scene(6000, 1200, seed=200)
    before = R.PASS_STATS["overflow"]
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device, hint=1)
    assert R.PASS_STATS["overflow"] == before + 1
    assert emitted > int(1 * 1.25) + 4096, emitted
    for cap in (int(1 * 1.25) + 4096, D):                         # the pass that overflowed and the re-run
        B = _blocks(cap)
        assert B >= 1 and _took(cap)[:2] == (-(-B // 2), 2) and _took(cap)[2] > 0, (cap, B, _took(cap))


def test_two_calls_give_the_same_point_list(gpu_device, hooks, place):
    hooks(0)
    place(2, 3)
    sc, cam = _spread_scene(20_000, 1200, seed=198)
    _, ranges_a, plist_a, (D, _) = _check(sc, cam, gpu_device)
    _, ranges_b, plist_b, _ = _check(sc, cam, gpu_device, hint=None)
    assert _took(D)[1] == 3 and _took(D)[2] > 0, _took(D)
    np.testing.assert_array_equal(plist_a, plist_b)
    np.testing.assert_array_equal(ranges_a, ranges_b)


def test_the_librarys_own_choice(gpu_device, hooks, place):
    """no hook set, 24 x 16 tiles, 50 000 Gaussians of about 26 tiles each: 1.3 M pairs, more than two trips for each of the
    library's 128 chunks, so its rule stages -- G = 1 and two slices (128 x 2 workgroups)"""
    hooks(0)
    place(0, 0, 0)
    w, h, f = 16 * 24, 16 * 16, 300.0
    tiles = 24 * 16
    sc = make_scene(50_000, w, h, f, f, seed=201, log_scale_mean=-2.3)
    cam = make_camera(w, h, f, f)
    ref, ranges, _, (D, emitted) = _check(sc, cam, gpu_device, w=w, h=h, f=f, images=False)
    assert D >= 2 * 128 * _trip(), D
    B = _blocks(D, tiles)
    chunks, slices, words = _took(D, tiles)
    assert B == 128 and (chunks, slices) == (128, 2) and words > 0, (D, emitted, B, chunks, slices, words)
