"""GPU: the one-wave path of the per-tile depth sort (binning.hip::wave_sort_list) against the oracle's binning.

A list of 2 .. ogs_raster_tile_sort_capacity(0) entries is cut into buckets on the top eight bits of its key range (digit =
(key - smallest key) >> shift; the ids' range when the list has one key) by a pass that is not stable, and every entry is then
ranked inside its bucket on the total order (key, id).  A list whose largest bucket holds more than the bucket cap
(ogs_raster_tile_sort_capacity(2)) takes the stable LSD passes and the look at the ties instead.  Either way the reference order (oracle.raster_oracle.bin_tiles: stable argsort of
tile << 32 | depth bits over pairs emitted in id order) must come out bit for bit: keys, point list and tile ranges, in the default
(culled) binning mode and in full-binning mode (helpers.hip_export_binning holds the culled list against the full one and
returns the full one).

Scenes as in tests/test_18: a 64 x 48 image, identity camera, every visible Gaussian inside tile (1, 1) -- one list of exactly n
entries -- plus 1 500 culled Gaussians at random indices.  With the identity camera the depth key is the bit pattern of z, so
the cases craft z from bits.  Every case runs under the library's rule, under a forced cap of 1 (every list takes the LSD passes)
and under a cap above any list (every list is ranked inside its buckets, however large they are); the three results are held
against the oracle, hence against each other.  ogs_raster_tile_sort_debug and ogs_raster_tile_count_debug are process-wide and
are handed back by the fixture."""
import numpy as np
import pytest
import torch

from opengaussian_amd.synthetic import make_camera, make_scene
from tests import helpers

pytestmark = pytest.mark.gpu

W, H, F = 64, 48, 60.0
TILE_11 = 1 * ((W + 15) // 16) + 1          # tile (1, 1)
N_CULLED = 1500
BG = (0.2, 0.1, 0.3)
ABOVE_ANY_LIST = 1 << 20


def _lib():
    from opengaussian_amd import _lib as L
    return L.lib()


def _capacity(level):
    """0: the longest list one wave sorts alone; 2: the bucket cap in force"""
    return int(_lib().ogs_raster_tile_sort_capacity(level))


@pytest.fixture
def hooks():
    """cap(bucket_cap) and count(force_blocks, reverse); the library's own choices come back afterwards"""
    lib = _lib()

    class Hooks:
        cap = staticmethod(lambda c: lib.ogs_raster_tile_sort_debug(c))
        count = staticmethod(lambda force, reverse=0: lib.ogs_raster_tile_count_debug(1, 1, force, reverse))
    yield Hooks
    lib.ogs_raster_tile_sort_debug(0)
    lib.ogs_raster_tile_count_debug(1, 1, 0, 0)


def _bits_to_z(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _scene(z, seed):
    """len(z) Gaussians at depth z whose pixel centres fall in [20, 28)^2 (radius <= 3: tile (1, 1) alone), opacity 0.3, plus
    N_CULLED Gaussians behind the camera at random indices."""
    z = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32))
    n = z.shape[0]
    P = n + N_CULLED
    sc = make_scene(P, W, H, F, F, seed=seed, log_scale_mean=-6.0, log_scale_std=0.3)
    g = torch.Generator().manual_seed(2000 + seed)
    px = 20.0 + 8.0 * torch.rand(n, generator=g)
    py = 20.0 + 8.0 * torch.rand(n, generator=g)
    # pixel centre = f x / z + (W - 1) / 2 for the identity camera
    vis_means = torch.stack([(px - (W - 1) / 2) * z / F, (py - (H - 1) / 2) * z / F, z], dim=1)
    means = torch.empty(P, 3)
    culled = torch.randperm(P, generator=g)[:N_CULLED]
    is_vis = torch.ones(P, dtype=torch.bool)
    is_vis[culled] = False
    means[is_vis] = vis_means
    means[~is_vis] = torch.tensor([0.0, 0.0, -1.0])
    sc.means3D = means.contiguous()
    sc.opacities[:] = 0.3
    return sc, make_camera(W, H, F, F), is_vis.numpy()


def _reference(sc, cam, is_vis, z):
    from oracle import raster_oracle as ro
    inp = helpers.oracle_inputs(sc, cam, use_sh=True)
    ref = ro.render_forward(W=W, H=H, tanfovx=W / (2 * F), tanfovy=H / (2 * F), bg=np.array(BG, np.float32), sh_degree=3, **inp)
    n = len(z)
    b = ref["binning"]
    # the scene is what the case means it to be: one list of n entries whose keys are the bits of z
    assert int((ref["geom"].radii > 0).sum()) == n and b.num_rendered == n
    lens = (b.ranges[:, 1] - b.ranges[:, 0]).astype(np.int64)
    assert lens[TILE_11] == n, lens
    zbits = np.asarray(z, np.float32).view(np.uint32)
    want = np.sort(zbits.astype(np.uint64) | (np.uint64(TILE_11) << np.uint64(32)))
    np.testing.assert_array_equal(np.asarray(b.keys_sorted, dtype=np.uint64), want)
    return inp, ref


def _lists(inp, cam, dev):
    (color, radii, depth, alpha), _ = helpers.hip_forward(inp, cam, BG, 3, dev, requires_grad=True)
    keys, ranges, ncontrib, plist = helpers.hip_export_binning(color)
    return radii.cpu().numpy(), keys, plist, ranges


def _check(z, seed, dev, hooks, caps=(0, 1, ABOVE_ANY_LIST), count=None):
    """the case under every cap of `caps` (0: the rule) against the oracle; count: (force_blocks, reverse) of the counting sort by
    tile, whose chunks then hand the list over in another order than by id"""
    sc, cam, is_vis = _scene(z, seed)
    inp, ref = _reference(sc, cam, is_vis, z)
    if count is not None:
        hooks.count(*count)
    rule = _capacity(2)
    for cap in caps:
        hooks.cap(cap)
        assert _capacity(2) == (cap if cap > 0 else rule)
        radii, keys, plist, ranges = _lists(inp, cam, dev)
        np.testing.assert_array_equal(radii, ref["geom"].radii, err_msg=f"cap {cap}")
        np.testing.assert_array_equal(keys, ref["binning"].keys_sorted, err_msg=f"cap {cap}")
        np.testing.assert_array_equal(plist, ref["binning"].point_list, err_msg=f"cap {cap}")
        np.testing.assert_array_equal(ranges, ref["binning"].ranges, err_msg=f"cap {cap}")
    hooks.cap(0)
    return ref


def _uniform_z(n, seed):
    return (2.0 + 6.0 * np.random.default_rng(seed).random(n)).astype(np.float32)


@pytest.mark.parametrize("case", ["2", "63", "64", "65", "511", "513", "wave-1", "wave"])
def test_list_lengths(gpu_device, hooks, case):
    wave = _capacity(0)
    n = {"wave-1": wave - 1, "wave": wave}.get(case) or int(case)
    _check(_uniform_z(n, n), n, gpu_device, hooks)


def test_all_keys_equal(gpu_device, hooks):
    """only the ids differ: the digit comes from the ids; the counting sort hands the list over back to front"""
    z = np.full(700, 3.25, np.float32)
    _check(z, 700, gpu_device, hooks)
    _check(z, 700, gpu_device, hooks, count=(3, 1))


def test_two_depth_values(gpu_device, hooks):
    """two buckets of 350: above the rule's cap; under a cap above n the whole list is ranked inside them"""
    z = np.where(np.random.default_rng(5).permutation(700) < 350, np.float32(2.5), np.float32(6.0)).astype(np.float32)
    assert _capacity(2) < 350 < ABOVE_ANY_LIST
    _check(z, 701, gpu_device, hooks)


@pytest.mark.parametrize("over", [0, 1])
def test_largest_bucket_at_the_cap(gpu_device, hooks, over):
    """one key at 2.0, one at 8.0, cap (+ 1) keys at 4.0 + j ulps: a range of 2^24, the digit is (key - key of 2.0) >> 17, the
    keys at 4.0 share digit 64"""
    cap = _capacity(2)
    m = cap + over
    assert m < (1 << 17) and m + 2 <= _capacity(0)
    bits = np.concatenate([[0x40000000, 0x41000000], 0x40800000 + np.random.default_rng(6 + over).permutation(m)])
    bits = bits[np.random.default_rng(60 + over).permutation(m + 2)]
    _check(_bits_to_z(bits), 900 + over, gpu_device, hooks)


def test_span_shorter_than_the_digit(gpu_device, hooks):
    """keys that differ in their lowest 3 bits only: eight buckets, many ties"""
    bits = 0x40800000 + np.random.default_rng(7).integers(0, 8, 600)
    _check(_bits_to_z(bits), 600, gpu_device, hooks)
    _check(_bits_to_z(bits), 600, gpu_device, hooks, count=(3, 1))


def test_widest_span(gpu_device, hooks):
    z = np.exp(np.random.default_rng(8).uniform(np.log(0.25), np.log(1e30), 600)).astype(np.float32)
    z[0], z[1] = 0.25, 1e30
    _check(z, 601, gpu_device, hooks)


def test_equal_depth_pairs_with_distant_ids(gpu_device, hooks):
    """z[1::2] = z[0::2]: equal keys whose ids are interleaved with the others', in id order and back to front"""
    z = _uniform_z(600, 9)
    z[1::2] = z[0::2]
    _check(z, 602, gpu_device, hooks)
    _check(z, 602, gpu_device, hooks, count=(3, 1))


def test_two_calls_give_identical_lists(gpu_device, hooks):
    z = _uniform_z(800, 10)
    z[1::2] = z[0::2]
    z[:200] = z[0]                                               # one bucket of 200 besides
    sc, cam, is_vis = _scene(z, 603)
    inp, _ = _reference(sc, cam, is_vis, z)
    hooks.count(3, 0)
    for cap in (0, ABOVE_ANY_LIST):
        hooks.cap(cap)
        first, second = _lists(inp, cam, gpu_device), _lists(inp, cam, gpu_device)
        for a, b in zip(first, second):
            np.testing.assert_array_equal(a, b, err_msg=f"cap {cap}")
