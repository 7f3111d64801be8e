"""CPU: the scratch size queries of the scan and sort library (csrc/radix_sort.hip) are host arithmetic.  The scan carves its
per-workgroup partial sums out of `tmp` level by level, and the two forward-geometry calls lend it the sort's scratch
(gt.sort_tmp): that borrow is sound only while the sort's scratch is at least the scan's, at every n."""
import os

import pytest

TILE = 2048                     # elements per scan workgroup
FLAT_BLOCKS = 16384             # workgroups up to which the scan stays on its two-launch route
EDGES = (1, 2, 7, 8, 9, 2047, 2048, 2049, 4096, 4097, 524_288, 524_289, 526_336, 526_337, 1_000_003, 2_097_152, 2_097_153, 3_145_728, 3_145_729,
         4_194_305, 33_554_432, 33_554_433, 33_554_432 + 3 * 2048 + 5)


@pytest.fixture(scope="module")
def lib():
    from opengaussian_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def _sizes():
    ns = {1 << b for b in range(31)} | {2 ** 31 - 1}
    for e in EDGES + (TILE * FLAT_BLOCKS, TILE * TILE, TILE * TILE * 4):
        ns |= {e - 1, e, e + 1}
    return sorted(n for n in ns if 1 <= n < 2 ** 31)


def _blocks(n):
    return -(-n // TILE)


def test_scan_scratch_is_monotone_and_covers_every_level(lib):
    sizes = _sizes()
    assert sizes[0] == 1 and sizes[-1] == 2 ** 31 - 1 and len(sizes) > 60
    prev = 0
    for n in sizes:
        got = int(lib.ogs_selftest_scan_tmp_bytes(n))
        assert got >= prev, f"n={n}: {got} bytes after {prev} for a smaller n"
        prev = got
        need = 4 * _blocks(n)                                   # one partial sum per workgroup
        if _blocks(n) > FLAT_BLOCKS:                            # the partials are scanned in turn: one sum per workgroup of those
            need += 4 * _blocks(_blocks(n))
            assert _blocks(_blocks(n)) <= FLAT_BLOCKS, "a third level: not reachable below 2^31 elements"
        assert got >= need, f"n={n}: {got} bytes, the partial sums alone take {need}"
    assert int(lib.ogs_selftest_scan_tmp_bytes(0)) == int(lib.ogs_selftest_scan_tmp_bytes(1)) > 0
    assert int(lib.ogs_selftest_scan_tmp_bytes(-5)) == int(lib.ogs_selftest_scan_tmp_bytes(1))


def test_sort_scratch_holds_the_scan_that_borrows_it(lib):
    """forward_geometry_impl (csrc/capi.hip) hands gt.sort_tmp to exclusive_scan_u32 over P elements; GeomTmp::carve
    (csrc/ogs_common.h) takes it as `g.sort_tmp = c.take<char>(sort_tmp_bytes(P))`"""
    for n in _sizes():
        sort_bytes, scan_bytes = int(lib.ogs_selftest_radix_tmp_bytes(n)), int(lib.ogs_selftest_scan_tmp_bytes(n))
        assert sort_bytes >= scan_bytes, f"n={n}: the sort's scratch {sort_bytes} is below the scan's {scan_bytes}"
