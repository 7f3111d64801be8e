"""GPU: the exclusive prefix sum of csrc/radix_sort.hip (exclusive_scan_u32) on its own, through the C ABI test hook.  Every offset
the binning phase, densify, the kNN graph and index and connected components write through comes out of it.

Reference: torch on the device in int64 -- cumsum of the (gathered, count-truncated) input minus the input, modulo 2^32 -- which
shares no code with the kernels.  Everything is compared exactly.

Every call
  * writes into an `out` that is poisoned together with a guard region behind it,
  * gets a `tmp` of exactly ogs_selftest_scan_tmp_bytes(n) bytes with a poisoned guard behind it,
  * has its total (when asked for) written into the middle one of three poisoned words,
and the guards, every `out` element at or past the count and the neighbours of the total must come back untouched.

The scan takes one of three routes by size, and each size group pins its route by the launch counts of the profiling hook
(reduce, apply<true>, apply<false>, total kernel): one workgroup (0, 0, 1, 0) up to 2048 elements; two launches (1, 1, 0, 0) up to
16384 workgroups, every workgroup summing the partials before it; above that the partials are scanned in turn (2, 1, 1, and the
total kernel when a total is asked for).  A moved constant fails the test instead of silently testing another path."""
import pytest
import torch

from opengaussian_amd import _lib

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF
POISON = 0x6B5A3C1D
TMP_POISON = 0xA5
GUARD = 4096                                    # words behind out, bytes behind tmp
INVALID_ARG = -1

ONE = (0, 0, 1)                                 # launches: scan_reduce_kernel, scan_apply_kernel<true>, scan_apply_kernel<false>
FLAT = (1, 1, 0)
MULTI = (2, 1, 1)                               # + scan_total_kernel when a total is asked for
LAST_FLAT = 33_554_432                          # 16384 workgroups of 2048
# 524 288 / 524 289: the 256th and 257th workgroup; workgroup b adds up the b partials before it 256 at a time, so the second
# trip of that loop is first taken by the 258th workgroup (b = 257): 526 336 is the last size without one, 526 337 the first with
SIZES = [(n, ONE) for n in (1, 2, 7, 8, 9, 2047, 2048)] + \
        [(n, FLAT) for n in (2049, 4096, 4097, 524_288, 524_289, 526_336, 526_337, 1_000_003, LAST_FLAT)] + \
        [(n, MULTI) for n in (LAST_FLAT + 1, LAST_FLAT + 3 * 2048 + 5)]
ROUTE = dict(SIZES)
ROUTE.update({1500: ONE, 10_000: FLAT})
FAMILIES = ("tiles", "flags", "wrap")
LARGE = 30_000_000                              # from here on: tile counts and wrapping words only

_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """inputs and references are built once per (family, size) and shared; released when the file is done"""
    yield
    import gc
    _CACHE.clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _draw(family, n, dev, salt=0):
    g = torch.Generator(device=dev).manual_seed(n * 7 + FAMILIES.index(family) + 1000 * salt)
    if family == "tiles":                       # tiles touched per Gaussian: 0...300, half of them zero
        v = torch.randint(0, 301, (n,), generator=g, device=dev)
        return (v * (torch.rand(n, generator=g, device=dev) < 0.5)).to(torch.int32)
    if family == "flags":
        return torch.randint(0, 2, (n,), generator=g, device=dev).to(torch.int32)
    return torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, device=dev).to(torch.int32)      # the sum wraps many times


def _as_i32(u):
    """int64 values in [0, 2^32) as the int32 with the same bits"""
    return torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32)


def _reference(elements):
    """(exclusive prefix sums modulo 2^32 as int32 bits [n + 1], the last one being the total): entry c is also the total of
    the first c elements, which is what a device-side count of c must give"""
    x = elements.to(torch.int64) & M32
    inc = torch.cumsum(x, 0)
    excl = torch.cat([(inc - x) & M32, (inc[-1:] & M32)])
    return _as_i32(excl)


def _input(family, n, dev):
    """(input, reference), built once"""
    key = (family, n)
    if key not in _CACHE:
        x = _draw(family, n, dev)
        _CACHE[key] = (x, _reference(x))
    return _CACHE[key]


class _Result:
    pass


def _scan(dev, src, n, gather=None, n_dev=None, total=True, inplace=False):
    """one call of the hook with poisoned, guarded buffers; returns everything the checks look at"""
    lib = _lib.lib()
    r = _Result()
    guard = torch.full((GUARD,), POISON, dtype=torch.int32, device=dev)
    if inplace:
        assert src.numel() == n
        r.out = torch.cat([src, guard])
        in_ptr = r.out.data_ptr()
    else:
        r.out = torch.full((n + GUARD,), POISON, dtype=torch.int32, device=dev)
        in_ptr = src.data_ptr()
    r.tmp_bytes = int(lib.ogs_selftest_scan_tmp_bytes(n))
    r.tmp = torch.full((r.tmp_bytes + GUARD,), TMP_POISON, dtype=torch.uint8, device=dev)
    r.total = torch.full((3,), POISON, dtype=torch.int32, device=dev)
    count = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    _lib.prof_enable(1)
    try:
        r.rc = lib.ogs_selftest_scan_u32(in_ptr, None if gather is None else gather.data_ptr(), r.out.data_ptr(), n,
                                         r.total.data_ptr() + 4 if total else None, None if count is None else count.data_ptr(),
                                         r.tmp.data_ptr(), torch.cuda.current_stream().cuda_stream)
        r.error = lib.ogs_last_error().decode()
        torch.cuda.synchronize()
        prof = _lib.prof_collect()
    finally:
        _lib.prof_enable(0)
    calls = lambda name: prof.get(name, {}).get("calls", 0)
    r.launches = (calls("scan_reduce_kernel"), calls("scan_apply_kernel<true>"), calls("scan_apply_kernel<false>"))
    r.total_launches = calls("scan_total_kernel")
    r.others = sorted(set(prof) - {"scan_reduce_kernel", "scan_apply_kernel<true>", "scan_apply_kernel<false>", "scan_total_kernel"})
    return r


def _check(r, n, count, ref, route, total, what, original=None):
    """ref: _reference() of the elements the scan sees (entry `count` is the total of the first `count`)"""
    assert r.rc == 0, f"{what}: {r.error}"
    assert not r.others, f"{what}: unexpected launches {r.others}"
    assert r.launches == route, f"{what}: launches (reduce, apply<true>, apply<false>) = {r.launches}, the route is {route}"
    assert r.total_launches == (1 if total and route == MULTI else 0), f"{what}: {r.total_launches} total kernels"
    bad = r.out[:count] != ref[:count]
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {count} prefixes differ, the first at {int(bad.nonzero()[0])}"
    if original is None:
        assert bool((r.out[count:n] == POISON).all()), f"{what}: an output at or past the count was written"
    else:
        assert torch.equal(r.out[count:n], original[count:n]), f"{what}: an in-place element at or past the count was written"
    assert bool((r.out[n:] == POISON).all()), f"{what}: the guard behind out was written"
    assert bool((r.tmp[r.tmp_bytes:] == TMP_POISON).all()), f"{what}: the guard behind tmp was written"
    words = r.total.tolist()
    assert words[0] == POISON and words[2] == POISON, f"{what}: a neighbour of the total was written"
    if total:
        assert words[1] == int(ref[count]), f"{what}: total {words[1] & M32} against {int(ref[count]) & M32}"
    else:
        assert words[1] == POISON, f"{what}: a total nobody asked for was written"


# ---- every route, every edge, three input families, with and without the total -------------------------------------------------
@pytest.mark.parametrize("n,family", [(n, f) for n, _ in SIZES for f in FAMILIES if not (n > LARGE and f == "flags")])
def test_scan_matches_cumsum(gpu_device, n, family):
    x, ref = _input(family, n, gpu_device)
    for total in (True, False):
        r = _scan(gpu_device, x, n, total=total)
        _check(r, n, n, ref, ROUTE[n], total, f"{family} n={n} total={total}")


# ---- in place ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 2048, 4097, 524_289, 526_337, LAST_FLAT])
def test_in_place_with_total_on_the_one_workgroup_and_flat_routes(gpu_device, n):
    x, ref = _input("wrap", n, gpu_device)
    r = _scan(gpu_device, x.clone(), n, inplace=True)
    _check(r, n, n, ref, ROUTE[n], True, f"in place n={n}", original=x)


def test_in_place_without_total_on_the_multi_level_route(gpu_device):
    n = LAST_FLAT + 1
    x, ref = _input("wrap", n, gpu_device)
    r = _scan(gpu_device, x.clone(), n, total=False, inplace=True)
    _check(r, n, n, ref, MULTI, False, f"in place n={n}", original=x)


def _assert_refused(r, n, original, message):
    assert r.rc == INVALID_ARG and message in r.error, (r.rc, r.error)
    assert r.launches == (0, 0, 0) and r.total_launches == 0 and not r.others, "a refused call launched something"
    assert torch.equal(r.out[:n], original), "a refused call changed the data"
    assert bool((r.out[n:] == POISON).all()) and bool((r.tmp == TMP_POISON).all()) and r.total.tolist() == [POISON] * 3


def test_in_place_with_total_on_the_multi_level_route_is_refused_before_any_launch(gpu_device):
    """scan_total_kernel adds the last input to the last prefix; in place the input is gone by then"""
    n = LAST_FLAT + 1
    x, _ = _input("wrap", n, gpu_device)
    _assert_refused(_scan(gpu_device, x.clone(), n, inplace=True), n, x, "total with in-place scan unsupported")


@pytest.mark.parametrize("n", [9, 5000])
def test_in_place_with_gather_is_refused_before_any_launch(gpu_device, n):
    """element i reads in[gather[i]], which another thread may already have overwritten with its prefix"""
    x = _draw("tiles", n, gpu_device, salt=1)
    gather = torch.randint(0, n, (n,), device=gpu_device).to(torch.int32)
    for total in (True, False):
        _assert_refused(_scan(gpu_device, x.clone(), n, gather=gather, total=total, inplace=True), n, x,
                        "gather with in-place scan unsupported")


# ---- gather --------------------------------------------------------------------------------------------------------------------
def _gathered(family, n, dev):
    """in of another length m, indices in [0, m) with repeats"""
    m = n // 2 + 3
    src = _draw(family, m, dev, salt=2)
    g = torch.Generator(device=dev).manual_seed(n + 17)
    gather = torch.randint(0, m, (n,), generator=g, device=dev).to(torch.int32)
    return src, gather, _reference(src[gather.to(torch.int64)])


@pytest.mark.parametrize("n", [4097, 524_289, 526_337, LAST_FLAT + 1])
@pytest.mark.parametrize("family", ["tiles", "wrap"])
def test_scan_of_gathered_elements(gpu_device, n, family):
    src, gather, ref = _gathered(family, n, gpu_device)
    r = _scan(gpu_device, src, n, gather=gather)
    _check(r, n, n, ref, ROUTE[n], True, f"gather {family} n={n}")


# ---- a count in device memory --------------------------------------------------------------------------------------------------
COUNTS = [(1500, c) for c in (0, 1, 700, 1500, 5000)] + \
         [(10_000, c) for c in (0, 1, 2047, 2048, 2049, 4096, 9999, 10_000, 20_000)] + \
         [(LAST_FLAT + 1, c) for c in (5, LAST_FLAT, LAST_FLAT + 1)]


@pytest.mark.parametrize("capacity,n_dev", COUNTS)
def test_device_side_count(gpu_device, capacity, n_dev):
    """the launches are sized for the capacity; the count is min(*n_dev, capacity), the total is that of the first `count`
    elements -- the tail is full of large words here, so reading one of them shows -- and no output at or past it is written
    (ogs_common.h promises it, duplicate relies on it)"""
    x, ref = _input("wrap", capacity, gpu_device)
    count = min(n_dev, capacity)
    for total in (True, False):
        r = _scan(gpu_device, x, capacity, n_dev=n_dev, total=total)
        _check(r, capacity, count, ref, ROUTE[capacity], total, f"capacity {capacity} count {n_dev} total={total}")


@pytest.mark.parametrize("n_dev", [0, 4097, 20_000])
def test_device_side_count_with_gather(gpu_device, n_dev):
    """the depth-order scan of the grouped pass: tiles touched gathered through the depth order, which holds only the Gaussians
    the depth sort kept"""
    capacity = 10_000
    src, gather, ref = _gathered("tiles", capacity, gpu_device)
    r = _scan(gpu_device, src, capacity, gather=gather, n_dev=n_dev)
    _check(r, capacity, min(n_dev, capacity), ref, FLAT, True, f"gather, capacity {capacity} count {n_dev}")


def test_device_side_count_in_place(gpu_device):
    capacity, n_dev = 10_000, 4097
    x, ref = _input("wrap", capacity, gpu_device)
    r = _scan(gpu_device, x.clone(), capacity, n_dev=n_dev, inplace=True)
    _check(r, capacity, n_dev, ref, FLAT, True, "in place with a count", original=x)


# ---- nothing to scan -----------------------------------------------------------------------------------------------------------
def test_no_elements(gpu_device):
    x = _draw("tiles", 16, gpu_device)
    for total in (True, False):
        r = _scan(gpu_device, x, 0, total=total)
        assert r.rc == 0, r.error
        assert r.launches == (0, 0, 0) and r.total_launches == 0 and not r.others
        assert bool((r.out == POISON).all()) and bool((r.tmp == TMP_POISON).all())
        assert r.total.tolist() == [POISON, 0 if total else POISON, POISON]
