"""GPU: the stable LSD radix sort of the binning phase (keys bit-exact, ties by index) on its own,
through the C ABI test hook -- both implementations (three launches per pass; one launch per pass with decoupled look-back)
against torch's stable sort, at ragged sizes around the tile boundaries, every digit split and adversarial key sets."""
import ctypes as C

import pytest
import torch

from opengaussian_amd import _lib

pytestmark = pytest.mark.gpu


def _sort(keys, key_bits, variant, dev, items=0):
    lib = _lib.lib()
    n = keys.numel()
    tmp = torch.empty(int(lib.ogs_selftest_radix_tmp_bytes(n)), dtype=torch.uint8, device=dev)
    k = [keys.clone(), torch.full_like(keys, -1)]
    v = [torch.arange(n, dtype=torch.int32, device=dev), torch.full((n,), -1, dtype=torch.int32, device=dev)]
    res = C.c_int32(-1)
    _lib.check(lib.ogs_selftest_radix_sort(k[0].data_ptr(), v[0].data_ptr(), k[1].data_ptr(), v[1].data_ptr(), n, key_bits, variant,
                                           items, None, tmp.data_ptr(), C.byref(res), torch.cuda.current_stream().cuda_stream),
               "radix")
    torch.cuda.synchronize()
    return k[res.value], v[res.value]


def _check(keys, key_bits, dev, what):
    mask = (1 << key_bits) - 1
    want_k, want_v = torch.sort(keys.to(torch.int64) & 0xFFFFFFFF & mask, stable=True)
    for variant in (0, 1):
        k, v = _sort(keys, key_bits, variant, dev)
        got_digits = k.to(torch.int64) & 0xFFFFFFFF & mask
        assert torch.equal(got_digits, want_k), f"{what}: keys, variant {variant}"
        assert torch.equal(v.to(torch.int64), want_v), f"{what}: stable order (ties by index), variant {variant}"
        assert torch.equal(k, keys[v.to(torch.int64)]), f"{what}: keys travel with their values, variant {variant}"


@pytest.mark.parametrize("n", [1, 2, 63, 64, 255, 1023, 1024, 1025, 4095, 4096, 4097, 100_000, 262_144, 262_145, 1_000_003])
def test_radix_sort_matches_stable_sort_full_keys(gpu_device, n):
    g = torch.Generator().manual_seed(n)
    depth = torch.rand(n, generator=g) * 99.8 + 0.2                      # positive view depths -> their bit patterns
    _check(depth.view(torch.int32).to(gpu_device), 32, gpu_device, f"depth bits n={n}")
    ties = torch.randint(0, 7, (n,), generator=g, dtype=torch.int32)     # heavy ties: stability carries the order
    _check(ties.to(gpu_device), 32, gpu_device, f"ties n={n}")


@pytest.mark.parametrize("key_bits", [1, 4, 7, 8, 9, 11, 13, 16, 17, 24, 25, 30, 31])      # 30: the 8/8/8/6 plan of the kNN box sort
def test_radix_sort_every_digit_split(gpu_device, key_bits):
    n = 70_001
    g = torch.Generator().manual_seed(key_bits)
    keys = torch.randint(0, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int32) & ((1 << key_bits) - 1)
    _check(keys.to(gpu_device), key_bits, gpu_device, f"{key_bits}-bit tile ids")


def test_radix_sort_adversarial_keys(gpu_device):
    n = 300_007
    dev = gpu_device
    _check(torch.zeros(n, dtype=torch.int32, device=dev), 32, dev, "all equal")                 # one digit run spans every tile
    _check(torch.arange(n, dtype=torch.int32, device=dev).flip(0).contiguous(), 32, dev, "descending")
    _check(torch.arange(n, dtype=torch.int32, device=dev), 32, dev, "already sorted")
    alt = (torch.arange(n, device=dev) % 2).to(torch.int32) * 0x7FFFFFFF
    _check(alt.contiguous(), 32, dev, "two extreme values alternating")


def _sort_drop(keys, key_bits, variant, dev, n_dev=None):
    lib = _lib.lib()
    n = keys.numel()
    tmp = torch.empty(int(lib.ogs_selftest_radix_tmp_bytes(n)), dtype=torch.uint8, device=dev)
    k = [keys.clone(), torch.full_like(keys, -1)]
    v = [torch.arange(n, dtype=torch.int32, device=dev), torch.full((n,), -1, dtype=torch.int32, device=dev)]
    res = C.c_int32(-1)
    _lib.check(lib.ogs_selftest_radix_sort(k[0].data_ptr(), v[0].data_ptr(), k[1].data_ptr(), v[1].data_ptr(), n, key_bits, variant | 2,
                                           0, None if n_dev is None else n_dev.data_ptr(), tmp.data_ptr(), C.byref(res),
                                           torch.cuda.current_stream().cuda_stream), "radix")
    torch.cuda.synchronize()
    kept = res.value >> 1
    return k[res.value & 1][:kept], v[res.value & 1][:kept], kept


@pytest.mark.parametrize("n,key_bits,frac", [(1, 13, 1.0), (64, 6, 0.5), (1025, 8, 0.9), (4097, 13, 0.52), (100_000, 12, 0.52),
                                            (262_145, 13, 0.3), (1_000_003, 13, 0.52), (300_007, 17, 0.0), (70_001, 9, 1.0)])
def test_radix_sort_drop_mode_is_the_stable_sort_of_the_kept_keys(gpu_device, n, key_bits, frac):
    """Default binning mode: the first pass of the tile sort leaves out the keys 0xFFFFFFFF (the (Gaussian, tile) pairs that cannot
    reach their tile) and the later passes run on the survivors.  Both implementations, one and more passes, none / some / all
    dropped: the result is torch's stable sort of the kept keys, values (= original positions) in step, count reported."""
    g = torch.Generator().manual_seed(n * 31 + key_bits)
    keys = torch.randint(0, 1 << key_bits, (n,), generator=g, dtype=torch.int64)
    dropped = torch.rand(n, generator=g) < frac
    keys_in = torch.where(dropped, torch.full_like(keys, 0xFFFFFFFF), keys).to(torch.int32).to(gpu_device)   # wraps to -1
    keep_idx = torch.nonzero(~dropped).flatten()
    want_k, order = torch.sort(keys[keep_idx], stable=True)
    want_v = keep_idx[order]
    for variant in (0, 1):
        k, v, kept = _sort_drop(keys_in, key_bits, variant, gpu_device)
        assert kept == keep_idx.numel(), (variant, kept, keep_idx.numel())
        assert torch.equal(k.to(torch.int64).cpu() & 0xFFFFFFFF, want_k), f"keys, variant {variant}"
        assert torch.equal(v.to(torch.int64).cpu(), want_v), f"stable order, variant {variant}"


@pytest.mark.parametrize("items", [4, 16])
def test_one_launch_sort_with_a_forced_tile_size_at_4m_keys(gpu_device, items):
    """The configuration of the round-3 memory fault (gpurun_out/ab_S1M-1080p_sweep4.err: one-launch passes with 1024-key tiles
    over the 7.4 M (Gaussian, tile) pairs of the headline scene; DESIGN.md section 3 "the round-3 fault"): 4 Mi + 3 keys through
    radix_onesweep_kernel<4> need 4 x 4097 x 256 status words, which ogs_selftest_radix_tmp_bytes / sort_tmp_bytes must cover.
    The tile size is an explicit argument of the hook now (no environment switch); 16 for the other instantiation."""
    n = (4 << 20) + 3
    g = torch.Generator().manual_seed(items)
    keys = torch.randint(0, 1 << 13, (n,), generator=g, dtype=torch.int32).to(gpu_device)        # 13-bit tile ids, two passes
    k, v = _sort(keys, 13, 1, gpu_device, items=items)
    want_k, want_v = torch.sort(keys.to(torch.int64), stable=True)
    assert torch.equal(k.to(torch.int64), want_k)
    assert torch.equal(v.to(torch.int64), want_v)
    lib = _lib.lib()
    tiles4 = (n + 1023) // 1024
    assert int(lib.ogs_selftest_radix_tmp_bytes(n)) >= 4 * 256 * 4 * tiles4, "scratch must hold four 1024-key-tile status tables"


@pytest.mark.parametrize("variant", [0, 1])
def test_drop_mode_with_a_device_count_of_zero_reports_zero_kept(gpu_device, variant):
    """a deferred-capacity render phase whose view sees nothing runs the tile sort with *n_dev == 0.  Tile 0 of
    the one-launch pass used to return before storing the kept count, which the later passes, the tile ranges and pack read from
    (uninitialised) device memory.  The hook poisons the word first: both implementations must report 0."""
    n = 5000
    keys = torch.randint(0, 1 << 13, (n,), dtype=torch.int32).to(gpu_device)
    n_dev = torch.zeros(1, dtype=torch.int32, device=gpu_device)
    _, _, kept = _sort_drop(keys, 13, variant, gpu_device, n_dev=n_dev)
    assert kept == 0
    n_dev.fill_(1234)                                   # and a true count below the capacity
    k, v, kept = _sort_drop(keys, 13, variant, gpu_device, n_dev=n_dev)
    want_k, order = torch.sort(keys[:1234].to(torch.int64), stable=True)
    assert kept == 1234
    assert torch.equal(k.to(torch.int64), want_k) and torch.equal(v.to(torch.int64), order)


def test_look_back_bound_of_zero_polls_raises(gpu_device):
    """a one-launch pass whose look-back wait runs out used to set a device word nobody read -- wrong order,
    rc 0.  Fault injection through the hook (variant bit 2: bound = 0 polls; with 1000 tiles some workgroup always finds a
    predecessor unpublished): the call must fail with OGS_ERR_DEVICE, the sticky word must be clear afterwards, and the next sort
    must be correct again."""
    lib = _lib.lib()
    n = 1_000_003
    keys = torch.randint(0, 2 ** 31 - 1, (n,), dtype=torch.int32).to(gpu_device)
    with pytest.raises(_lib.OgsError, match="look-back"):
        _sort(keys, 32, 1 | 4, gpu_device, items=4)
    assert lib.ogs_check_async_status() == 0
    _check(keys, 32, gpu_device, "after the injected fault")


# ---- long lists through the three-launch passes ------------------------------------------------------------------------------------
# 2048 workgroups per histogram row is one trip of radix_rowscan_kernel's carry loop; up to 3 Mi keys a workgroup takes 1024 keys
# (radix_hist_kernel<4> / radix_scatter_kernel<4>), above that 2048 (<8>)
LONG = [(2_097_152, 4), (2_097_153, 4), (3_145_728, 4), (3_145_729, 8), (4_194_305, 8)]


def _profiled(call):
    _lib.prof_enable(1)
    try:
        result = call()
        torch.cuda.synchronize()
        return result, _lib.prof_collect()
    finally:
        _lib.prof_enable(0)


def _assert_three_launch_kernels(prof, items, passes, what):
    calls = lambda name: prof.get(name, {}).get("calls", 0)
    other = 12 - items
    assert calls(f"radix_hist_kernel<{items}>") == passes and calls(f"radix_scatter_kernel<{items}>") == passes, (what, sorted(prof))
    assert calls(f"radix_hist_kernel<{other}>") == 0 and calls(f"radix_scatter_kernel<{other}>") == 0, (what, sorted(prof))
    assert calls("radix_rowscan_kernel") == passes and not any(k.startswith("radix_onesweep") for k in prof), (what, sorted(prof))


@pytest.mark.parametrize("n,items", LONG)
def test_three_launch_sort_of_long_lists(gpu_device, n, items):
    """13-bit tile ids (two passes) and all-equal keys (one histogram row carries every count) at the sizes around the second
    trip of the row scan and around the change of the keys per workgroup, which the profiler's launch names pin"""
    dev = gpu_device
    g = torch.Generator(device=dev).manual_seed(n)
    for what, keys in (("tile ids", torch.randint(0, 1 << 13, (n,), generator=g, device=dev).to(torch.int32)),
                       ("all equal", torch.full((n,), 4321, dtype=torch.int32, device=dev))):
        (k, v), prof = _profiled(lambda: _sort(keys, 13, 0, dev))
        _assert_three_launch_kernels(prof, items, 2, f"{what} n={n}")
        want_k, want_v = torch.sort(keys.to(torch.int64), stable=True)
        assert torch.equal(k.to(torch.int64), want_k), f"{what} n={n}: keys"
        assert torch.equal(v.to(torch.int64), want_v), f"{what} n={n}: stable order (ties by index)"


@pytest.mark.parametrize("n", [3_145_729, 4_194_305])
def test_three_launch_drop_sort_of_long_lists(gpu_device, n):
    """the headline tile sort: 2048-key workgroups, drop mode, about half the (Gaussian, tile) pairs dropped"""
    dev = gpu_device
    g = torch.Generator(device=dev).manual_seed(n + 1)
    keys = torch.randint(0, 1 << 13, (n,), generator=g, device=dev)
    dropped = torch.rand(n, generator=g, device=dev) < 0.5
    keys_in = torch.where(dropped, torch.full_like(keys, -1), keys).to(torch.int32)
    keep_idx = torch.nonzero(~dropped).flatten()
    want_k, order = torch.sort(keys[keep_idx], stable=True)
    (k, v, kept), prof = _profiled(lambda: _sort_drop(keys_in, 13, 0, dev))
    _assert_three_launch_kernels(prof, 8, 2, f"drop n={n}")
    assert kept == keep_idx.numel(), (kept, keep_idx.numel())
    assert torch.equal(k.to(torch.int64), want_k), "keys"
    assert torch.equal(v.to(torch.int64), keep_idx[order]), "stable order"


# ---- a count in device memory, nothing dropped: the tile sort of the full-binning deferred render phase --------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("capacity,count", [(5000, 0), (5000, 1), (5000, 1234), (5000, 5000), (5000, 5010), (300_007, 150_003)])
def test_device_side_count_without_drop(gpu_device, variant, capacity, count):
    """The launches are sized for the capacity and the kernels read min(*n_dev, capacity): the first `count` results are the
    stable sort of the first `count` keys.  Every write of a pass lands below the count, so behind it the buffer pair of the
    input still holds the input and the other pair its poison; with a count of 0 nothing is written at all."""
    dev = gpu_device
    lib = _lib.lib()
    g = torch.Generator().manual_seed(capacity + count)
    keys = torch.randint(0, 1 << 13, (capacity,), generator=g, dtype=torch.int32).to(dev)
    ids = torch.arange(capacity, dtype=torch.int32, device=dev)
    tmp = torch.empty(int(lib.ogs_selftest_radix_tmp_bytes(capacity)), dtype=torch.uint8, device=dev)
    k = [keys.clone(), torch.full_like(keys, -1)]
    v = [ids.clone(), torch.full_like(ids, -1)]
    n_dev = torch.tensor([count], dtype=torch.int32, device=dev)
    res = C.c_int32(-1)
    _lib.check(lib.ogs_selftest_radix_sort(k[0].data_ptr(), v[0].data_ptr(), k[1].data_ptr(), v[1].data_ptr(), capacity, 13, variant,
                                           0, n_dev.data_ptr(), tmp.data_ptr(), C.byref(res),
                                           torch.cuda.current_stream().cuda_stream), "radix")
    torch.cuda.synchronize()
    assert res.value == 0, "two passes: the result is in the buffer pair of the input"
    c = min(count, capacity)
    want_k, want_v = torch.sort(keys[:c].to(torch.int64), stable=True)
    assert torch.equal(k[0][:c].to(torch.int64), want_k), "keys"
    assert torch.equal(v[0][:c].to(torch.int64), want_v), "stable order (ties by index)"
    assert torch.equal(k[0][c:], keys[c:]) and torch.equal(v[0][c:], ids[c:]), "a key or value at or past the count was written"
    assert bool((k[1][c:] == -1).all()) and bool((v[1][c:] == -1).all()), "the other buffer pair was written at or past the count"
    if c == 0:
        assert bool((k[1] == -1).all()) and bool((v[1] == -1).all()), "a count of 0 wrote to the poisoned output buffers"
