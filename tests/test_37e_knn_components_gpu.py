"""GPU: connected components of the kNN graph (include/ogs_knn.h: ogs_knn_components) through the C ABI and through
opengaussian_amd.knn.components, against tests/knn_components_restatement.py.

The result is unique, so comp, count, sizes and first must be EQUAL to the restatement's, the zero and -1 tails included; every
output and tmp sits between canaries."""
import numpy as np
import pytest
import torch

from tests import knn_components_cases as cc
from tests import knn_components_restatement as cr

pytestmark = pytest.mark.gpu

GUARD = 256
I_CANARY, B_CANARY = -77777, 0xA5


def _lib():
    from opengaussian_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dev, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)


def _guarded(numel, dtype, fill, dev):
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + numel]


def _intact(buf, numel, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + numel:] == fill).all())


def capi_components(dev, idx, d2=None, max_d2=None, labels=None, with_first=True):
    """ogs_knn_components with canaries around the four outputs and tmp; (comp, count, sizes, first) as NumPy"""
    L = _lib()
    n, K = idx.shape
    it, dt, lt = _dev(idx, dev, torch.int32), _dev(d2, dev, torch.float32), _dev(labels, dev, torch.int32)
    mt = None if max_d2 is None else torch.tensor([max_d2], dtype=torch.float32, device=dev)
    nbytes = int(L.lib().ogs_knn_components_tmp_bytes(n))
    cbuf, comp = _guarded(n, torch.int32, I_CANARY, dev)
    sbuf, sizes = _guarded(n, torch.int32, I_CANARY, dev)
    fbuf, first = _guarded(n, torch.int32, I_CANARY, dev)
    nbuf, count = _guarded(1, torch.int32, I_CANARY, dev)
    tbuf, tmp = _guarded(nbytes, torch.uint8, B_CANARY, dev)
    L.check(L.lib().ogs_knn_components(n, K, L.ptr(it), L.ptr(dt), L.ptr(mt), L.ptr(lt), L.ptr(comp), L.ptr(sizes),
                                       L.ptr(first) if with_first else None, L.ptr(count), L.ptr(tmp), nbytes, _stream()),
            "ogs_knn_components")
    torch.cuda.synchronize()
    assert _intact(cbuf, n, I_CANARY) and _intact(sbuf, n, I_CANARY) and _intact(fbuf, n, I_CANARY), (n, K)
    assert _intact(nbuf, 1, I_CANARY) and _intact(tbuf, nbytes, B_CANARY), (n, K)
    if not with_first:
        assert bool((first == I_CANARY).all())
    return comp.cpu().numpy(), count.cpu().numpy(), sizes.cpu().numpy(), first.cpu().numpy()


NAMES = ("comp", "count", "sizes", "first")


def assert_components(dev, what, idx, d2=None, max_d2=None, labels=None):
    """equal to the restatement, and the same bytes from a second call; returns what the kernel gave"""
    want = cr.components(idx, d2, max_d2, labels)
    got = capi_components(dev, idx, d2, max_d2, labels)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), (what, name)
    again = capi_components(dev, idx, d2, max_d2, labels)
    assert all(np.array_equal(a, g) for a, g in zip(again, got)), (what, "two calls")
    return got


def test_degenerate_sizes_and_slots(gpu_device):
    L = _lib()
    count = torch.full((3,), I_CANARY, dtype=torch.int32, device=gpu_device)
    L.check(L.lib().ogs_knn_components(0, 4, None, None, None, None, None, None, None, L.ptr(count[1:]), None, 0, _stream()), "n = 0")
    assert count.tolist() == [I_CANARY, 0, I_CANARY]
    for slot in (-1, 0, 1, cc.I32.min):                                     # n = 1: nothing, itself, past the end
        got = assert_components(gpu_device, ("n=1", slot), np.array([[slot]], np.int32))
        assert got[0].tolist() == [0] and got[1].tolist() == [1] and got[2].tolist() == [1] and got[3].tolist() == [0]
    got = assert_components(gpu_device, "K=1", np.array([[2], [-1], [-1], [1], [4]], np.int32))
    assert got[0].tolist() == [0, 1, 0, 1, 2]
    none = np.full((300, 3), -1, np.int32)
    got = assert_components(gpu_device, "all -1", none, np.full((300, 3), np.inf, np.float32), 1.0)
    assert got[1][0] == 300 and np.array_equal(got[0], np.arange(300)) and (got[2] == 1).all()
    got = assert_components(gpu_device, "junk", cc.junk_slots())
    assert 10 < got[1][0] < 190
    without = capi_components(gpu_device, cc.junk_slots(), with_first=False)                 # first may be NULL
    assert all(np.array_equal(a, b) for a, b in zip(without[:3], got[:3]))


@pytest.mark.parametrize("cuts", [(), cc.PATH_CUTS])
def test_path_graph(gpu_device, cuts):
    idx, _ = cc.path_graph(cuts=cuts)
    got = assert_components(gpu_device, ("path", cuts), idx)
    assert got[1][0] == len(cuts) + 1 and got[3][0] == 0


@pytest.mark.parametrize("K", [1, 32])
def test_star(gpu_device, K):
    got = assert_components(gpu_device, ("star", K), cc.star(K=K))
    assert got[1][0] == 1 and got[3][0] == 0 and got[2][0] == cc.STAR_N and not got[0].any()


def test_one_way_edge_joins(gpu_device):
    got = assert_components(gpu_device, "one way", cc.one_way())
    assert got[0].tolist() == [0] * 9 + [1]


def _table(dev, pts, K):
    from opengaussian_amd import knn
    idx, d2 = knn.neighbors(torch.from_numpy(pts).to(dev), K)
    return idx.cpu().numpy(), d2.cpu().numpy()


def test_threshold_on_exact_distances(gpu_device):
    pts = cc.lattice()
    n = len(pts)
    idx, d2 = _table(gpu_device, pts, 8)
    below = np.nextafter(np.float32(1), np.float32(0))
    assert assert_components(gpu_device, "d2 == max_d2", idx, d2, 1.0)[1][0] == 2
    assert assert_components(gpu_device, "next float below", idx, d2, below)[1][0] == n
    assert assert_components(gpu_device, "NaN", idx, d2, np.nan)[1][0] == n
    assert assert_components(gpu_device, "across the gap", idx, d2, 4.0)[1][0] == 1
    assert assert_components(gpu_device, "-inf", idx, d2, -np.inf)[1][0] == n
    assert assert_components(gpu_device, "+inf", idx, d2, np.inf)[1][0] == 1
    assert assert_components(gpu_device, "no d2", idx, None, below)[1][0] == 1               # either NULL: distances are ignored
    assert assert_components(gpu_device, "no max_d2", idx, d2, None)[1][0] == 1
    nan_d2 = d2.copy()
    nan_d2[::3] = np.nan                                                    # NaN on the other side of the compare
    assert_components(gpu_device, "NaN d2", idx, nan_d2, 4.0)
    few = pts[:5]                                                           # n <= K: the lists end in idx = -1, d2 = +inf
    idx5, d25 = _table(gpu_device, few, 8)
    assert (idx5 == -1).any() and np.isinf(d25[idx5 == -1]).all()
    assert assert_components(gpu_device, "+inf slots", idx5, d25, np.inf)[1][0] == 1


def test_labels(gpu_device):
    full = cc.lattice(gap_after=())
    n = len(full)
    idx, d2 = _table(gpu_device, full, 8)
    lab = cc.checkerboard_labels(full)
    got = assert_components(gpu_device, "two classes", idx, d2, 2.0, lab)
    assert got[1][0] == 2 and got[2][:2].sum() == n
    assert assert_components(gpu_device, "two classes, d2 <= 1", idx, d2, 1.0, lab)[1][0] == n
    holes = cc.checkerboard_labels(full, holes=15)
    got = assert_components(gpu_device, "holes", idx, d2, 2.0, holes)
    assert ((got[0] == -1) == (holes == -1)).all() and got[2].sum() == n - 15
    got = assert_components(gpu_device, "wall", idx, d2, 2.0, cc.wall_labels(full))
    assert got[1][0] == 2
    assert_components(gpu_device, "labels, no distances", idx, None, None, holes)
    wide = (lab.astype(np.int64) * (cc.I32.max - 1)).astype(np.int32)       # label values are compared, never used as an index
    assert assert_components(gpu_device, "large labels", idx, d2, 2.0, wide)[1][0] == 2
    got = assert_components(gpu_device, "all inactive", idx, d2, 2.0, np.full(n, -1, np.int32))
    assert got[1][0] == 0 and (got[0] == -1).all() and not got[2].any() and (got[3] == -1).all()
    assert assert_components(gpu_device, "min label", idx, d2, 2.0, np.full(n, cc.I32.min, np.int32))[1][0] == 0


@pytest.mark.parametrize("n,K", cc.TABLE_SIZES)
def test_real_tables(gpu_device, n, K):
    idx, d2 = _table(gpu_device, cc.blobs(n, 100 + n + K), K)
    thr = cc.threshold_of(d2)
    lab = np.random.default_rng(n + K).integers(-1, 3, n).astype(np.int32)
    few = assert_components(gpu_device, (n, K, "no threshold"), idx)
    many = assert_components(gpu_device, (n, K, "threshold"), idx, d2, thr)
    assert few[1][0] < many[1][0]
    assert_components(gpu_device, (n, K, "threshold and labels"), idx, d2, thr, lab)
    # the slots of a row in another order: the same bytes
    sidx, sd2 = cc.permute_slots(idx, d2, n)
    assert all(np.array_equal(a, b) for a, b in zip(capi_components(gpu_device, sidx, sd2, thr), many)), (n, K, "slot order")
    # the rows renumbered: the same partition
    pidx, pd2, pos = cc.permute_rows(idx, d2, n + 1)
    moved = assert_components(gpu_device, (n, K, "rows renumbered"), pidx, pd2, thr)
    assert moved[1][0] == many[1][0] and np.array_equal(cr.canonical(moved[0][pos]), cr.canonical(many[0]))
    assert np.array_equal(np.sort(moved[2]), np.sort(many[2]))


def test_public_wrapper(gpu_device):
    from opengaussian_amd import knn
    pts = cc.blobs(1000, 5)
    it, dt = knn.neighbors(torch.from_numpy(pts).to(gpu_device), 8)
    idx, d2 = it.cpu().numpy(), dt.cpu().numpy()
    thr = cc.threshold_of(d2)
    lab = np.random.default_rng(1).integers(-1, 4, 1000)
    want = cr.components(idx, d2, thr, lab)
    for max_d2 in (float(thr), torch.tensor(float(thr), device=gpu_device), torch.tensor([float(thr)], device=gpu_device)):
        got = knn.components(it, dt, max_d2, torch.from_numpy(lab).to(gpu_device))
        assert [g.dtype for g in got] == [torch.int32] * 4 and [tuple(g.shape) for g in got] == [(1000,), (1,), (1000,), (1000,)]
        assert all(g.is_cuda for g in got) and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    got = knn.components(it.to(torch.int64))                                # other integer types are converted
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, cr.components(idx)))
    empty = knn.components(torch.zeros((0, 4), dtype=torch.int32, device=gpu_device))
    assert empty[1].tolist() == [0] and empty[0].numel() == 0


def test_bad_arguments_are_errors(gpu_device):
    L = _lib()
    lib, s = L.lib(), _stream()
    n, K = 10, 2
    idx = torch.zeros((n, K), dtype=torch.int32, device=gpu_device)
    b = torch.full((64,), I_CANARY, dtype=torch.int32, device=gpu_device)
    tmp = torch.empty(1 << 16, dtype=torch.uint8, device=gpu_device)
    p, big = L.ptr(b), 1 << 16
    assert lib.ogs_knn_components(-1, K, L.ptr(idx), None, None, None, p, p, p, p, L.ptr(tmp), big, s) == -1
    assert lib.ogs_knn_components(n, 0, L.ptr(idx), None, None, None, p, p, p, p, L.ptr(tmp), big, s) == -1
    assert lib.ogs_knn_components(1 << 27, 16, L.ptr(idx), None, None, None, p, p, p, p, L.ptr(tmp), big, s) == -1     # n * K = 2^31
    assert lib.ogs_knn_components(n, K, None, None, None, None, p, p, p, p, L.ptr(tmp), big, s) == -1
    assert lib.ogs_knn_components(n, K, L.ptr(idx), None, None, None, None, p, p, p, L.ptr(tmp), big, s) == -1
    assert lib.ogs_knn_components(n, K, L.ptr(idx), None, None, None, p, None, p, p, L.ptr(tmp), big, s) == -1
    assert lib.ogs_knn_components(n, K, L.ptr(idx), None, None, None, p, p, p, None, L.ptr(tmp), big, s) == -1
    assert lib.ogs_knn_components(0, K, None, None, None, None, None, None, None, None, None, 0, s) == -1              # count is always needed
    assert lib.ogs_knn_components(n, K, L.ptr(idx), None, None, None, p, p, p, p, None, big, s) == -1
    assert lib.ogs_knn_components(n, K, L.ptr(idx), None, None, None, p, p, p, p, L.ptr(tmp), 8, s) == -1 and b"tmp" in lib.ogs_last_error()
    torch.cuda.synchronize()
    assert bool((b == I_CANARY).all())                                      # none of these calls wrote anything


def test_status_word_is_clean_after_the_module(gpu_device):
    torch.cuda.synchronize()
    assert _lib().lib().ogs_check_async_status() == 0
