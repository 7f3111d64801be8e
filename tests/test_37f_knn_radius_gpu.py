"""GPU: radius counts and exact DBSCAN (include/ogs_knn.h: ogs_knn_radius_count, ogs_knn_dbscan) through the C ABI and through
opengaussian_amd.knn, against tests/knn_radius_restatement.py.

The results are unique, so every output must be EQUAL to the restatement's, the zero and -1 tails included, and a second call
must give the same bytes; every output and tmp sits between canaries."""
import numpy as np
import pytest
import torch

from tests import knn_components_cases as cc
from tests import knn_radius_cases as rc
from tests import knn_radius_restatement as rr

pytestmark = pytest.mark.gpu

GUARD = 256
I_CANARY, B_CANARY = -77777, 0xA5
NAMES = ("cluster", "core", "degree", "sizes", "first", "count")


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


def capi_dbscan(dev, pts, eps2, min_pts, labels=None, with_degree=True, with_first=True):
    """ogs_knn_dbscan with canaries around the six outputs and tmp; the six arrays as NumPy, in the order of NAMES"""
    L = _lib()
    n = len(pts)
    pt, lt = _dev(pts, dev, torch.float32), _dev(labels, dev, torch.int32)
    et = torch.tensor([eps2], dtype=torch.float32, device=dev)
    nbytes = int(L.lib().ogs_knn_dbscan_tmp_bytes(n))
    cbuf, cluster = _guarded(n, torch.int32, I_CANARY, dev)
    kbuf, core = _guarded(n, torch.uint8, B_CANARY, dev)
    dbuf, degree = _guarded(n, torch.int32, I_CANARY, dev)
    sbuf, sizes = _guarded(n, torch.int32, I_CANARY, dev)
    fbuf, first = _guarded(n, torch.int32, I_CANARY, dev)
    nbuf, count = _guarded(1, torch.int32, I_CANARY, dev)
    tbuf, tmp = _guarded(nbytes, torch.uint8, B_CANARY, dev)
    L.check(L.lib().ogs_knn_dbscan(n, L.ptr(pt), L.ptr(et), min_pts, L.ptr(lt), L.ptr(cluster), L.ptr(core),
                                   L.ptr(degree) if with_degree else None, L.ptr(sizes), L.ptr(first) if with_first else None,
                                   L.ptr(count), L.ptr(tmp), nbytes, _stream()), "ogs_knn_dbscan")
    torch.cuda.synchronize()
    assert _intact(cbuf, n, I_CANARY) and _intact(kbuf, n, B_CANARY) and _intact(dbuf, n, I_CANARY), n
    assert _intact(sbuf, n, I_CANARY) and _intact(fbuf, n, I_CANARY) and _intact(nbuf, 1, I_CANARY), n
    assert _intact(tbuf, nbytes, B_CANARY), n
    if not with_degree:
        assert bool((degree == I_CANARY).all())
    if not with_first:
        assert bool((first == I_CANARY).all())
    return tuple(t.cpu().numpy() for t in (cluster, core, degree, sizes, first, count))


def assert_dbscan(dev, what, pts, eps2, min_pts, labels=None):
    """equal to the restatement, and the same bytes from a second call; returns what the kernels gave"""
    want = rr.dbscan(pts, eps2, min_pts, labels)
    got = capi_dbscan(dev, pts, eps2, min_pts, labels)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)
    again = capi_dbscan(dev, pts, eps2, min_pts, labels)
    assert all(np.array_equal(a, g) for a, g in zip(again, got)), (what, "two calls")
    return got


def _index(dev, pts):
    L = _lib()
    n = len(pts)
    pt = _dev(pts, dev, torch.float32)
    ibytes, tbytes = int(L.lib().ogs_knn_index_bytes(n)), int(L.lib().ogs_knn_index_build_tmp_bytes(n))
    index = torch.empty(max(ibytes, 1), dtype=torch.uint8, device=dev)
    tmp = torch.empty(max(tbytes, 1), dtype=torch.uint8, device=dev)
    L.check(L.lib().ogs_knn_index_build(n, L.ptr(pt), L.ptr(index), ibytes, L.ptr(tmp), tbytes, _stream()), "ogs_knn_index_build")
    return index


def capi_count(dev, index, n, queries, r2, ref_labels=None, query_labels=None):
    L = _lib()
    m = len(queries)
    qt = _dev(queries, dev, torch.float32)
    rl, ql = _dev(ref_labels, dev, torch.int32), _dev(query_labels, dev, torch.int32)
    rt = torch.tensor([r2], dtype=torch.float32, device=dev)
    nbytes = int(L.lib().ogs_knn_radius_count_tmp_bytes(n, m))
    cbuf, count = _guarded(m, torch.int32, I_CANARY, dev)
    tbuf, tmp = _guarded(nbytes, torch.uint8, B_CANARY, dev)
    L.check(L.lib().ogs_knn_radius_count(n, L.ptr(index), m, L.ptr(qt), L.ptr(rt), L.ptr(rl), L.ptr(ql), L.ptr(count), L.ptr(tmp),
                                         nbytes, _stream()), "ogs_knn_radius_count")
    torch.cuda.synchronize()
    assert _intact(cbuf, m, I_CANARY) and _intact(tbuf, nbytes, B_CANARY), (n, m)
    return count.cpu().numpy()


def assert_count(dev, what, pts, index, queries, r2, ref_labels=None, query_labels=None):
    want = rr.radius_count(pts, queries, r2, ref_labels, query_labels)
    got = capi_count(dev, index, len(pts), queries, r2, ref_labels, query_labels)
    assert got.dtype == np.int32 and np.array_equal(got, want), what
    assert np.array_equal(capi_count(dev, index, len(pts), queries, r2, ref_labels, query_labels), got), (what, "two calls")
    return got


@pytest.fixture(scope="module")
def size_cases():
    return {n: (rc.blobs(n), rc.eps2_of(rc.blobs(n))) for n in rc.DBSCAN_SIZES}


def test_degenerate_sizes(gpu_device):
    L = _lib()
    for min_pts in (1, 2):
        count = torch.full((3,), I_CANARY, dtype=torch.int32, device=gpu_device)
        L.check(L.lib().ogs_knn_dbscan(0, None, None, min_pts, None, None, None, None, None, None, L.ptr(count[1:]), None, 0, _stream()),
                "n = 0")
        assert count.tolist() == [I_CANARY, 0, I_CANARY]
    one = np.array([[0.25, 0.5, 0.75]], np.float32)
    got = assert_dbscan(gpu_device, "n=1, min_pts=1", one, 1.0, 1)
    assert [g.tolist() for g in got] == [[0], [1], [1], [1], [0], [1]]
    got = assert_dbscan(gpu_device, "n=1, min_pts=2", one, 1.0, 2)
    assert [g.tolist() for g in got] == [[-1], [0], [1], [0], [-1], [0]]
    index = _index(gpu_device, one)
    out = torch.full((5,), I_CANARY, dtype=torch.int32, device=gpu_device)
    r2 = torch.ones(1, device=gpu_device)
    L.check(L.lib().ogs_knn_radius_count(0, None, 3, None, None, None, None, L.ptr(out[1:]), None, 0, _stream()), "n = 0")
    L.check(L.lib().ogs_knn_radius_count(1, L.ptr(index), 0, None, L.ptr(r2), None, None, None, None, 0, _stream()), "m = 0")
    assert out.tolist() == [I_CANARY, 0, 0, 0, I_CANARY]


@pytest.mark.parametrize("n", rc.DBSCAN_SIZES)
def test_dbscan_sizes(gpu_device, size_cases, n):
    pts, eps2 = size_cases[n]
    got = assert_dbscan(gpu_device, n, pts, eps2, rc.MIN_PTS)
    assert got[1].any() and not got[1].all() and got[5][0] >= 1
    lab = np.random.default_rng(n).integers(-1, 3, n).astype(np.int32)
    assert_dbscan(gpu_device, (n, "labels"), pts, eps2 * np.float32(4), 3, lab)
    if n == 129:
        without = capi_dbscan(gpu_device, pts, eps2, rc.MIN_PTS, with_degree=False, with_first=False)      # both may be NULL
        assert all(np.array_equal(without[i], got[i]) for i in (0, 1, 3, 5))


@pytest.mark.parametrize("n", rc.COUNT_N)
def test_radius_count_sizes(gpu_device, n):
    pts = cc.blobs(n, 50 + n)
    index = _index(gpu_device, pts)
    r2 = np.float32(0.01)
    rlab = np.random.default_rng(n).integers(-1, 3, n).astype(np.int32)
    for m in rc.COUNT_M:
        q = rc.queries_inside(m, 7 * n + m)
        got = assert_count(gpu_device, (n, m), pts, index, q, r2)
        qlab = np.random.default_rng(m).integers(-1, 3, m).astype(np.int32)
        assert_count(gpu_device, (n, m, "labels"), pts, index, q, np.float32(0.09), rlab, qlab)
        assert_count(gpu_device, (n, m, "+inf"), pts, index, q, np.inf)
        out = rc.queries_outside(m, m)
        assert not assert_count(gpu_device, (n, m, "outside"), pts, index, out, r2).any()
        assert (assert_count(gpu_device, (n, m, "outside, reaching"), pts, index, out, np.float32(40.0)) == n).all()
    if n == 5000:
        assert got.max() > 64                                               # more than one box of rows in reach


def test_threshold_edge_on_a_lattice(gpu_device):
    pts = cc.lattice()
    n = len(pts)
    assert assert_dbscan(gpu_device, "eps2 == 1", pts, 1.0, 1)[5][0] == 2
    got = assert_dbscan(gpu_device, "next float below", pts, rc.BELOW_ONE, 1)
    assert (got[2] == 1).all() and got[5][0] == n
    assert assert_dbscan(gpu_device, "across the gap", pts, 4.0, 1)[5][0] == 1
    for bad in (np.nan, -1.0):
        got = assert_dbscan(gpu_device, bad, pts, bad, 1)
        assert not got[2].any() and not got[1].any() and (got[0] == -1).all() and got[5][0] == 0
    got = assert_dbscan(gpu_device, "+inf", pts, np.inf, n)
    assert (got[2] == n).all() and got[5][0] == 1 and got[3][0] == n
    twice = np.concatenate((pts, pts[:30]))                                 # coincident rows: eps2 = 0 counts exactly those
    got = assert_dbscan(gpu_device, "eps2 == 0", twice, 0.0, 2)
    assert got[2].tolist() == [2] * 30 + [1] * (n - 30) + [2] * 30 and got[5][0] == 30
    index = _index(gpu_device, pts)
    assert assert_count(gpu_device, "count, eps2 == 1", pts, index, pts, 1.0).max() == 5
    assert (assert_count(gpu_device, "count, below", pts, index, pts, rc.BELOW_ONE) == 1).all()
    for bad in (np.nan, -1.0):
        assert not assert_count(gpu_device, ("count", bad), pts, index, pts, bad).any()
    assert (assert_count(gpu_device, "count, +inf", pts, index, pts, np.inf) == n).all()


def test_min_pts_extremes(gpu_device):
    from opengaussian_amd import knn
    pts = rc.graph_blobs()
    n = len(pts)
    got = assert_dbscan(gpu_device, "min_pts = 1", pts, rc.GRAPH_EPS2, 1)
    assert got[1].all() and (got[0] >= 0).all()
    xyz = torch.from_numpy(pts).to(gpu_device)
    idx, d2 = knn.neighbors(xyz, 32)                                        # at most 31 others within eps: the table holds them all
    comp, count, sizes, first = knn.components(idx, d2, float(rc.GRAPH_EPS2))
    assert np.array_equal(comp.cpu().numpy(), got[0]) and count.item() == got[5][0]
    assert np.array_equal(sizes.cpu().numpy(), got[3]) and np.array_equal(first.cpu().numpy(), got[4])
    got = assert_dbscan(gpu_device, "min_pts = n + 1", pts, np.inf, n + 1)
    assert got[5][0] == 0 and (got[0] == -1).all() and not got[1].any() and (got[2] == n).all() and (got[4] == -1).all()


def test_border_rules(gpu_device):
    pts = rc.two_blocks()
    cluster, core, degree, sizes, first, count = assert_dbscan(gpu_device, "two blocks", pts, 1.0, 4)
    assert count[0] == 2 and first[:2].tolist() == [1, 10] and sizes[:2].tolist() == [10, 9]
    assert not core[[0, 2, 6, 8, 18]].any() and cluster[[0, 2, 6, 8]].tolist() == [0] * 4      # corners are borders
    assert cluster[18] == cluster[7] == 0 and cluster[10] == 1             # (3, 1) goes to the smaller core row, bridges nothing
    assert cluster[19:].tolist() == [-1, -1] and degree[19:].tolist() == [2, 2]        # non-core neighbours only: noise
    back = assert_dbscan(gpu_device, "two blocks, reversed", pts[::-1].copy(), 1.0, 4)[0][::-1]
    assert back[18] == back[10] != back[7] and back[19:].tolist() == [-1, -1]


@pytest.mark.parametrize("cuts", [(), cc.PATH_CUTS])
def test_long_chain(gpu_device, cuts):
    pts, p = rc.path_points(cuts)
    got = assert_dbscan(gpu_device, ("path", cuts), pts, 1.0, 2)
    assert got[5][0] == len(cuts) + 1 and got[1].all() and got[4][0] == 0


def test_coincident_points_contend_for_one_root(gpu_device):
    pts = rc.coincident()
    got = assert_dbscan(gpu_device, "coincident", pts, 0.0, 2)
    assert (got[2][:-1] == rc.COINCIDENT).all() and got[2][-1] == 1 and got[5][0] == 1 and got[3][0] == rc.COINCIDENT
    assert not got[0][:-1].any() and got[0][-1] == -1
    got = assert_dbscan(gpu_device, "coincident, eps2 = 1", pts, 1.0, rc.COINCIDENT + 1)       # equality: the last row is in reach
    assert got[1].all() and (got[2] == rc.COINCIDENT + 1).all() and not got[0].any() and got[3][0] == rc.COINCIDENT + 1


def test_labels(gpu_device):
    full = cc.lattice(gap_after=())
    n = len(full)
    lab = cc.checkerboard_labels(full)
    got = assert_dbscan(gpu_device, "two classes", full, 2.0, 1, lab)
    assert got[5][0] == 2 and got[3][:2].sum() == n
    assert assert_dbscan(gpu_device, "two classes, eps2 = 1", full, 1.0, 1, lab)[5][0] == n
    holes = cc.checkerboard_labels(full, holes=15)
    got = assert_dbscan(gpu_device, "holes", full, 2.0, 1, holes)
    assert ((got[0] == -1) == (holes == -1)).all() and got[3].sum() == n - 15 and not got[2][holes == -1].any()
    assert assert_dbscan(gpu_device, "wall", full, 1.0, 2, cc.wall_labels(full))[5][0] == 2
    wide = (lab.astype(np.int64) * (rc.I32.max - 1)).astype(np.int32)       # label values are compared, never used as an index
    assert assert_dbscan(gpu_device, "large labels", full, 2.0, 1, wide)[5][0] == 2
    got = assert_dbscan(gpu_device, "all inactive", full, 2.0, 1, np.full(n, -1, np.int32))
    assert got[5][0] == 0 and (got[0] == -1).all() and not got[3].any() and (got[4] == -1).all() and not got[2].any()
    assert assert_dbscan(gpu_device, "min label", full, 2.0, 1, np.full(n, rc.I32.min, np.int32))[5][0] == 0
    index = _index(gpu_device, full)
    q = full[::3] + np.float32(0.25)
    both = assert_count(gpu_device, "count, labels", full, index, q, 2.0, wide, wide[::3])
    neither = assert_count(gpu_device, "count, no labels", full, index, q, 2.0)
    assert (both <= neither).all() and (both < neither).any() and both.any()
    assert not assert_count(gpu_device, "count, inactive queries", full, index, q, 2.0, lab, np.full(len(q), -1, np.int32)).any()
    assert not assert_count(gpu_device, "count, inactive rows", full, index, q, 2.0, np.full(n, -1, np.int32), lab[::3]).any()


def test_permuted_input_gives_the_same_partition(gpu_device, size_cases):
    pts, eps2 = size_cases[4097]
    lab = np.random.default_rng(9).integers(-1, 2, len(pts)).astype(np.int32)
    for labels in (None, lab):
        base = capi_dbscan(gpu_device, pts, eps2, rc.MIN_PTS, labels)
        ppts, plab, pos = rc.permuted(pts, labels, 4098)
        moved = assert_dbscan(gpu_device, ("permuted", labels is not None), ppts, eps2, rc.MIN_PTS, plab)
        fixed = ~rc.ambiguous_borders(pts, eps2, rc.MIN_PTS, labels)        # every row but a border between two clusters
        assert moved[5][0] == base[5][0] and np.array_equal(moved[1][pos], base[1]) and np.array_equal(moved[2][pos], base[2])
        assert np.array_equal(rr.canonical(moved[0][pos][fixed]), rr.canonical(base[0][fixed]))


def test_public_wrappers(gpu_device, size_cases):
    from opengaussian_amd import knn
    pts, eps2 = size_cases[4097]
    eps = float(np.sqrt(np.float64(eps2)))
    e2 = np.float32(eps) * np.float32(eps)                                  # the square as the wrapper makes it
    lab = np.random.default_rng(2).integers(-1, 4, len(pts))
    xyz, labels = torch.from_numpy(pts).to(gpu_device), torch.from_numpy(lab).to(gpu_device)
    want = rr.dbscan(pts, e2, rc.MIN_PTS, lab)
    for e in (eps, torch.tensor(eps, device=gpu_device), torch.tensor([eps], device=gpu_device)):
        got = knn.dbscan(xyz, e, rc.MIN_PTS, labels)
        assert isinstance(got, knn.Dbscan) and got.core.dtype is torch.bool and all(t.is_cuda for t in got)
        for name, w in zip(NAMES, want):
            assert np.array_equal(getattr(got, name).cpu().numpy().astype(w.dtype), w), name
    empty = knn.dbscan(torch.zeros((0, 3), device=gpu_device), 1.0, 3)
    assert empty.count.tolist() == [0] and empty.cluster.numel() == 0
    q = rc.queries_inside(300, 3)
    qt = torch.from_numpy(q).to(gpu_device)
    index = knn.Index(xyz)
    assert np.array_equal(index.radius_count(qt, eps).cpu().numpy(), rr.radius_count(pts, q, e2))
    qlab = np.random.default_rng(4).integers(-1, 4, len(q))
    got = index.radius_count(qt, torch.tensor(eps, device=gpu_device), labels, torch.from_numpy(qlab).to(gpu_device))
    assert got.dtype is torch.int32 and np.array_equal(got.cpu().numpy(), rr.radius_count(pts, q, e2, lab, qlab))
    assert np.array_equal(knn.radius_count(xyz, eps, qt).cpu().numpy(), rr.radius_count(pts, q, e2))
    assert np.array_equal(knn.radius_count(xyz, eps, labels=labels).cpu().numpy(), want[2])        # the set against itself
    with pytest.raises(ValueError):
        index.radius_count(qt, eps, labels=labels)
    with pytest.raises(ValueError):
        knn.dbscan(xyz, eps, 0)
    with pytest.raises(ValueError):
        knn.dbscan(xyz, -1.0, 3)


def test_bad_arguments_are_errors(gpu_device):
    L = _lib()
    lib, s = L.lib(), _stream()
    n = 10
    pts = torch.zeros((n, 3), dtype=torch.float32, device=gpu_device)
    e = torch.ones(1, dtype=torch.float32, device=gpu_device)
    b = torch.full((64,), I_CANARY, dtype=torch.int32, device=gpu_device)
    tmp = torch.empty(1 << 20, dtype=torch.uint8, device=gpu_device)
    index = _index(gpu_device, np.zeros((n, 3), np.float32))
    P, E, p, T, I, big = L.ptr(pts), L.ptr(e), L.ptr(b), L.ptr(tmp), L.ptr(index), 1 << 20
    assert lib.ogs_knn_dbscan(-1, P, E, 1, None, p, p, p, p, p, p, T, big, s) == -1
    assert lib.ogs_knn_dbscan(1 << 31, P, E, 1, None, p, p, p, p, p, p, T, big, s) == -1
    assert lib.ogs_knn_dbscan(n, P, E, 0, None, p, p, p, p, p, p, T, big, s) == -1 and b"min_pts" in lib.ogs_last_error()
    assert lib.ogs_knn_dbscan(n, None, E, 1, None, p, p, p, p, p, p, T, big, s) == -1
    assert lib.ogs_knn_dbscan(n, P, None, 1, None, p, p, p, p, p, p, T, big, s) == -1
    assert lib.ogs_knn_dbscan(n, P, E, 1, None, None, p, p, p, p, p, T, big, s) == -1
    assert lib.ogs_knn_dbscan(n, P, E, 1, None, p, None, p, p, p, p, T, big, s) == -1
    assert lib.ogs_knn_dbscan(n, P, E, 1, None, p, p, p, None, p, p, T, big, s) == -1
    assert lib.ogs_knn_dbscan(n, P, E, 1, None, p, p, p, p, p, None, T, big, s) == -1
    assert lib.ogs_knn_dbscan(0, None, None, 1, None, None, None, None, None, None, None, None, 0, s) == -1       # count is always needed
    assert lib.ogs_knn_dbscan(n, P, E, 1, None, p, p, p, p, p, p, None, big, s) == -1
    assert lib.ogs_knn_dbscan(n, P, E, 1, None, p, p, p, p, p, p, T, 8, s) == -1 and b"tmp" in lib.ogs_last_error()
    assert lib.ogs_knn_dbscan_tmp_bytes(0) == 0 and lib.ogs_knn_dbscan_tmp_bytes(-3) == 0 and lib.ogs_knn_dbscan_tmp_bytes(1 << 31) == 0
    assert lib.ogs_knn_radius_count(-1, I, n, P, E, None, None, p, T, big, s) == -1
    assert lib.ogs_knn_radius_count(n, I, -1, P, E, None, None, p, T, big, s) == -1
    assert lib.ogs_knn_radius_count(n, I, 1 << 31, P, E, None, None, p, T, big, s) == -1
    assert lib.ogs_knn_radius_count(n, I, n, P, E, p, None, p, T, big, s) == -1 and b"labels" in lib.ogs_last_error()
    assert lib.ogs_knn_radius_count(n, I, n, P, E, None, p, p, T, big, s) == -1
    assert lib.ogs_knn_radius_count(n, None, n, P, E, None, None, p, T, big, s) == -1
    assert lib.ogs_knn_radius_count(n, I, n, None, E, None, None, p, T, big, s) == -1
    assert lib.ogs_knn_radius_count(n, I, n, P, None, None, None, p, T, big, s) == -1
    assert lib.ogs_knn_radius_count(n, I, n, P, E, None, None, None, T, big, s) == -1
    assert lib.ogs_knn_radius_count(n, I, n, P, E, None, None, p, None, big, s) == -1
    assert lib.ogs_knn_radius_count(n, I, n, P, E, None, None, p, T, 8, s) == -1 and b"tmp" in lib.ogs_last_error()
    assert lib.ogs_knn_radius_count_tmp_bytes(0, 5) == 0 and lib.ogs_knn_radius_count_tmp_bytes(5, 0) == 0
    torch.cuda.synchronize()
    assert bool((b == I_CANARY).all())                                      # none of these calls wrote anything


def test_status_word_is_clean_after_the_module(gpu_device):
    torch.cuda.synchronize()
    assert _lib().lib().ogs_check_async_status() == 0
