"""GPU: the k-means kernels (opengaussian_amd/csrc/kmeans.hip) past one trip per workgroup, at block / wave / width / size-limit
edges, on exact ties and off the origin.

Truth is oracle/kmeans_oracle.py (fp32, the kernel's operation order) or float64 NumPy (tests/helpers.py::
kmeans_step_attribution, kmeans_final_ids_attribution); two GPU results are compared with each other only where bit-identity is
the claim.  One shape per kernel of the table above launch_pass:

    A1  (k, d) = (10, 6), k_active = 7, id_offset = 130     kmeans_gemm_pass_kernel, CB = 1
    A4  (64, 9)                                             kmeans_gemm_pass_kernel, CB = 4
    B   (200, 6); (160, 9) with k_active = 100              kmeans_accum_bf16_kernel / kmeans_mfma_pass_kernel, DT > 0
    C   (64, 7); (256, 15)                                  kmeans_mfma_pass_kernel, DT = 0
    D   (300, 9); (8, 16)                                   kmeans_lds_pass_kernel

Trips: a pass launches min(ceil(N / 256), 1024) workgroups which grid-stride over the 256-row blocks.  N = 300 001 is 1 172 blocks:
workgroups 0..147 make TWO trips, the last block holds 225 rows.  N = 600 077 is 2 345 blocks: workgroups 0..296 make THREE trips
(both LDS buffers of the bf16 accumulate are reused), the last block holds 141 rows.

Wall time of this module on an MI355X host: 40 s (the CPU oracle dominates; the slowest case, C (256, 15) at N = 600 077, 10 s).
"""
import numpy as np
import pytest
import torch

from oracle import kmeans_oracle as ko
from tests import helpers

pytestmark = pytest.mark.gpu

assert_centers_close = helpers.assert_kmeans_centers_close
KM_TIE = helpers.KM_TIE

#        name        k    d   k_active  id_offset
PATHS = {
    "A1":        (10,  6,  7,    130),
    "A4":        (64,  9,  None, 0),
    "B-200x6":   (200, 6,  None, 0),
    "B-160x9":   (160, 9,  100,  0),
    "C-64x7":    (64,  7,  None, 0),
    "C-256x15":  (256, 15, None, 0),
    "D-300x9":   (300, 9,  None, 0),
    "D-8x16":    (8,   16, None, 0),
}
FIXED_ORDER = ["A1", "A4", "B-200x6", "B-160x9", "C-64x7", "C-256x15"]      # paths whose summation order is fixed (not D)


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31)))


def _rows_as_centres(feat, k, g):
    return feat[torch.randperm(feat.shape[0], generator=g)[:k]].clone()


def _oracle_ids(x, c):
    """ko._argmin_sqdist in the oracle's own 10 000-row chunks (its [rows, k] fp32 matrix does not grow with N)"""
    x = np.ascontiguousarray(x, np.float32)
    c = np.ascontiguousarray(c, np.float32)
    return np.concatenate([ko._argmin_sqdist(x[lo:lo + ko.CHUNK], c) for lo in range(0, len(x), ko.CHUNK)] or
                          [np.zeros(0, np.int64)])


def _f64_ids(x, c):
    """float64 first-minimum nearest centre and the distance to it, per row"""
    dmin, amin, _ = helpers._km_row_distances(np.asarray(x, np.float64), np.asarray(c, np.float64), [])
    return amin, dmin


def _accumulate(fdev, cdev, k_active=None):
    """ogs_kmeans_accumulate: the summed [k, d+1] table (sums | counts) of ONE accumulate pass, as float64 NumPy"""
    from opengaussian_amd import _lib
    from opengaussian_amd._lib import ptr
    lib = _lib.lib()
    N, d = int(fdev.shape[0]), int(fdev.shape[1])
    k = int(cdev.shape[0])
    assert fdev.is_contiguous() and cdev.is_contiguous() and fdev.dtype == cdev.dtype == torch.float32
    table = torch.full((k, d + 1), float("nan"), dtype=torch.float32, device=fdev.device)
    tmp = torch.empty(int(lib.ogs_kmeans_tmp_bytes(N, d, k)), dtype=torch.uint8, device=fdev.device)
    _lib.check(lib.ogs_kmeans_accumulate(ptr(fdev), N, d, ptr(cdev), k, int(k if k_active is None else k_active), ptr(table),
                                         ptr(tmp), torch.cuda.current_stream().cuda_stream), "ogs_kmeans_accumulate")
    torch.cuda.synchronize()
    return table.cpu().numpy().astype(np.float64)


def _assert_counts_are_the_assignment(table, ids, N, k, what):
    """The count column of an accumulate pass against the ids of the assign pass on the same centres: integers below 2^24, so
    EXACT, and they sum to N.  A dropped, repeated or stale block of a trip loop cannot survive this.  The two kernels of every
    path evaluate the same fp32 distance expression in the same order (A: the same GEMM kernel; B: the fused-multiply-add scan
    over the centres in both; C, D: nearest_centre<0> in both), so they cannot disagree on a row, a float64 tie below KM_TIE
    included: no row is exempt from this comparison."""
    counts = table[:, -1]
    assert counts.sum() == N, f"{what}: the count column sums to {counts.sum()}, not to N = {N}"
    np.testing.assert_array_equal(counts, np.bincount(ids, minlength=k).astype(np.float64), err_msg=f"{what}: counts != bincount(assign)")


# ---- 1. several trips per workgroup -----------------------------------------------------------------------------------------------
TRIP_CASES = [(name, 300_001) for name in PATHS] + [(name, 600_077) for name in ("B-200x6", "B-160x9", "C-256x15", "A4")]


@pytest.mark.parametrize("name,N", TRIP_CASES, ids=[f"{n}-{N}" for n, N in TRIP_CASES])
def test_trip_loops_follow_the_oracle_step_by_step(gpu_device, name, N):
    """Two Lloyd iterations, one at a time, EACH started from the oracle's centres (the scheme of
    test_lloyd_follows_reference_trajectory_step_by_step: a near-tie flip cannot cascade), at an N where workgroups make two
    (300 001) or three (600 077) trips.  Per iteration: the ids the iteration uses are float64 nearest centres up to KM_TIE and
    every centre is the float64 mean of its members and agrees with the oracle's (kmeans_step_attribution); the count column of
    ogs_kmeans_accumulate on the same centres is exactly bincount(assign ids).  Then one fused iters = 3 call lands on the replay
    of its own single iterations to 2e-6 (as attribute_root_run)."""
    from opengaussian_amd import kmeans
    k, d, k_active, off = PATHS[name]
    ka = k if k_active is None else k_active
    assert (N + 255) // 256 > (2048 if N > 600_000 else 1024), "the case must force the trips it is named for"
    g = _gen(k, d, N)
    feat = torch.rand(N, d, generator=g)
    init = _rows_as_centres(feat, k, g)
    nch = N // 10000 + 1
    fdev = feat.to(gpu_device)
    X = feat.numpy()
    c_prev, ids_prev_ref = init.numpy().copy(), None
    for t in range(2):
        what = f"{name} N={N} iteration {t + 1}"
        cdev = torch.from_numpy(c_prev).to(gpu_device).contiguous()
        ids_pre = kmeans.assign(fdev, cdev[:ka].contiguous()).cpu().numpy()
        _assert_counts_are_the_assignment(_accumulate(fdev, cdev, ka), ids_pre, N, k, what)
        kmeans.lloyd(fdev, cdev, iters=1, nchunks=nch, k_active=k_active, id_offset=off)
        c_next_ref, ids_next_ref = ko.lloyd(X, c_prev, iters=1, nchunks=nch, k_active=k_active)
        c_got = cdev.cpu().numpy()
        flips, cdiff = helpers.kmeans_step_attribution(X, c_prev[:ka], c_next_ref[:ka], ids_prev_ref, ids_pre, c_got[:ka], what=what)
        assert np.abs(c_got[ka:]).max(initial=0.0) == 0.0 and np.abs(c_next_ref[ka:]).max(initial=0.0) == 0.0      # inactive rows -> 0
        print(f"{what}: {flips} rows differ from the reference side, centres within {cdiff:.2e}")
        c_prev, ids_prev_ref = c_next_ref, ids_next_ref          # the oracle's ids under its new centres: next step's reference
    fused = init.to(gpu_device).clone()
    ids_fused = kmeans.lloyd(fdev, fused, iters=3, nchunks=nch, k_active=k_active, id_offset=off)
    replay = init.to(gpu_device).clone()
    for _ in range(3):
        kmeans.lloyd(fdev, replay, iters=1, nchunks=nch, k_active=k_active, id_offset=off)
    np.testing.assert_allclose(fused.cpu().numpy(), replay.cpu().numpy(), atol=2e-6, rtol=0)
    ids = ids_fused.cpu().numpy() - off
    assert ids.min() >= 0 and ids.max() < ka
    # the fused call's ids against float64 under ITS OWN centres
    f64_ids, _ = _f64_ids(X, fused.cpu().numpy()[:ka])
    helpers.kmeans_final_ids_attribution(X, fused.cpu().numpy()[:ka], f64_ids, fused.cpu().numpy()[:ka], ids, f"{name} N={N} fused ids")


# ---- 2. block, wave, width and limit edges -------------------------------------------------------------------------------------------
def _lloyd_against_oracle(dev, feat, init, iters, k_active=None, off=0, what="", sharded=False):
    """`iters` fused iterations against ko.lloyd: centres by assert_centers_close (every row, 1e-4), ids by
    kmeans_final_ids_attribution; inactive rows are zero on both sides."""
    from opengaussian_amd import kmeans
    N, k = feat.shape[0], init.shape[0]
    ka = k if k_active is None else k_active
    nch = N // 10000 + 1
    cref, iref = ko.lloyd(feat.numpy(), init.numpy(), iters=iters, nchunks=nch, k_active=k_active, id_offset=off)
    cent = init.to(dev).clone()
    run = kmeans.lloyd_sharded if sharded else kmeans.lloyd
    ids = run(feat.to(dev), cent, iters, nch, k_active=k_active, id_offset=off).cpu().numpy()
    c = cent.cpu().numpy()
    assert ids.shape == (N,) and ids.min() >= off and ids.max() < off + ka, what
    assert_centers_close(c, cref, what)
    assert np.abs(c[ka:]).max(initial=0.0) == 0.0, f"{what}: inactive rows must be rewritten to zero"
    return helpers.kmeans_final_ids_attribution(feat.numpy(), cref[:ka], iref - off, c[:ka], ids - off, what)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 511, 513])
@pytest.mark.parametrize("name", list(PATHS))
def test_block_and_wave_remainders(gpu_device, name, N):
    """Less than a wave, a wave +- 1, a block +- 1, two blocks +- 1 on every path, three fused iterations against the oracle.
    The centres are drawn independently of the rows, so clusters empty (all but at most N of them when N < k) and collapse to
    the zero row, where they are exact duplicates of each other."""
    k, d, k_active, off = PATHS[name]
    g = _gen(k, d, N, 2)
    feat = torch.rand(N, d, generator=g)
    init = torch.rand(k, d, generator=g)
    _lloyd_against_oracle(gpu_device, feat, init, 3, k_active, off, f"{name} N={N}")


@pytest.mark.parametrize("d", [9, 5])
@pytest.mark.parametrize("k", [16, 17, 64, 65, 256, 257])
def test_cluster_count_boundaries(gpu_device, k, d):
    """k on both sides of every cluster_blocks() boundary (CB = 1 | 4 | 16 | the LDS fallback), at the GEMM width and a generic one"""
    g = _gen(k, d, 3)
    feat = torch.rand(5000, d, generator=g)
    _lloyd_against_oracle(gpu_device, feat, _rows_as_centres(feat, k, g), 3, what=f"k={k} d={d}")


@pytest.mark.parametrize("k", [16, 64])
@pytest.mark.parametrize("d", [1, 2, 15, 16])
def test_feature_width_boundaries(gpu_device, d, k):
    """d = 15: the last width of the MFMA tiling (the count column is tile column 15); d = 16: the first of the fallback"""
    g = _gen(k, d, 4)
    feat = torch.rand(5000, d, generator=g)
    _lloyd_against_oracle(gpu_device, feat, _rows_as_centres(feat, k, g), 3, what=f"k={k} d={d}")


@pytest.mark.parametrize("sharded", [False, True], ids=["lloyd", "lloyd_sharded"])
@pytest.mark.parametrize("k,d", [(1024, 15), (8192, 1)])
def test_accumulator_size_limit(gpu_device, k, d, sharded):
    """k (d + 1) == OGS_KMEANS_MAX_ACC exactly: the [k, d+1] table is 64 KiB, so kmeans_reduce_finalize_kernel (lloyd) and
    kmeans_finalize_kernel (lloyd_sharded: accumulate + update) both need the > 48 KiB dynamic-LDS opt-in"""
    assert k * (d + 1) == 16384
    g = _gen(k, d, 5)
    feat = torch.rand(5000, d, generator=g)
    init = torch.rand(k, d, generator=g)
    _lloyd_against_oracle(gpu_device, feat, init, 2, what=f"limit k={k} d={d} sharded={sharded}", sharded=sharded)


def test_one_past_the_size_limit_raises(gpu_device):
    from opengaussian_amd import kmeans
    feat = torch.rand(100, 15, device=gpu_device)
    with pytest.raises(RuntimeError):
        kmeans.lloyd(feat, torch.rand(1025, 15, device=gpu_device), 1, 1)
    with pytest.raises(RuntimeError):
        kmeans.lloyd_sharded(feat, torch.rand(1025, 15, device=gpu_device), 1, 1)
    with pytest.raises(RuntimeError):
        kmeans.assign(feat, torch.rand(1025, 15, device=gpu_device))


UNALIGNED = [(n, s) for n in ("A4", "B-200x6", "B-160x9", "C-64x7", "C-256x15") for s in ((1, 3) if PATHS[n][1] == 6 else (1,))]


@pytest.mark.parametrize("name,skip", UNALIGNED, ids=[f"{n}-from-row-{s}" for n, s in UNALIGNED])
def test_unaligned_base_pointer_changes_no_bit(gpu_device, name, skip):
    """big[skip:] is contiguous, so the product passes its base pointer on as it is: not 16-byte aligned.  Only the staging
    differs (fast_trip of the GEMM kernel, the float4 branch of the MFMA kernel), so ids and centres are BIT-identical to the
    same call on a fresh copy of the slice; the unaligned assignment is also held to the oracle."""
    from opengaussian_amd import kmeans
    k, d, k_active, off = PATHS[name]
    ka = k if k_active is None else k_active
    N = 70_000
    g = _gen(k, d, skip, 6)
    big = torch.rand(N + skip, d, generator=g).to(gpu_device)
    view, copy = big[skip:], big[skip:].clone()
    assert view.is_contiguous() and view.contiguous().data_ptr() == view.data_ptr()
    assert view.data_ptr() % 16 != 0 and copy.data_ptr() % 16 == 0, "the case must be what it claims to be"
    init = _rows_as_centres(copy.cpu(), k, g).to(gpu_device)
    out = []
    for f in (view, copy):
        cent = init.clone()
        ids = kmeans.lloyd(f, cent, 3, N // 10000 + 1, k_active=k_active, id_offset=off)
        out.append((ids, cent, kmeans.assign(f, cent[:ka].contiguous(), id_offset=off)))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert torch.equal(out[0][0], out[0][2])                                   # lloyd's final ids ARE the assignment
    x, c = copy.cpu().numpy(), out[0][1].cpu().numpy()[:ka]
    helpers.kmeans_final_ids_attribution(x, c, _oracle_ids(x, c), c, out[0][2].cpu().numpy() - off, f"{name} unaligned assign")


@pytest.mark.parametrize("name", FIXED_ORDER)
def test_two_identical_calls_give_the_same_bits(gpu_device, name):
    """kmeans.hip's header claims a fixed summation order for the MFMA kernels (wave tables, partial tables, slices): two
    identical calls, with workgroups that make two trips, agree bit for bit.  Path D (kmeans_lds_pass_kernel) accumulates with
    LDS float atomics, whose order is not fixed -- its doc comment says so -- and is held to the oracle only (every test above)."""
    from opengaussian_amd import kmeans
    k, d, k_active, off = PATHS[name]
    N = 300_001
    g = _gen(k, d, 7)
    fdev = torch.rand(N, d, generator=g).to(gpu_device)
    init = _rows_as_centres(fdev.cpu(), k, g).to(gpu_device)
    runs = []
    for _ in range(2):
        cent = init.clone()
        runs.append((kmeans.lloyd(fdev, cent, 3, N // 10000 + 1, k_active=k_active, id_offset=off), cent))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---- 3. exact ties ----------------------------------------------------------------------------------------------------------------
# (a, b): centre row b is a bitwise copy of row a.  In the GEMM kernel lane group g = (c % 16) / 4 of cluster block c / 16 holds
# centre c: same lane | adjacent lane groups (permlane16 swap) | groups 0 and 2 (permlane32 swap) | groups 1 and 3 |
# across cluster blocks, groups 3 and 0 | far apart, groups 1 and 1 | last lane of blocks 1 and 3
GEMM_PAIRS = [(0, 1), (3, 4), (3, 8), (7, 12), (15, 16), (5, 37), (31, 63)]
TIE_CASES = ([("A4", 64, 9, p) for p in GEMM_PAIRS] + [("A4-d6", 64, 6, p) for p in GEMM_PAIRS] +
             [("B-200x6", 200, 6, (7, 130)), ("C-64x7", 64, 7, (3, 8)), ("D-300x9", 300, 9, (31, 263))])


def _tie_scene(k, d, a, b, g, extra_copy_of=None):
    """centres with row b == row a bitwise, and 20 000 uniform rows + 1 500 rows scattered tightly around that centre"""
    cent = torch.rand(k, d, generator=g)
    cent[b] = cent[a]
    feat = torch.cat([torch.rand(20_000, d, generator=g), cent[a][None, :] + 0.02 * torch.randn(1500, d, generator=g)])
    feat = feat[torch.randperm(feat.shape[0], generator=g)].contiguous()
    assert torch.equal(cent[a], cent[b])
    return feat, cent


@pytest.mark.parametrize("name,k,d,pair", TIE_CASES, ids=[f"{n}-{p[0]}-{p[1]}" for n, _, _, p in TIE_CASES])
def test_duplicate_centre_first_index_wins(gpu_device, name, k, d, pair):
    """Duplicate centres are normal here (every emptied cluster collapses to the zero row).  Row b is a copy of row a < b and
    that centre is the float64 nearest one for >= 1000 rows: assign never returns b, the accumulate pass counts every such row
    for a and leaves row b of the table at exactly zero, and after one Lloyd iteration centre b is exactly zero.  No tolerance
    applies to any of that.  Centre a is then the mean of ALL those rows: against the float64 mean, at the 2e-5 arithmetic bar
    of kmeans_step_attribution (an fp32 mean is not a float64 one), and against the oracle's centre a at its 1e-4."""
    from opengaussian_amd import kmeans
    a, b = pair
    g = _gen(k, d, a, b, 8)
    feat, cent = _tie_scene(k, d, a, b, g)
    X, Cn = feat.numpy(), cent.numpy()
    f64_ids, _ = _f64_ids(X, Cn)                                    # first minimum: a for the tied rows
    assert not (f64_ids == b).any() and int((f64_ids == a).sum()) >= 1000
    fdev, cdev = feat.to(gpu_device), cent.to(gpu_device)
    ids = kmeans.assign(fdev, cdev).cpu().numpy()
    assert not (ids == b).any(), f"{name}: assign returned the copy {b} of centre {a} on {int((ids == b).sum())} rows"
    helpers.kmeans_final_ids_attribution(X, Cn, f64_ids, Cn, ids, f"{name} tie {pair}")
    assert int((ids == a).sum()) >= 1000
    table = _accumulate(fdev, cdev)
    _assert_counts_are_the_assignment(table, ids, len(X), k, f"{name} tie {pair}")
    assert (table[b] == 0.0).all()
    c1 = cdev.clone()
    kmeans.lloyd(fdev, c1, iters=1, nchunks=len(X) // 10000 + 1)
    c1 = c1.cpu().numpy()
    assert (c1[b] == 0.0).all(), f"{name}: centre {b} must be exactly zero after the iteration, got {c1[b]}"
    assert np.abs(c1[a] - X[ids == a].astype(np.float64).mean(0)).max() < 2e-5
    cref, _ = ko.lloyd(X, Cn, iters=1)                              # the oracle takes the first minimum too: all tied rows go to a
    assert (cref[b] == 0.0).all() and np.abs(c1[a] - cref[a]).max() <= helpers.KM_CENTER_TOL


@pytest.mark.parametrize("name,k,d,ka,a,b", [("A1", 10, 6, 7, 2, 8), ("A4", 64, 9, 40, 3, 50), ("A4-d6", 64, 6, 17, 16, 33),
                                             ("B-160x9", 160, 9, 100, 10, 120), ("C-64x7", 64, 7, 30, 29, 30),
                                             ("D-300x9", 300, 9, 270, 5, 299)])
def test_copy_of_an_active_centre_beyond_k_active_is_never_chosen(gpu_device, name, k, d, ka, a, b):
    """k_active < k (leaf mode): rows >= k_active are not candidates, an exact copy of the nearest active centre included"""
    from opengaussian_amd import kmeans
    assert a < ka <= b
    g = _gen(k, d, a, b, 9)
    feat, cent = _tie_scene(k, d, a, b, g)
    X, Cn = feat.numpy(), cent.numpy()
    f64_ids, _ = _f64_ids(X, Cn[:ka])
    assert int((f64_ids == a).sum()) >= 1000
    fdev = feat.to(gpu_device)
    c0 = cent.to(gpu_device).clone()
    ids = kmeans.lloyd(fdev, c0, iters=0, nchunks=1, k_active=ka, id_offset=1000).cpu().numpy() - 1000     # assignment only
    assert torch.equal(c0.cpu(), cent)
    assert ids.min() >= 0 and ids.max() < ka
    helpers.kmeans_final_ids_attribution(X, Cn[:ka], f64_ids, Cn[:ka], ids, f"{name} k_active tie")
    table = _accumulate(fdev, cent.to(gpu_device), ka)
    _assert_counts_are_the_assignment(table, ids, len(X), k, f"{name} k_active tie")
    assert (table[ka:] == 0.0).all()


# ---- 4. scale and translation -----------------------------------------------------------------------------------------------------
OFF_ORIGIN = ["A4", "A1", "B-200x6", "B-160x9", "C-64x7"]
N_OFF = 100_000


def _base(name, salt):
    k, d, k_active, off = PATHS[name]
    g = _gen(k, d, salt)
    feat = torch.rand(N_OFF, d, generator=g)
    return feat, _rows_as_centres(feat, k, g), k_active, off


@pytest.mark.parametrize("name", OFF_ORIGIN)
def test_power_of_two_scale_commutes_bit_for_bit(gpu_device, name):
    """Every fp32 operation of every path commutes with a power-of-two scale, and so do the truncation splits and the 0 / 1
    one-hot factors; nothing is near underflow or overflow.  So scaling rows and centres by 2^10 or 2^-10 leaves the ids
    unchanged and scales the centres, bit for bit.  A failure means an unscaled constant has entered the distance."""
    from opengaussian_amd import kmeans
    feat, init, k_active, off = _base(name, 10)
    nch = N_OFF // 10000 + 1
    runs = {}
    for s in (1.0, 2.0 ** 10, 2.0 ** -10):
        cent = (init * s).to(gpu_device)
        ids = kmeans.lloyd((feat * s).to(gpu_device), cent, 3, nch, k_active=k_active, id_offset=off)
        runs[s] = (ids.cpu(), cent.cpu())
    for s in (2.0 ** 10, 2.0 ** -10):
        assert torch.equal(runs[s][0], runs[1.0][0]), f"{name}: ids change under the scale {s}"
        assert torch.equal(runs[s][1], runs[1.0][1] * s), f"{name}: centres are not the scaled centres under the scale {s}"
    assert len(torch.unique(runs[1.0][0])) > 1


def _reference_formulation_error(X32, ids, k):
    """E_ref: the worst error, against the float64 member means, of the REFERENCE's formulation on the same ids: fp32
    one_hot^T @ x per 10 000-row chunk, summed over the chunks in fp32, divided by the counts (kmeans_quantize.py:184-187,209)"""
    sums = torch.zeros(k, X32.shape[1], dtype=torch.float32)
    x, i = torch.from_numpy(X32), torch.from_numpy(ids)
    for lo in range(0, len(X32), 10000):
        onehot = torch.nn.functional.one_hot(i[lo:lo + 10000], k).to(torch.float32)
        sums += onehot.T @ x[lo:lo + 10000]
    counts = np.bincount(ids, minlength=k).astype(np.float64)
    means = np.stack([X32[ids == j].astype(np.float64).mean(0) if counts[j] else np.zeros(X32.shape[1]) for j in range(k)])
    got = sums.numpy().astype(np.float64) / np.maximum(counts, 1.0)[:, None]
    return float(np.abs(got - means)[counts > 0].max()), means, counts


def _off_origin_step(dev, feat, cent, k_active, what):
    """assign + one Lloyd iteration on (feat, cent).  Every id is the float64 nearest centre to within KM_TIE (helpers
    unchanged); at most 1e-3 N rows differ from the oracle's argmin (the oracle docstring's own cap); every centre is the float64
    mean of its members to max(2e-5, 4 E_ref).  Returns (worst excess distance, centre error, E_ref)."""
    from opengaussian_amd import kmeans
    k = cent.shape[0]
    ka = k if k_active is None else k_active
    X, Cn = feat.numpy(), cent.numpy()
    fdev, cdev = feat.to(dev), cent.to(dev).clone()
    ids = kmeans.assign(fdev, cdev[:ka].contiguous()).cpu().numpy()
    f64_ids, dmin = _f64_ids(X, Cn[:ka])
    chosen = np.sqrt(((X.astype(np.float64) - Cn[:ka].astype(np.float64)[ids]) ** 2).sum(-1))
    excess = float((chosen - dmin).max())
    n_off_f64 = int((ids != f64_ids).sum())
    n_off_oracle = int((ids != _oracle_ids(X, Cn[:ka])).sum())
    print(f"{what}: worst excess distance over the float64 minimum {excess:.3e} (KM_TIE {KM_TIE}); {n_off_f64} rows off the "
          f"float64 argmin, {n_off_oracle} off the oracle's")
    helpers.kmeans_final_ids_attribution(X, Cn[:ka], f64_ids, Cn[:ka], ids, what)
    assert n_off_oracle <= 1e-3 * len(X), f"{what}: {n_off_oracle} rows differ from the oracle's argmin"
    _assert_counts_are_the_assignment(_accumulate(fdev, cdev, ka), ids, len(X), k, what)
    kmeans.lloyd(fdev, cdev, iters=1, nchunks=len(X) // 10000 + 1, k_active=k_active)
    e_ref, means, counts = _reference_formulation_error(X, ids, k)
    got = cdev.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - means)[counts > 0].max())
    print(f"{what}: centres off the float64 member means by {err:.3e}; E_ref {e_ref:.3e}; ratio {err / max(e_ref, 1e-30):.2f}")
    assert np.abs(got[counts == 0]).max(initial=0.0) < 1e-5, f"{what}: empty clusters must collapse to ~0"
    assert err <= max(2e-5, 4 * e_ref), f"{what}: centre error {err:.3e} > max(2e-5, 4 x E_ref = {4 * e_ref:.3e})"
    return excess, err, e_ref


@pytest.mark.parametrize("name", OFF_ORIGIN)
def test_translated_data_keeps_the_tie_width(gpu_device, name):
    """Unit-spread rows translated by +100 in every column, centres drawn from the rows.  x - c and x - mu of nearby fp32 numbers
    round relative to the RESULT, so the translation buys no extra tie width: KM_TIE as everywhere.  Centres: the float64 mean of
    their own members within max(2e-5, 4 E_ref), E_ref measured here on the reference's formulation (the factor 4 is room for a
    different order of the same fp32 terms; a ratio above 4 is something to explain, not to widen).  Measured on an MI355X:
    worst excess 0 and 0 rows off the oracle's argmin on every path; centre error / E_ref = 3.1e-5 / 2.4e-5 = 1.28 (A4),
    2.7e-5 / 7.7e-5 = 0.35 (A1), 3.8e-5 / 2.3e-5 = 1.67 and 3.3e-5 / 2.8e-5 = 1.21 (B), 3.8e-5 / 3.1e-5 = 1.22 (C)."""
    feat, _, k_active, _ = _base(name, 11)
    feat = feat + 100.0
    cent = _rows_as_centres(feat, PATHS[name][0], _gen(12))
    _off_origin_step(gpu_device, feat, cent, k_active, f"{name} +100")


@pytest.mark.parametrize("name,zero_rows", [("A4", (3, 9, 17, 22, 31, 40, 55, 63)), ("A1", (2, 5))])
def test_translated_data_with_emptied_centres_keeps_the_tie_width(gpu_device, name, zero_rows):
    """As above, with 8 of the 64 (2 of the 7 active) centres at the zero row, where emptied clusters collapse to
    (kmeans_quantize.py:209).  The GEMM pass used to shift by the mean of the active centres, which such rows drag away from
    the data: a CPU emulation of that score arithmetic put 55 of 100 000 rows up to 3.4e-4 beyond the float64 minimum.  Measured
    on an MI355X with that shift: 74 rows, worst excess 3.4e-4 (A4); 93 rows, worst excess 1.7e-3 (A1).  With the shift taken
    from the rows (the centroid of 64 sampled rows): 0 rows, worst excess 0 on both; centre error / E_ref 1.67 (A4), 0.33 (A1)."""
    feat, _, k_active, _ = _base(name, 13)
    feat = feat + 100.0
    cent = _rows_as_centres(feat, PATHS[name][0], _gen(14))
    cent[list(zero_rows)] = 0.0
    _off_origin_step(gpu_device, feat, cent, k_active, f"{name} +100, {len(zero_rows)} centres at zero")


@pytest.mark.parametrize("name", OFF_ORIGIN)
def test_mixed_magnitude_columns_keep_the_tie_width(gpu_device, name):
    """The last three columns uniform in +-30, the others in [0, 1) (d = 9: six and three, the root level's features | scaled
    positions), centres drawn from the rows: KM_TIE as everywhere.  Measured on an MI355X: worst excess 0 on every path, centre
    error <= 1.1e-5, 1.40 .. 2.51 x E_ref."""
    feat, _, k_active, _ = _base(name, 15)
    feat[:, -3:] = feat[:, -3:] * 60.0 - 30.0
    cent = _rows_as_centres(feat, PATHS[name][0], _gen(16))
    _off_origin_step(gpu_device, feat, cent, k_active, f"{name} mixed columns")
