"""CPU: the NumPy restatement of the k-nearest-distance sums against goldens made by the reference's own code
(tests/golden/make_knn_golden.py), the K rule, the selection-by-bisection argument, the host glue of opengaussian_amd.knn
around a stand-in for the kernel, and the margin conditions of the inputs tests/test_37_knn_gpu.py runs on the GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import knn_cases as kc
from tests import knn_restatement as kr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_restatement_masks_equal_the_reference_block(gold):
    for n in gold["mask_sizes"]:
        for kind in gold["mask_kinds"]:
            k = f"mask/{n}/{kind}"
            st = kr.outlier_stats(gold[k + "/points"])
            assert np.array_equal(st["mask"], gold[k + "/mask"]), k
            assert st["K"] == int(int(n) ** 0.5)
            # the reference ran on fp64 distances, the restatement on fp32 ones (1e-7 each)
            assert st["mean"] == pytest.approx(float(gold[k + "/mean"]), rel=1e-5, abs=0), k
            if np.isnan(gold[k + "/std"]):
                assert np.isnan(st["std"]) and not st["mask"].any()
            else:
                assert st["std"] == pytest.approx(float(gold[k + "/std"]), rel=1e-5, abs=0), k


def test_restatement_distcuda2_equals_the_reference(gold):
    for name in gold["dist_cases"]:
        got, want = kr.dist_cuda2(gold[f"dist/{name}/points"]).astype(np.float64), gold[f"dist/{name}/out"].astype(np.float64)
        assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), (name, np.abs(got / want - 1)[want > 0].max())


def test_k_rule_at_perfect_squares():
    from opengaussian_amd import knn
    roots = np.concatenate([np.arange(0, 3000), [4095, 4096, 4097, 46340, 46341, 65535, 65536, 1_000_000, 1 << 26]])
    ns = np.unique(np.concatenate([roots * roots, roots * roots - 1, roots * roots + 1]))
    ns = ns[ns >= 0]
    got = knn.isqrt(torch.from_numpy(ns)).numpy()
    assert np.all(got * got <= ns) and np.all((got + 1) * (got + 1) > ns)
    small = ns[ns < (1 << 31)]                                  # every size a group can have: Python's own rule agrees
    assert [int(v) for v in knn.isqrt(torch.from_numpy(small))] == [int(int(v) ** 0.5) for v in small]
    assert [kr.k_rule(int(v), 2) for v in (1, 4, 9, 15, 16, 17)] == [2, 4, 6, 6, 8, 8]


def test_bisection_on_bit_patterns_selects_what_a_sort_selects(gold):
    """The kernel's argument in NumPy: the K-th smallest d2 is the smallest bit pattern t with count(d2 <= t) >= K, found in
    31 halvings of [0, 0x7f800000]; values below it once each plus the ties K - count_below times are the sorted sums."""
    for pts, K in ((gold["mask/100/clustered/points"], 10), (kc.tie_clouds(5)["dup"], 5), (kc.tie_clouds(7)["lattice"], 7)):
        d = kr.sqdist_rows(pts, np.arange(len(pts)))
        bits = d.view(np.uint32).astype(np.int64)
        lo, hi = np.zeros(len(pts), np.int64), np.full(len(pts), 0x7f800000, np.int64)
        for _ in range(31):
            mid = lo + ((hi - lo) >> 1)
            ok = (bits <= mid[:, None]).sum(1) >= K
            hi, lo = np.where(ok, mid, hi), np.where(ok, lo, mid + 1)
        assert np.array_equal(lo, hi)
        kth = hi.astype(np.uint32).view(np.float32)
        below = bits < hi[:, None]
        d64 = d.astype(np.float64)
        s1 = np.where(below, d64, 0).sum(1) + (K - below.sum(1)) * kth.astype(np.float64)
        s2 = np.where(below, d64 * d64, 0).sum(1) + (K - below.sum(1)) * kth.astype(np.float64) ** 2
        rk, r1, r2 = kr.ksum(pts, K)
        assert np.array_equal(kth, rk)
        assert np.allclose(s1, r1, rtol=1e-13, atol=0) and np.allclose(s2, r2, rtol=1e-13, atol=0)


def test_gpu_test_inputs_have_their_margins(gold):
    """Masks are compared exactly on the GPU, so no row of those inputs may sit near its threshold (1e-6 relative: the
    reach of a reordered fp64 sum is 1e-13)."""
    assert kr.outlier_stats(kc.click_variant(), k_scale=2, std_weight=0.1)["margin"].min() > 1e-6
    assert kr.outlier_stats(kc.click_variant())["margin"].min() > 1e-6          # smoke() runs the default rule on it
    pts, group, sizes = kc.many_groups()
    worst = min(kr.outlier_stats(pts[group == g])["margin"].min() for g in range(kc.MANY_GROUPS) if sizes[g] > 0)
    assert worst > 1e-6
    assert (sizes == 0).sum() >= 6 and sizes[0] == 0 and sizes[-1] == 0 and sizes[320] == 0 and (group == -1).sum() == 5000
    for K in (5, 7):                                          # the tie inputs do tie at the K-th value
        c = kc.tie_clouds(K)
        d = np.sort(kr.sqdist_rows(c["dup"], np.arange(len(c["dup"]))), axis=1)
        assert ((d[:, K - 1] == 0) & (d[:, K] == 0)).sum() == K + 2
        d = np.sort(kr.sqdist_rows(c["lattice"], np.arange(216)), axis=1)
        assert (d[:, K - 1] == d[:, K]).mean() > 0.5 and (d[:, K - 1] > 0).all()      # most rows: a shell straddles K


# ---- the host glue of opengaussian_amd.knn around a CPU stand-in for the kernel ---------------------------------------------
class _FakeLib:
    """ogs_knn_group_ksum on host memory through the same pointers, computed by the restatement; rows outside
    [begin[0], begin[G]) are not written, as the header says."""
    def __init__(self):
        self.calls = 0

    def ogs_knn_group_ksum(self, n, pts, G, begin, k, kth, s1, s2, stream):
        arr = lambda p, ct, m: np.ctypeslib.as_array((ct * m).from_address(p))
        self.calls += 1
        P = arr(pts, ctypes.c_float, n * 3).reshape(n, 3)
        B, Kk = arr(begin, ctypes.c_int32, G + 1), arr(k, ctypes.c_int32, G)
        o_kth = arr(kth, ctypes.c_float, n) if kth else np.zeros(n, np.float32)            # kth may be NULL
        o1, o2 = arr(s1, ctypes.c_double, n), arr(s2, ctypes.c_double, n)
        assert np.all(np.diff(B) >= 0) and B[0] >= 0 and B[-1] <= n
        for g in range(G):
            if B[g + 1] > B[g]:
                o_kth[B[g]:B[g + 1]], o1[B[g]:B[g + 1]], o2[B[g]:B[g + 1]] = kr.ksum(P[B[g]:B[g + 1]], Kk[g])
        return 0


@pytest.fixture
def cpu_knn(monkeypatch):
    from opengaussian_amd import knn
    fake = _FakeLib()
    monkeypatch.setattr(knn, "_need_gpu", lambda t, name: None)
    monkeypatch.setattr(knn, "_stream", lambda: 0)
    monkeypatch.setattr(knn._lib, "lib", lambda: fake)
    return knn, fake


def test_glue_sorts_groups_and_returns_the_callers_order(cpu_knn):
    knn, fake = cpu_knn
    rng = np.random.default_rng(3)
    group = rng.integers(-2, 9, 400)                           # -2, -1 and 7, 8 (>= num_groups) belong to no group
    pts = rng.random((400, 3)).astype(np.float32)
    kth, s1, s2 = knn.group_ksum(torch.from_numpy(pts), torch.from_numpy(group), 7, 5)
    rk, r1, r2 = kr.group_ksum(pts, group, 7, 5)
    inside = (group >= 0) & (group < 7)
    assert np.array_equal(kth.numpy()[inside], rk[inside]) and np.array_equal(s1.numpy()[inside], r1[inside])
    assert np.array_equal(s2.numpy()[inside], r2[inside])
    assert not kth.numpy()[~inside].any() and not s1.numpy()[~inside].any()
    assert fake.calls == 1                                      # all groups in one launch
    per_group = torch.tensor([0, 1, 2, 3, 1000, 4, 5])          # K = 0 writes zeros, K > n_g clamps
    kth, s1, _ = knn.group_ksum(torch.from_numpy(pts), torch.from_numpy(group), 7, per_group)
    rk, r1, _ = kr.group_ksum(pts, group, 7, per_group.numpy())
    assert np.array_equal(kth.numpy()[inside], rk[inside]) and np.array_equal(s1.numpy()[inside], r1[inside])
    assert not s1.numpy()[group == 0].any()


def test_glue_outlier_mask_and_distcuda2_equal_the_goldens(cpu_knn, gold):
    knn, _ = cpu_knn
    for n in gold["mask_sizes"]:
        for kind in gold["mask_kinds"]:
            k = f"mask/{n}/{kind}"
            got = knn.outlier_mask(torch.from_numpy(gold[k + "/points"]))
            assert got.dtype == torch.bool and np.array_equal(got.numpy(), gold[k + "/mask"]), k
    # the same cases as groups of one call, shuffled together with rows of no group
    names = [f"mask/{n}/{kind}" for n in gold["mask_sizes"] for kind in gold["mask_kinds"] if int(n) <= 1024]
    pts = np.concatenate([gold[k + "/points"] for k in names] + [np.zeros((50, 3), np.float32)])
    group = np.concatenate([np.full(len(gold[k + "/points"]), 2 * i + 1) for i, k in enumerate(names)] + [np.full(50, -1)])
    want = np.concatenate([gold[k + "/mask"] for k in names] + [np.zeros(50, bool)])
    perm = np.random.default_rng(0).permutation(len(group))
    got = knn.outlier_mask(torch.from_numpy(pts[perm]), torch.from_numpy(group[perm]), 2 * len(names) + 3)   # even ids: empty groups
    assert np.array_equal(got.numpy(), want[perm])
    p = kc.click_variant()
    assert np.array_equal(knn.outlier_mask(torch.from_numpy(p), k_scale=2, std_weight=0.1).numpy(),
                          kr.outlier_mask(p, k_scale=2, std_weight=0.1))
    for name in gold["dist_cases"]:
        got = knn.distCUDA2(torch.from_numpy(gold[f"dist/{name}/points"]))
        want = gold[f"dist/{name}/out"].astype(np.float64)
        assert got.dtype == torch.float32 and np.all(np.abs(got.numpy() - want) <= 1e-6 * np.abs(want)), name


def test_cpu_tensors_are_refused():
    from opengaussian_amd import knn
    p = torch.rand(10, 3)
    for call in (lambda: knn.outlier_mask(p), lambda: knn.distCUDA2(p), lambda: knn.group_ksum(p, None, 1, 3)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
