"""GPU: the k-nearest-distance kernel (include/ogs_knn.h) through its C ABI and through opengaussian_amd.knn, against the
NumPy restatement (tests/knn_restatement.py) and the goldens made by the reference's own code (tests/golden/knn_golden.npz).

`kth` must be bit-identical to the restatement's sorted selection; `sum1` / `sum2` are sums of at most a few thousand exactly
representable fp64 terms in another order: 1e-12 relative."""
import os
import types

import numpy as np
import pytest
import torch

from tests import helpers
from tests import knn_cases as kc
from tests import knn_restatement as kr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_golden.npz")
CANARY = -12345.0
SUM_RTOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _tile():
    from opengaussian_amd import _lib
    return int(_lib.lib().ogs_knn_tile_points())


def capi_ksum(dev, points, begin, k, with_kth=True):
    """ogs_knn_group_ksum on rows that are already sorted by group; outputs start as CANARY."""
    from opengaussian_amd import _lib
    n = len(points)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    pts, b, kk = t(points, torch.float32), t(begin, torch.int32), t(k, torch.int32)
    kth = torch.full((n,), CANARY, dtype=torch.float32, device=dev) if with_kth else None
    s1 = torch.full((n,), CANARY, dtype=torch.float64, device=dev)
    s2 = torch.full((n,), CANARY, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().ogs_knn_group_ksum(n, _lib.ptr(pts), len(k), _lib.ptr(b), _lib.ptr(kk), _lib.ptr(kth), _lib.ptr(s1),
                                              _lib.ptr(s2), torch.cuda.current_stream().cuda_stream), "ogs_knn_group_ksum")
    torch.cuda.synchronize()
    return (None if kth is None else kth.cpu().numpy()), s1.cpu().numpy(), s2.cpu().numpy()


def assert_sums(got1, got2, want1, want2, what):
    assert np.all(np.abs(got1 - want1) <= SUM_RTOL * np.abs(want1)), (what, "sum1")
    assert np.all(np.abs(got2 - want2) <= SUM_RTOL * np.abs(want2)), (what, "sum2")


# rows in all (the group sits behind 3 rows of no group, the rest follows it): 0 = just the group + 7; the larger totals
# take the kernel's two-queries-per-thread form, which is chosen by the row count (16 384 and up)
SIZES = [(n, 0) for n in (1, 2, 3, 9, 10, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 4097)] + \
        [(257, 40000), (1025, 70000), (2049, 70000)]


@pytest.mark.parametrize("n,rows", SIZES)
def test_one_group_every_k(gpu_device, n, rows):
    assert _tile() == 1024, "SIZES brackets the LDS tile: update it with the kernel"
    total = max(rows, n + 7)
    pts = kc.cloud(total, 100 + n)
    grp = pts[3:3 + n]
    d = np.sort(kr.sqdist_rows(grp, np.arange(n)), axis=1).astype(np.float64)
    outside = np.ones(total, bool)
    outside[3:3 + n] = False
    for K in sorted({0, 1, min(4, n), int(n ** 0.5), n, n + 5}):
        kth, s1, s2 = capi_ksum(gpu_device, pts, [3, 3 + n], [K])
        Kc = min(K, n)
        if Kc == 0:
            assert not kth[3:3 + n].any() and not s1[3:3 + n].any() and not s2[3:3 + n].any()
        else:
            assert np.array_equal(kth[3:3 + n], d[:, Kc - 1].astype(np.float32)), (n, K)
            assert_sums(s1[3:3 + n], s2[3:3 + n], d[:, :Kc].sum(1), (d[:, :Kc] ** 2).sum(1), (n, K))
        assert np.all(kth[outside] == CANARY) and np.all(s1[outside] == CANARY) and np.all(s2[outside] == CANARY)
    _, s1b, _ = capi_ksum(gpu_device, pts, [3, 3 + n], [int(n ** 0.5)], with_kth=False)       # kth = NULL
    Kc = int(n ** 0.5)
    assert np.all(np.abs(s1b[3:3 + n] - d[:, :Kc].sum(1)) <= SUM_RTOL * d[:, :Kc].sum(1))


@pytest.fixture(scope="module")
def many():
    pts, group, sizes = kc.many_groups()
    K = np.array([int(s ** 0.5) for s in sizes])
    return pts, group, sizes, K, kr.group_ksum(pts, group, kc.MANY_GROUPS, K)


def test_many_groups_capi_and_canary(gpu_device, many):
    pts, group, sizes, K, (rk, r1, r2) = many
    order = np.argsort(group, kind="stable")                   # -1 first
    begin = 5000 + np.concatenate([[0], np.cumsum(sizes)])
    kth, s1, s2 = capi_ksum(gpu_device, pts[order], begin, K)
    assert np.all(kth[:5000] == CANARY) and np.all(s1[:5000] == CANARY) and np.all(s2[:5000] == CANARY)
    assert np.array_equal(kth[5000:], rk[order][5000:])
    assert_sums(s1[5000:], s2[5000:], r1[order][5000:], r2[order][5000:], "many groups")


def test_many_groups_through_knn_py_in_callers_order_and_deterministic(gpu_device, many):
    from opengaussian_amd import knn
    pts, group, sizes, K, (rk, r1, r2) = many
    p, g = torch.from_numpy(pts).to(gpu_device), torch.from_numpy(group).to(gpu_device)
    a = knn.group_ksum(p, g, kc.MANY_GROUPS, knn.isqrt)
    b = knn.group_ksum(p, g, kc.MANY_GROUPS, knn.isqrt)
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                # same bits
    inside = group >= 0
    kth, s1, s2 = (x.cpu().numpy() for x in a)
    assert np.array_equal(kth[inside], rk[inside])
    assert_sums(s1[inside], s2[inside], r1[inside], r2[inside], "knn.group_ksum")
    assert not kth[~inside].any() and not s1[~inside].any() and not s2[~inside].any()
    keep = knn.outlier_mask(p, g, kc.MANY_GROUPS).cpu().numpy()
    assert np.array_equal(keep, kr.outlier_mask(pts, group, kc.MANY_GROUPS))
    assert not keep[group == 2].any()                           # the group of one point: std = nan


@pytest.mark.parametrize("K", [5, 7])
def test_exact_ties(gpu_device, K):
    for name, pts in kc.tie_clouds(K).items():
        n = len(pts)
        kth, s1, s2 = capi_ksum(gpu_device, pts, [0, n], [K])
        rk, r1, r2 = kr.ksum(pts, K)
        assert np.array_equal(kth, rk), name
        assert_sums(s1, s2, r1, r2, name)
        if name == "dup":
            assert (kth == 0).sum() >= K + 2 and (s1 == 0).sum() >= K + 2       # the K-th value is a tie and zero
        else:
            assert np.array_equal(s1, r1) and np.array_equal(s2, r2)            # small integers: exact in any order


def test_offset_cloud(gpu_device):
    pts = kc.cloud(1000, 8, shift=1000.0)
    kth, s1, s2 = capi_ksum(gpu_device, pts, [0, 1000], [31])
    rk, r1, r2 = kr.ksum(pts, 31)
    assert np.array_equal(kth, rk) and (kth > 0).all()
    assert_sums(s1, s2, r1, r2, "offset")


def test_fixtures_of_the_reference(gpu_device, gold):
    from opengaussian_amd import knn
    for n in gold["mask_sizes"]:
        for kind in gold["mask_kinds"]:
            k = f"mask/{n}/{kind}"
            got = knn.outlier_mask(torch.from_numpy(gold[k + "/points"]).to(gpu_device))
            assert np.array_equal(got.cpu().numpy(), gold[k + "/mask"]), k
    for name in gold["dist_cases"]:
        got = knn.distCUDA2(torch.from_numpy(gold[f"dist/{name}/points"]).to(gpu_device))
        want = gold[f"dist/{name}/out"].astype(np.float64)
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert np.all(np.abs(got.cpu().numpy() - want) <= 1e-6 * np.abs(want)), name
    p = kc.click_variant()                                      # scripts/render_by_click.py:177,183
    got = knn.outlier_mask(torch.from_numpy(p).to(gpu_device), k_scale=2, std_weight=0.1)
    assert np.array_equal(got.cpu().numpy(), kr.outlier_mask(p, k_scale=2, std_weight=0.1))


def test_twenty_thousand_points_without_an_n_by_n_buffer(gpu_device):
    from opengaussian_amd import knn
    n = 20000
    pts = kc.cloud(n, 20)
    p = torch.from_numpy(pts).to(gpu_device)
    knn.outlier_mask(p[:100])                                   # load the library outside the measured window
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    keep = knn.outlier_mask(p)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"outlier_mask n={n}: peak {peak} bytes = {peak / n:.1f} per point")
    assert peak < 64 * n
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    kth, s1, s2 = knn.group_ksum(p, None, 1, 141)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"group_ksum n={n}: peak {peak} bytes = {peak / n:.1f} per point")
    assert peak < 64 * n
    rows = np.random.default_rng(1).choice(n, 256, replace=False)
    rk, r1, r2 = kr.ksum(pts, 141, rows=rows)
    assert np.array_equal(kth.cpu().numpy()[rows], rk)
    assert_sums(s1.cpu().numpy()[rows], s2.cpu().numpy()[rows], r1, r2, "n = 20000")
    # the mask of the sampled rows from the kernel's own group totals (the restatement of all 20 000 rows is not needed)
    S1, S2, N = float(s1.sum()), float(s2.sum()), n * 141.0
    limit = S1 / N + np.sqrt((S2 - S1 * S1 / N) / (N - 1))
    margin = np.abs(r1 / 141 - limit) / limit
    ok = margin > 1e-6
    assert ok.sum() >= 250 and np.array_equal(keep.cpu().numpy()[rows][ok], (r1 / 141 < limit)[ok])


def test_cpu_tensors_are_refused_and_bad_sizes_are_errors(gpu_device):
    from opengaussian_amd import _lib, knn
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn.outlier_mask(torch.rand(10, 3))
    assert _lib.lib().ogs_knn_group_ksum(-1, None, 1, None, None, None, None, None, None) == -1
    assert _lib.lib().ogs_knn_group_ksum(10, None, 1, None, None, None, None, None, None) == -1
    assert knn.outlier_mask(torch.zeros(0, 3, device=gpu_device)).shape == (0,)


# ---- through render() ---------------------------------------------------------------------------------------------------------
def _margin_f64(points):
    """|row mean - limit| / limit of the reference's rule on one leaf, everything in float64."""
    p = points.astype(np.float64)
    n = len(p)
    K = int(n ** 0.5)
    d = np.sort(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1), axis=1)[:, :K]
    limit = d.mean() + d.std(ddof=1)
    return np.abs(d.mean(axis=1) - limit) / limit


def test_render_post_process_equals_the_leafwise_torch_filter(gpu_device, monkeypatch):
    """render(post_process=True) over all leaves through knn.outlier_mask == the same call with the branch served leaf by leaf
    by renderer._knn_mean_filter (the n x n torch stand-in render() used before): same leaf ids, identical images."""
    from opengaussian_amd import knn
    from opengaussian_amd import renderer as R
    from tests.test_11_render_gpu import FakeGaussians
    dev = gpu_device
    W, H, f, P = 112, 80, 90.0, 6000
    sc, cam = helpers.tiny_scene(P, W, H, f, seed=31, log_scale_mean=-3.5)
    cam = cam.to(dev)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    root_num, leaf_num = 4, 5
    g = torch.Generator().manual_seed(2)
    leaf_idx = torch.randint(0, root_num * leaf_num, (P,), generator=g).to(dev)
    leaf_idx[leaf_idx == 7] = 6                       # leaf 7 empty, leaf 13 almost empty (< 10 points)
    few = torch.nonzero(leaf_idx == 13).flatten()
    leaf_idx[few[5:]] = 12
    kw = dict(iteration=1, rescale=False, render_feat_map=False, root_num=root_num, leaf_num=leaf_num,
              leaf_cluster_idx=leaf_idx, post_process=True, selected_leaf_id=None)
    seen = []

    def kernel_path(points, group, num_groups):
        seen.append((points.detach().cpu().numpy(), group.cpu().numpy(), num_groups))
        return knn.outlier_mask(points, group, num_groups)

    def leafwise_torch(points, group, num_groups):
        keep = torch.zeros_like(group, dtype=torch.bool)
        for g_ in torch.unique(group[group >= 0]).tolist():
            rows = torch.nonzero(group == g_).flatten()
            keep[rows] = R._knn_mean_filter(points[rows])
        return keep

    outs = []
    for path in (kernel_path, leafwise_torch):
        monkeypatch.setattr(R, "_knn", types.SimpleNamespace(outlier_mask=path))
        with torch.no_grad():
            outs.append(R.render(cam, FakeGaussians(sc, dev), pipe, torch.tensor([0.1, 0.0, 0.2], device=dev), **kw))
    (points, group, num_groups), = seen
    assert num_groups == root_num * leaf_num
    leaves = [l for l in range(num_groups) if (group == l).sum() > 0]
    margins = {l: _margin_f64(points[group == l]).min() for l in leaves if (group == l).sum() > 1}
    print("smallest margin per leaf:", {l: "%.1e" % m for l, m in margins.items()})
    assert len(margins) >= 18 and min(margins.values()) > 1e-5, "choose another seed: a row sits on its threshold"
    a, b = outs
    assert a["occured_leaf_id"] == b["occured_leaf_id"] and len(a["occured_leaf_id"]) >= 18
    assert 7 not in a["occured_leaf_id"] and 13 not in a["occured_leaf_id"]
    for x, y in zip(a["leaf_clusters_imgs"], b["leaf_clusters_imgs"]):
        assert x.shape == y.shape and torch.equal(x, y)
    assert torch.equal(a["leaf_cluster_silhouettes"], b["leaf_cluster_silhouettes"])
