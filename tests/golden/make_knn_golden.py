"""Generate tests/golden/knn_golden.npz by RUNNING THE REFERENCE's own code on the CPU.

Run in the build container only (``python tests/golden/make_knn_golden.py``): /root/reference never travels, only the
vectors do.

(a) ``distCUDA2`` of scene/gaussian_model.py:28-36 (the scipy KDTree form the reference substitutes for simple_knn),
    compiled from the source text (ast) because the module imports `plyfile`; run on seeded clouds.
(b) lines 292-309 of gaussian_renderer/__init__.py -- the `post_process` block of render() -- taken from the source text and
    executed as they stand on a handful of point sets, with ``pytorch3d.ops.knn_points`` replaced by a float64 brute-force
    stand-in that returns the ascending squared distances (``.dists`` of ``knn_points(x, x, K=K)``).  Stored: the points, the
    mask the block writes into ``filter_idx``, and its mean and std.

Every stored case of (b) is asserted to have no row within 1e-6 (relative) of its threshold, so that fp32 distances and the
order of a sum cannot change a decision.  The exception is a case whose K nearest distances are ALL exactly zero (K = 1: only
the self-distance): row values and threshold are then exact zeros in any arithmetic and `0 < 0` keeps nothing everywhere.
"""
import ast
import os
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_MODEL = "/root/reference/scene/gaussian_model.py"
REF_RENDER = "/root/reference/gaussian_renderer/__init__.py"
BLOCK = (292, 309)                     # 1-based, inclusive

DIST_CASES = ["n5", "n64", "n1000_dup", "n4097_shift"]
MASK_SIZES = [1, 3, 9, 10, 16, 100, 1024, 1500]
MASK_KINDS = ["uniform", "clustered"]


def dist_cloud(name):
    """Seeded clouds for distCUDA2 (shared with the tests through the stored points)."""
    n = int(name[1:].split("_")[0])
    rng = np.random.default_rng(4100 + n)
    p = rng.random((n, 3)).astype(np.float32)
    if name.endswith("_dup"):
        p[n // 2:n // 2 + 50] = p[:50]             # exact duplicates: zero distances among the nearest
        p[-3:] = p[0]                              # one point present five times
    if name.endswith("_shift"):
        p = p + np.float32(1000.0)
    return p


def mask_cloud(n, kind):
    rng = np.random.default_rng(5200 + 7 * n + (kind == "clustered"))
    if kind == "uniform":
        return rng.random((n, 3)).astype(np.float32)
    p = (rng.standard_normal((n, 3)) * 0.1).astype(np.float32)
    out = rng.random(n) < 0.06                      # far outliers around a tight cluster
    p[out] = (rng.random((int(out.sum()), 3)) * 6.0 - 3.0).astype(np.float32)
    return p


def load_distcuda2():
    from scipy.spatial import KDTree
    ns = {"torch": torch, "np": np, "KDTree": KDTree}
    tree = ast.parse(open(REF_MODEL).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "distCUDA2"]
    assert len(fn) == 1
    exec(compile(ast.Module(body=fn, type_ignores=[]), REF_MODEL, "exec"), ns)
    return ns["distCUDA2"]


def knn_points(p1, p2, K=1, **_):
    d2 = ((p1.double()[:, :, None, :] - p2.double()[:, None, :, :]) ** 2).sum(-1)
    vals, idx = torch.topk(d2, K, dim=-1, largest=False, sorted=True)
    return types.SimpleNamespace(dists=vals, idx=idx, knn=None)


def load_block():
    lines = open(REF_RENDER).read().split("\n")[BLOCK[0] - 1:BLOCK[1]]
    src = textwrap.dedent("\n".join(lines))
    assert src.startswith("max_time = 5") and "pytorch3d.ops.knn_points(" in src and "filter_idx[filter_idx != 0] = mask" in src
    assert src.rstrip().endswith("max_time -= 1")
    return compile(src, REF_RENDER, "exec")


def run_block(code, points):
    p3d = types.SimpleNamespace(ops=types.SimpleNamespace(knn_points=knn_points))
    n = points.shape[0]
    ns = {"pytorch3d": p3d, "torch": torch, "post_process": True, "means3D": torch.from_numpy(points),
          "filter_idx": torch.ones(n, dtype=torch.bool)}
    exec(code, ns)
    assert ns["max_time"] == 4
    vals = ns["nearest_k_distance"]
    assert vals.dtype == torch.float64 and vals.shape == (1, n, int(n ** 0.5))
    return (ns["filter_idx"].numpy().copy(), float(ns["mean_nearest_k_distance"]), float(ns["std_nearest_k_distance"]),
            vals[0].mean(dim=-1).numpy())


def main():
    store = {"dist_cases": np.array(DIST_CASES), "mask_sizes": np.array(MASK_SIZES), "mask_kinds": np.array(MASK_KINDS)}
    dist = load_distcuda2()
    for name in DIST_CASES:
        p = dist_cloud(name)
        out = dist(torch.from_numpy(p))
        assert out.dtype == torch.float32 and out.shape == (len(p),)
        store[f"dist/{name}/points"] = p
        store[f"dist/{name}/out"] = out.numpy()
        print("distCUDA2", name, "mean %.3e" % float(out.mean()), "zeros", int((out == 0).sum()))
    code = load_block()
    for n in MASK_SIZES:
        for kind in MASK_KINDS:
            p = mask_cloud(n, kind)
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")             # std of one value (n = 1): nan, as the reference gets it
                mask, mean, std, row_mean = run_block(code, p)
            limit = mean + std
            if np.isfinite(limit) and not (limit == 0.0 and not row_mean.any()):
                margin = np.abs(row_mean - limit) / abs(limit)
                assert margin.min() > 1e-6, (n, kind, margin.min())
                note = "margin %.2e" % margin.min()
            else:
                assert not mask.any()
                note = "limit %r: nothing kept" % limit
            k = f"mask/{n}/{kind}"
            store[k + "/points"], store[k + "/mask"] = p, mask
            store[k + "/mean"], store[k + "/std"] = np.float64(mean), np.float64(std)
            print("post_process", n, kind, "kept", int(mask.sum()), note)
    path = os.path.join(HERE, "knn_golden.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
