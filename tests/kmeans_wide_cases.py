"""Seeded case builders of the wide k-means tests (tests/test_kmeans_wide_host.py, tests/test_22_kmeans_wide_gpu.py).

The sizes that shape csrc/kmeans_wide.hip are restated here; the tests check them against the library's getters, so that the
shapes below sit on both sides of each."""
import functools

import numpy as np

ROW_TILE = 64          # rows of a workgroup (48 for D > 384, 32 for D > 512, 16 for D > 768: LDS_DIMS below)
CENTRE_TILE = 16
DIM_STEP = 32
STAGE = 4096           # centres packed at a time
MAX_DIM = 1024
MAX_K = 16384
LDS_DIMS = (384, 512, 768)  # the last D of the 64-row, of the 48-row and of the 32-row tile
METRICS = ("l2", "cosine")

# (N, D, k) of the planted-partition test: the issue's fixed shapes, then N, k, D around every tile size, the widths at which the
# row tile changes, the largest D, and a k past one stage
PLANTED_SHAPES = [(1, 17, 1), (63, 17, 5), (65, 33, 17), (1000, 100, 37), (257, 512, 64), (300, 1024, 3), (777, 17, 300),
                  (ROW_TILE - 1, 33, 5), (ROW_TILE + 1, 33, 5), (2 * ROW_TILE + 1, 9, 3),
                  (100, 17, CENTRE_TILE - 1), (100, 17, CENTRE_TILE), (100, 17, CENTRE_TILE + 1), (100, 17, 2 * CENTRE_TILE + 1),
                  (100, DIM_STEP - 1, 5), (100, DIM_STEP, 5), (100, DIM_STEP + 1, 5),
                  (70, LDS_DIMS[0], 5), (70, LDS_DIMS[0] + 1, 5), (70, LDS_DIMS[1] + 1, 5), (70, LDS_DIMS[2], 5), (70, LDS_DIMS[2] + 1, 5),
                  (97, LDS_DIMS[1], 33),
                  (40, MAX_DIM, 20), (50, 17, STAGE + 1)]

# (name, N, D, k, metric, distribution, offset) of the near-minimiser test
RANDOM_CASES = [("uniform/100", 1000, 100, 37, "l2", "uniform", 0.0),
                ("uniform/17", 777, 17, 300, "l2", "uniform", 0.0),
                ("uniform/512", 520, 512, 64, "l2", "uniform", 0.0),
                ("uniform+100", 1000, 33, 100, "l2", "uniform", 100.0),
                ("normal/64", 1000, 64, 50, "cosine", "normal", 0.0),
                ("normal/512", 600, 512, 320, "cosine", "normal", 0.0)]


def unit(a):
    """rows of `a` normalised in float64, rounded to fp32: what a caller hands the cosine metric"""
    a = np.asarray(a, np.float64)
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def planted(N, D, k, metric, seed=0):
    """(X [N, D] fp32, C [k, D] fp32, labels [N]): rows within 1e-3 of their centre, centres far apart -- the gap between the
    best and the second-best centre is orders of magnitude above any rounding.  Cosine: unit centres, rows at random scales."""
    rng = np.random.default_rng([seed, N, D, k, METRICS.index(metric)])
    C = rng.normal(size=(k, D)) * 10.0
    if k > 1 and D == 1:
        C = (np.arange(k, dtype=np.float64)[:, None] - k / 2) * 10.0
    labels = rng.permutation(np.arange(N) % k) if N >= k else rng.permutation(k)[:N]
    if metric == "cosine":
        C = unit(C).astype(np.float64)
        X = (C[labels] + 1e-3 * rng.normal(size=(N, D)) / np.sqrt(D)) * np.exp2(rng.integers(-3, 4, size=(N, 1)))
    else:
        X = C[labels] + 1e-3 * rng.normal(size=(N, D))
    return X.astype(np.float32), C.astype(np.float32), labels.astype(np.int64)


@functools.lru_cache(maxsize=None)
def random_case(name):
    """(X, C, metric) of RANDOM_CASES[name]: centres are jittered data rows (cosine: normalised)"""
    _, N, D, k, metric, distribution, offset = next(c for c in RANDOM_CASES if c[0] == name)
    rng = np.random.default_rng([7, N, D, k])
    X = (rng.random(size=(N, D)) if distribution == "uniform" else rng.normal(size=(N, D))) + offset
    C = X[rng.permutation(N)[:k]] + 0.05 * rng.normal(size=(k, D))
    X = X.astype(np.float32)
    return X, (unit(C) if metric == "cosine" else C.astype(np.float32)), metric


def weights(N, seed, zeros=True):
    """positive fp32 row weights, every fifth one exactly 0"""
    w = np.random.default_rng([11, N, seed]).uniform(0.25, 4.0, size=N).astype(np.float32)
    if zeros:
        w[::5] = 0.0
    return w


def codebook_scene(N=2000, D=64, k=8, seed=3):
    """(features [N, D] fp32, directions [k, D] fp32 unit, labels [N], init [k, D]): unit-vector clusters of unequal sizes; init is
    one row of every cluster"""
    rng = np.random.default_rng([seed, N, D, k])
    dirs = unit(rng.normal(size=(k, D)))
    labels = np.sort(rng.integers(0, k, size=N))
    labels[:k] = np.arange(k)                                   # no cluster is empty
    labels = rng.permutation(labels)
    X = unit(dirs[labels].astype(np.float64) + 0.02 * rng.normal(size=(N, D)) / np.sqrt(D))
    first = np.array([int(np.flatnonzero(labels == c)[0]) for c in range(k)])
    return X, dirs, labels.astype(np.int64), X[first].copy()
