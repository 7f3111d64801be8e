"""Seeded case builders of the wide-seeding tests (tests/test_kmeans_seed_host.py, tests/test_22b_kmeans_seed_gpu.py), and the
restatement's answer for each of them, computed once and shared."""
import functools

import numpy as np

from tests import kmeans_seed_restatement as sr

SEED_ROWS = 256        # rows of one row-pass workgroup and of one block sum (ogs_kmeans_wide_seed_rows; the tests compare)
PICK_THREADS = 1024    # the pick workgroup: past SEED_ROWS * PICK_THREADS rows every thread walks a run of block sums
MAX_DIM = 1024
MAX_K = 16384

# (N, D, k): the issue's D (1, 3, 6, 63, 64, 65, 255, 257, 1024), N (1; k; 63, 64, 65; one block - 1, a block, a block + 1; two blocks
# + 1; ~5000: twenty blocks under the pick scan) and k (1, 2, 33, N), not as a full product; then D on both sides of every width at
# which the lanes per row (1, 2, 4 ... 64: D = 4, 8 ... 256) or the trips of a whole wave (D = 256, 512, 768) change; then N past
# one and past two block sums per pick thread (narrow rows: the restatement stays cheap)
SHAPES = [(1, 1, 1), (1, 3, 2), (2, 6, 2), (33, 63, 33), (63, 64, 33), (64, 65, 2), (65, 255, 33), (65, 1, 65), (64, 6, 64),
          (SEED_ROWS - 1, 257, 33), (SEED_ROWS, 3, 33), (SEED_ROWS + 1, 64, 2), (SEED_ROWS + 1, 63, 33),
          (2 * SEED_ROWS + 1, 6, 33), (2 * SEED_ROWS + 1, 1024, 2), (5000, 65, 33), (5000, 1, 33), (5000, 255, 1), (70, 1024, 33),
          (300, 257, 2)]
SHAPES += [(200, D, 5) for D in (4, 5, 8, 9, 16, 17, 32, 33, 128, 129, 256, 512, 513, 768, 769)]
SHAPES += [(SEED_ROWS * PICK_THREADS + 300, 1, 3), (2 * SEED_ROWS * PICK_THREADS + 77, 3, 4)]

MIXTURE_DIMS = (16, 67)
MIXTURE_SEEDS = (0, 1, 2, 3, 4, 5)
MIXTURE_K = 32


@functools.lru_cache(maxsize=None)
def shape_case(N, D, k):
    """(X, w or None, scale or None, seed, restatement): loose clumps, so that later rounds change some rows and leave others;
    every other shape has weights (with zeros) and every third a row scale"""
    idx = SHAPES.index((N, D, k))
    rng = np.random.default_rng([5, N, D, k])
    clumps = rng.normal(size=(max(1, min(N, 7)), D)) * 3.0
    X = (clumps[rng.integers(0, len(clumps), size=N)] + rng.normal(size=(N, D))).astype(np.float32)
    w = None
    if idx % 2 == 1:
        w = rng.uniform(0.25, 4.0, size=N).astype(np.float32)
        w[::5] = 0.0
        if not w.any():
            w[-1] = 1.5
    scale = rng.uniform(0.5, 2.0, size=N).astype(np.float32) if idx % 3 == 2 else None
    seed = 1000 + idx
    return X, w, scale, seed, sr.seed(X, k, w, scale, seed, C_fill=C_FILL)


C_FILL = -12345.0      # what the GPU test leaves in C before the call: rows that are not seeded keep it


@functools.lru_cache(maxsize=None)
def mixture(D, seed, N=4096, small=20, clusters=32, sigma=0.05):
    """(X [N, D] fp32, labels [N]): one cluster of N - 31 * 20 = 3476 rows and 31 of 20 rows each, sigma = 0.05 about centres
    4 * N(0, 1), in random row order"""
    rng = np.random.default_rng([17, D, seed])
    centres = 4.0 * rng.normal(size=(clusters, D))
    labels = np.concatenate([np.zeros(N - (clusters - 1) * small, np.int64), np.repeat(np.arange(1, clusters), small)])
    labels = rng.permutation(labels)
    X = centres[labels] + sigma * rng.normal(size=(N, D))
    return X.astype(np.float32), labels


@functools.lru_cache(maxsize=None)
def mixture_seeded(D, seed):
    """prune_report of the mixture with k = 32: (Seeded, skipped, pairs, wrongly skipped)"""
    X, _ = mixture(D, seed)
    return sr.prune_report(X, MIXTURE_K, seed_=seed)


def clusters_hit(labels, rows):
    return len(set(labels[np.asarray(rows)[np.asarray(rows) >= 0]].tolist()))


def randperm_rows(N, k, seed):
    """the rows build_codebook(init=None) starts from when every row is valid"""
    import torch
    return torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))[:k].numpy()


def duplicated(N=300, D=20, m=7, seed=4):
    """m distinct rows, each many times over, in random order"""
    rng = np.random.default_rng([23, N, D, m, seed])
    base = rng.normal(size=(m, D)).astype(np.float32)
    which = rng.permutation(np.arange(N) % m)
    return base[which], which
