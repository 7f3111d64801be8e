"""Case builders of the kNN graph tests (tests/test_knn_graph_host.py asserts what the GPU tests rely on)."""
import numpy as np

CHUNK = 256                                     # ogs_knn_transpose_chunk(): the GPU test asserts that the library says the same
I32 = np.iinfo(np.int32)
TABLE_N = (1, 2, 5, 63, 64, 65, 257)            # clouds of the neighbour tables; the ones with n <= K hold -1 slots
TABLE_K = (1, 3, 4, 16, 32)
WIDTHS = (1, 3, 4, 5, 6, 64, 65)                # both column forms, one and several lanes per slot (8 L >= D: 65 takes 16 lanes)
HUB_DEGREES = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)


def invalid_values(R):
    """every flavour of an index outside [0, R)"""
    return np.array([-1, R, I32.min, I32.max], np.int64)


def random_idx(n, K, R, seed, bad=0.2):
    """idx int32 [n, K] with values in [0, R) and a share `bad` of invalid ones of every flavour (R = 0: all invalid)"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, max(R, 1), (n, K)).astype(np.int64)
    hit = rng.random((n, K)) < (bad if R > 0 else 2.0)
    flavours = invalid_values(R)
    idx[hit] = flavours[np.arange(int(hit.sum())) % 4]           # all four, as long as four slots are hit
    return idx.astype(np.int32)


def weights(idx, R, seed, positive=False):
    """fp32 weights with NaN parked in the invalid slots: nothing may read those as values"""
    rng = np.random.default_rng(seed)
    w = rng.random(idx.shape) + 0.1 if positive else rng.standard_normal(idx.shape)
    w = w.astype(np.float32)
    w[(idx < 0) | (idx.astype(np.int64) >= R)] = np.nan
    return w


def hub_graph(seed=7, n=400, K=4):
    """A square graph (R = n) with n * K = 1600 slots: rows 0..3 are hubs with in-degrees HUB_DEGREES exactly -- below, at and
    above the chunk size and past two chunks -- the remaining 300-odd slots point at random rows of [4, n / 2) or nowhere (every
    invalid flavour), so that the rows from n / 2 on have no incoming edge; row n - 1 has invalid slots only."""
    rng = np.random.default_rng(seed)
    E = n * K
    assert sum(HUB_DEGREES) + 300 <= E - K
    flat = np.empty(E, np.int64)
    free = rng.permutation(E - K)                               # the last row's slots are set below
    pos = 0
    for hub, deg in enumerate(HUB_DEGREES):
        flat[free[pos:pos + deg]] = hub
        pos += deg
    rest = free[pos:]
    flat[rest] = rng.integers(4, n // 2, len(rest))
    bad = rest[rng.random(len(rest)) < 0.15]
    flat[bad] = invalid_values(n)[np.arange(len(bad)) % 4]
    flat[E - K:] = invalid_values(n)[np.arange(K) % 4]
    return flat.reshape(n, K).astype(np.int32)


def one_target(n=65, K=16, R=9, target=5):
    """every slot points at one row"""
    return np.full((n, K), target, np.int32)


def sparse_rows(seed=3, n=256, K=16, R=70_000):
    """n * K = 4096 slots over 70 000 rows: three radix digits, most rows empty"""
    return random_idx(n, K, R, seed, bad=0.05)


def features(n, D, seed):
    return np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)
