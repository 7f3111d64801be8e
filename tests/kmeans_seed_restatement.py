"""NumPy restatement of the wide seeding (include/ogs_kmeans.h, "wide seeding"): float32 for dist() in the header's order, Python
integers for the draw, no pruning.  The library's rows, C, ids, d2 and stats[0] are np.array_equal to what seed() returns.

prune_report() replays the header's pruning rule on top of it: how many (row, round) pairs the rule skips, and whether it ever
skipped a row that would have changed."""
import collections

import numpy as np

U = 2.0 ** -24
MASK64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15

Seeded = collections.namedtuple("Seeded", "C rows ids d2 seeded E")


def rand64(seed, r):
    """splitmix64 of the header: the r-th output of the stream that starts at `seed`"""
    z = (seed + (r + 1) * GAMMA) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def pick(q, rnd):
    """the smallest i whose inclusive prefix sum of the integer masses q exceeds t = (rnd * T) >> 64; None when T = 0"""
    q = np.asarray(q, np.int64)
    T = int(q.sum())
    if T == 0:
        return None
    t = (rnd * T) >> 64
    return int(np.searchsorted(np.cumsum(q), t, side="right"))


def masses(value, E):
    """q_i = floor(ldexp(value_i, 31 - E)) as int64"""
    return np.floor(np.ldexp(np.asarray(value, np.float32), 31 - int(E))).astype(np.int64)


def exponent(value):
    """the frexp exponent of the largest value (0 for 0)"""
    return int(np.frexp(np.float32(np.max(value)))[1]) if len(value) else 0


def points(X, scale=None):
    """y_ij = fl32(scale_i * x_ij)"""
    X = np.ascontiguousarray(X, np.float32)
    return X if scale is None else (np.asarray(scale, np.float32)[:, None] * X).astype(np.float32)


def dist(Y, c):
    """fp32 dist(y_i, c) of every row of Y [n, D]: differences first, accumulator j mod 256 in ascending j, then the binary tree
    s[q] = s[2q] + s[2q + 1] over the 256 accumulators (zeros past D are exact, so narrow rows fold a shorter table)"""
    Y = np.asarray(Y, np.float32)
    n, D = Y.shape
    d = Y - np.asarray(c, np.float32)[None, :]
    t = d * d
    assert t.dtype == np.float32
    P = 256 if D > 256 else 1 << max(D - 1, 0).bit_length()
    pad = np.zeros((n, -(-D // P) * P), np.float32)
    pad[:, :D] = t
    s = pad[:, :P].copy()
    for j0 in range(P, pad.shape[1], P):
        s = s + pad[:, j0:j0 + P]
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2]
    return s[:, 0]


def first_pick(w, seed):
    """the row round 0 draws"""
    w = np.asarray(w, np.float32)
    return pick(masses(w, exponent(w)), rand64(seed, 0))


def seed(X, k, w=None, scale=None, seed=0, C_fill=0.0, on_round=None):
    """Seeded(C [k, D], rows [k], ids [N], d2 [N], seeded, E).  C rows past `seeded` keep C_fill, rows are -1 there.
    on_round(r, Y, C, ids, d2, new_d): called in every round r >= 1 before the rows change (prune_report hooks in here)."""
    Y = points(X, scale)
    N, D = Y.shape
    w = np.ones(N, np.float32) if w is None else np.asarray(w, np.float32)
    C = np.full((k, D), C_fill, np.float32)
    rows = np.full(k, -1, np.int64)
    ids = np.zeros(N, np.int64)
    d2 = np.zeros(N, np.float32)
    i = first_pick(w, seed) if N else None
    if i is None:
        return Seeded(C, rows, ids, d2, 0, 0)
    rows[0], C[0] = i, Y[i]
    d2 = dist(Y, C[0])
    E = exponent(w * d2)
    for r in range(1, k):
        i = pick(masses(w * d2, E), rand64(seed, r))
        if i is None:
            return Seeded(C, rows, ids, d2, r, E)
        rows[r], C[r] = i, Y[i]
        nd = dist(Y, C[r])
        if on_round is not None:
            on_round(r, Y, C, ids, d2, nd)
        closer = nd < d2
        d2 = np.where(closer, nd, d2)
        ids = np.where(closer, r, ids)
    return Seeded(C, rows, ids, d2, k, E)


def skip_rule(d, b):
    """the header's pruning rule in fp32: d = d2_i, b = dist(C[r], C[ids_i])"""
    d, b = np.asarray(d, np.float32), np.asarray(b, np.float32)
    lhs = b * np.float32(1.0 - 2.0 ** -10)
    rhs = (np.float32(4.0) * d) * np.float32(1.0 + 2.0 ** -10)
    return (d == 0) | ((d >= np.float32(2.0 ** -100)) & (lhs >= rhs))


def prune_report(X, k, w=None, scale=None, seed_=0):
    """(Seeded, skipped pairs, pairs of the rounds r >= 1, rows the rule skipped although they would have changed)"""
    tally = {"skipped": 0, "wrong": 0}

    def on_round(r, Y, C, ids, d2, nd):
        cc = dist(C[:r], C[r])
        skip = skip_rule(d2, cc[ids])
        tally["skipped"] += int(skip.sum())
        tally["wrong"] += int((skip & (nd < d2)).sum())

    out = seed(X, k, w, scale, seed_, on_round=on_round)
    return out, tally["skipped"], len(X) * max(out.seeded - 1, 0), tally["wrong"]
