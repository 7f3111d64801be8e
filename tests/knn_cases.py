"""Seeded inputs shared by tests/test_knn_host.py (which checks their margin conditions on the CPU) and
tests/test_37_knn_gpu.py (which runs the kernel on them)."""
import numpy as np

MANY_GROUPS = 640


def cloud(n, seed, shift=0.0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)).astype(np.float32) + np.float32(shift)).astype(np.float32)


def many_groups(seed=77):
    """640 groups of 0..300 rows, empty ones at the start, in the middle and at the end; rows of no group (-1) interleaved;
    the caller's order is shuffled, so that the stable sort has work to do.  Returns (points, group, sizes)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 301, MANY_GROUPS)
    sizes[[0, 1, 319, 320, 321, MANY_GROUPS - 1]] = 0
    sizes[[2, 100]] = [1, 2]
    group = np.concatenate([np.repeat(np.arange(MANY_GROUPS), sizes), np.full(5000, -1)])
    rng.shuffle(group)
    n = len(group)
    # every group is its own blob, so that groups differ in scale and offset
    centre = rng.standard_normal((MANY_GROUPS + 1, 3)).astype(np.float32) * 3.0
    spread = (0.05 + rng.random(MANY_GROUPS + 1) * 0.5).astype(np.float32)
    points = (centre[group] + rng.standard_normal((n, 3)).astype(np.float32) * spread[group][:, None]).astype(np.float32)
    return points, group.astype(np.int64), sizes


def click_variant(seed=5):
    """One object-sized selection for the k_scale = 2, std_weight = 0.1 rule of scripts/render_by_click.py."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((700, 3)) * 0.2).astype(np.float32)
    p[::23] += (rng.random((len(p[::23]), 3)) * 4.0 - 2.0).astype(np.float32)
    return p


def tie_clouds(K):
    """Exact ties at the K-th value.  'dup': one point present 2, another 3 and a third K + 2 times among distinct points --
    for the rows of the last the K-th value is a tie AND zero.  'lattice': a 6 x 6 x 6 integer lattice, where the squared
    distances are small integers and whole shells of equal distance straddle K."""
    rng = np.random.default_rng(900 + K)
    base = rng.random((40, 3)).astype(np.float32)
    dup = np.concatenate([base, base[[0]], base[[1]], base[[1]], np.repeat(base[[2]], K + 1, axis=0)])
    rng.shuffle(dup)
    g = np.arange(6, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return {"dup": dup.astype(np.float32), "lattice": lattice.astype(np.float32)}
