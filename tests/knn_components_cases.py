"""Case builders of the connected-components tests (tests/test_knn_components_host.py asserts what the GPU tests rely on)."""
import numpy as np

BLOCK_SLOTS = 256                               # slots one workgroup of the hook kernel takes (kBlock of csrc/ogs_common.h)
I32 = np.iinfo(np.int32)
PATH_N = 4097                                   # 17 workgroups of one slot per row
PATH_SEED = 3
PATH_CUTS = (700, 2048, 3500)                   # chain positions whose link is removed
STAR_N = 3000
TABLE_SIZES = ((63, 4), (64, 4), (65, 4), (64, 1), (65, 16), (255, 1), (257, 1), (5000, 16))     # n * K = 252 / 256 / 260, 255 / 257


def path_graph(n=PATH_N, seed=PATH_SEED, cuts=()):
    """K = 1: row p[t] lists p[t - 1] for a seeded permutation p -- one chain through every workgroup, in no order the row
    numbers know of; p[0] and the positions in `cuts` list nothing.  Returns (idx [n, 1], p)."""
    p = np.random.default_rng(seed).permutation(n)
    idx = np.full((n, 1), -1, np.int32)
    idx[p[1:], 0] = p[:-1]
    for t in cuts:
        idx[p[t], 0] = -1
    return idx, p


def star(n=STAR_N, K=1):
    """every slot of every row names the last row (whose own slots are self slots)"""
    return np.full((n, K), n - 1, np.int32)


def one_way():
    """Rows 0..7: a cluster, each listing its two ring neighbours.  Row 8 lists row 3 and nothing lists row 8.  Row 9 lists
    nothing and is listed by nothing."""
    idx = np.full((10, 2), -1, np.int32)
    for i in range(8):
        idx[i] = ((i + 1) % 8, (i + 7) % 8)
    idx[8, 1] = 3
    return idx


def junk_slots(n=200, K=3, seed=5):
    """a random table in which four slots of five lie outside [0, n), in every flavour"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n, (n, K)).astype(np.int64)
    hit = rng.random((n, K)) < 0.8
    idx[hit] = np.array([-1, n, n + 1, -2, I32.min, I32.max], np.int64)[np.arange(int(hit.sum())) % 6]
    return idx.astype(np.int32)


def lattice(nx=12, ny=9, gap_after=(5,)):
    """Integer points (x, y, 0), the columns after those in `gap_after` shifted by one more unit: squared distances are small
    integers, exact in fp32.  Neighbours in a column and in a piece are at d2 = 1, across a gap at d2 = 4."""
    xs = np.arange(nx, dtype=np.int64)
    for g in gap_after:
        xs[g + 1:] += 1
    x, y = np.meshgrid(xs, np.arange(ny), indexing="ij")
    return np.stack((x.reshape(-1), y.reshape(-1), np.zeros(nx * ny, np.int64)), 1).astype(np.float32)


def checkerboard_labels(points, holes=0, seed=1):
    """class (x + y) % 2, and `holes` seeded rows set to -1"""
    lab = ((points[:, 0] + points[:, 1]).astype(np.int64) % 2).astype(np.int32)
    if holes:
        lab[np.random.default_rng(seed).choice(len(lab), holes, replace=False)] = -1
    return lab


def wall_labels(points, x_wall=3.0):
    """one class everywhere, the column x = x_wall inactive: a wall that bridges nothing"""
    lab = np.zeros(len(points), np.int32)
    lab[points[:, 0] == x_wall] = -1
    return lab


def blobs(n, seed, centres=4, spread=0.05):
    """n points in `centres` seeded Gaussian blobs inside the unit cube, rows shuffled"""
    rng = np.random.default_rng(seed)
    c = rng.random((centres, 3))
    which = rng.integers(0, centres, n)
    return (c[which] + spread * rng.standard_normal((n, 3))).astype(np.float32)


def threshold_of(d2, column=1):
    """a threshold that cuts a real table into many pieces: the median of one column of its distances"""
    col = np.asarray(d2)[:, min(column, d2.shape[1] - 1)]
    return np.float32(np.median(col[np.isfinite(col)])) if np.isfinite(col).any() else np.float32(0)


def permute_rows(idx, d2, seed):
    """The same graph with its rows renumbered: new row pos[i] is old row i.  Returns (idx', d2', pos)."""
    n = len(idx)
    perm = np.random.default_rng(seed).permutation(n)                      # new row r is old row perm[r]
    pos = np.empty(n, np.int64)
    pos[perm] = np.arange(n)
    old = idx[perm].astype(np.int64)
    new = np.where((old >= 0) & (old < n), pos[np.clip(old, 0, n - 1)], old)
    return new.astype(np.int32), None if d2 is None else d2[perm], pos


def permute_slots(idx, d2, seed):
    """every row's slots in a seeded order of its own"""
    rng = np.random.default_rng(seed)
    order = np.argsort(rng.random(idx.shape), axis=1)
    return np.take_along_axis(idx, order, 1), None if d2 is None else np.take_along_axis(d2, order, 1)


# ---- scenes of tests/test_38b_instances_gpu.py ------------------------------------------------------------------------------------
INSTANCE_K = 8
INSTANCE_MAX_DIST = 0.25
FLOATER = 3                                     # points of a planted floater


def instance_scene(seed=11):
    """Three classes (0, 1, 2) and a class to ignore (7): per class a few blobs of 60..120 points far apart, plus two 3-point
    floaters of class 0 and 1 away from everything, plus unlabelled (-1) points sprinkled THROUGH the blobs.
    Returns (points, labels, blob id per row: 0.. for the blobs, -1 for floaters and unlabelled rows)."""
    rng = np.random.default_rng(seed)
    centres = np.array([[0, 0, 0], [2, 0, 0], [4, 0, 0], [0, 2, 0], [2, 2, 0], [4, 2, 0], [0, 4, 0], [2, 4, 0]], np.float64)
    cls = [0, 1, 0, 2, 1, 0, 7, 2]
    pts, lab, blob = [], [], []
    for b, (c, l) in enumerate(zip(centres, cls)):
        m = int(rng.integers(60, 121))
        pts.append(c + 0.08 * rng.standard_normal((m, 3)))
        lab += [l] * m
        blob += [b] * m
    for c, l in (([1, 1, 3], 0), ([3, 1, 3], 1)):
        pts.append(np.asarray(c, np.float64) + 0.01 * rng.standard_normal((FLOATER, 3)))
        lab += [l] * FLOATER
        blob += [-1] * FLOATER
    m = 40
    pts.append(centres[rng.integers(0, len(centres), m)] + 0.08 * rng.standard_normal((m, 3)))
    lab += [-1] * m
    blob += [-1] * m
    order = rng.permutation(len(lab))
    return (np.concatenate(pts).astype(np.float32)[order], np.asarray(lab, np.int64)[order], np.asarray(blob, np.int64)[order])


FILTER_K = 8
FILTER_GROUPS = 3


def filter_scene(seed=21):
    """FILTER_GROUPS groups, each a main blob of 300 points (sigma 0.1) and a DENSE floater of 40 points (sigma 0.004) two
    units above it, plus rows of no group (-1 and FILTER_GROUPS).  The floater is denser than the blob, so a filter on the
    mean distance to the nearest neighbours keeps it.  Returns (points, group, main: bool, True on the main blobs)."""
    rng = np.random.default_rng(seed)
    pts, grp, main = [], [], []
    for g in range(FILTER_GROUPS):
        c = np.array([3.0 * g, 0, 0])
        pts.append(c + 0.1 * rng.standard_normal((300, 3)))
        pts.append(c + np.array([0, 0, 2.0]) + 0.004 * rng.standard_normal((40, 3)))
        grp += [g] * 340
        main += [True] * 300 + [False] * 40
    pts.append(np.array([1.5, 0, 0]) + 0.1 * rng.standard_normal((20, 3)))
    grp += [-1] * 10 + [FILTER_GROUPS] * 10
    main += [False] * 20
    order = rng.permutation(len(grp))
    return (np.concatenate(pts).astype(np.float32)[order], np.asarray(grp, np.int64)[order], np.asarray(main, bool)[order])
