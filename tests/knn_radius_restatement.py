"""NumPy restatement of ogs_knn_radius_count and ogs_knn_dbscan (include/ogs_knn.h) and of the two functions
opengaussian_amd.query builds on them: d2 in fp32 in the stated order, counts, cores, a min-root union-find over the core pairs,
the border rule by lexsort((j, d2)), the numbering by smallest core row.  tests/test_knn_radius_host.py pins it to a brute-force
flood fill and to scikit-learn."""
import numpy as np

from tests import knn_components_restatement as cr


def d2_matrix(q, p):
    """fp32 [m, n]: (dx*dx + dy*dy) + dz*dz with dx = x_q - x_p, every operation rounded to fp32"""
    q, p = np.asarray(q, np.float32), np.asarray(p, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (q[:, None, a] - p[None, :, a] for a in range(3))
        return (dx * dx + dy * dy) + dz * dz


def within(q, p, r2, qlab=None, plab=None):
    """bool [m, n]: d2 <= r2 as an fp32 compare (NaN on either side: False), and -- with labels -- equal labels >= 0"""
    with np.errstate(invalid="ignore"):
        ok = d2_matrix(q, p) <= np.float32(r2)
    if qlab is not None:
        ql, pl = np.asarray(qlab, np.int64), np.asarray(plab, np.int64)
        ok &= (ql[:, None] == pl[None, :]) & (ql[:, None] >= 0)
    return ok


def radius_count(points, queries, r2, ref_labels=None, query_labels=None):
    """count int32 [m]"""
    if len(points) == 0:
        return np.zeros(len(queries), np.int32)
    return within(queries, points, r2, query_labels, ref_labels).sum(1).astype(np.int32)


def dbscan(points, eps2, min_pts, labels=None):
    """(cluster int32 [n], core uint8 [n], degree int32 [n], sizes int32 [n], first int32 [n], count int32 [1])"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(pts)
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels, np.int64)
    near = within(pts, pts, eps2, lab, lab) if n else np.zeros((0, 0), bool)
    degree = near.sum(1).astype(np.int32)
    core = degree >= min_pts
    parent = np.arange(n, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in np.nonzero(core)[0].tolist():
        js = np.nonzero(near[i, :i] & core[:i])[0]                         # the core pairs (i, j) with j < i: every pair once
        for j in np.unique(parent[js]).tolist():                           # parent[j] stands for j: a member of the same set
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)                              # the smallest core row is the root
    root = np.full(n, -1, np.int64)
    d2 = d2_matrix(pts, pts) if n else np.zeros((0, 0), np.float32)
    for i in range(n):
        if core[i]:
            root[i] = find(i)
        else:
            js = np.nonzero(near[i] & core)[0]
            if len(js):
                root[i] = find(int(js[np.lexsort((js, d2[i, js]))[0]]))     # the smallest (d2, j)
    is_root = core & (root == np.arange(n))
    dense = np.cumsum(is_root) - 1
    cluster = np.where(root >= 0, dense[np.maximum(root, 0)], -1).astype(np.int32)
    C = int(is_root.sum())
    sizes, first = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    if C:
        sizes[:C] = np.bincount(cluster[cluster >= 0], minlength=C)[:C]
        first[:C] = np.nonzero(is_root)[0]
    return cluster, core.astype(np.uint8), degree, sizes, first, np.array([C], np.int32)


def flood_fill(points, eps2, min_pts, labels=None):
    """The same six arrays by brute force: a fill over the core graph from every unvisited core in row order, then the borders"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(pts)
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels, np.int64)
    d2 = d2_matrix(pts, pts)
    near = within(pts, pts, eps2, lab, lab)
    degree = near.sum(1).astype(np.int32)
    core = degree >= min_pts
    cluster = np.full(n, -1, np.int32)
    first = np.full(n, -1, np.int32)
    C = 0
    for s in range(n):
        if not core[s] or cluster[s] >= 0:
            continue
        cluster[s] = C
        stack = [s]
        while stack:
            for v in np.nonzero(near[stack.pop()] & core)[0]:
                if cluster[v] < 0:
                    cluster[v] = C
                    stack.append(int(v))
        first[C] = s
        C += 1
    for i in range(n):
        if not core[i]:
            best = None
            for j in np.nonzero(near[i] & core)[0].tolist():
                if best is None or (d2[i, j], j) < best:
                    best = (d2[i, j], j)
            if best is not None:
                cluster[i] = cluster[best[1]]
    sizes = np.zeros(n, np.int32)
    sizes[:C] = np.bincount(cluster[cluster >= 0], minlength=C)[:C] if C else 0
    return cluster, core.astype(np.uint8), degree, sizes, first, np.array([C], np.int32)


def segment_instances_dbscan(points, labels, eps, min_pts=8, min_size=1, ignore=()):
    """(instance int32 [n], num, instance_label [num], instance_size int32 [num]) of query.segment_instances_dbscan"""
    lab = np.asarray(labels, np.int64)
    lab = np.where((lab < 0) | np.isin(lab, np.asarray(list(ignore), np.int64)), -1, lab)
    cluster, _, _, sizes, first, count = dbscan(points, np.float32(eps) * np.float32(eps), min_pts, lab)
    C = int(count[0])
    keep = np.append(sizes[:C] >= min_size, False)                         # one spare entry: an empty table indexes it
    new_id = np.cumsum(keep) - 1
    at = np.where(cluster >= 0, cluster, C)
    instance = np.where(keep[at], new_id[at], -1).astype(np.int32)
    return instance, int(keep.sum()), lab[first[:C][keep[:C]]], sizes[:C][keep[:C]]


def density_filter(points, group=None, num_groups=1, eps=None, min_pts=8, min_share=None):
    """keep-mask bool [n] of query.density_filter"""
    n = len(points)
    g = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64)
    g = np.where((g < 0) | (g >= num_groups), -1, g)
    cluster, _, _, sizes, first, count = dbscan(points, np.float32(eps) * np.float32(eps), min_pts, g)
    C = int(count[0])
    keep = np.zeros(max(C, 1), bool)
    cgroup = g[first[:C]]
    for grp in range(num_groups):
        cs = np.nonzero(cgroup == grp)[0]
        if len(cs) == 0:
            continue
        if min_share is None:
            keep[cs[np.argmax(sizes[cs])]] = True                          # argmax: the first of equal sizes
        else:
            keep[cs[sizes[cs].astype(np.float64) >= float(min_share) * float(sizes[cs].sum())]] = True
    return (cluster >= 0) & keep[np.maximum(cluster, 0)]


canonical = cr.canonical
