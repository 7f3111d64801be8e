"""NumPy restatement of ogs_knn_components (include/ogs_knn.h) and of the two functions opengaussian_amd.query builds on it: a
union-find with min-root hooking in a plain loop over the slots, then the numbering by ascending first row.
tests/test_knn_components_host.py pins it to a brute-force flood fill."""
import numpy as np


def edge_mask(idx, d2=None, max_d2=None, labels=None):
    """bool [n, K]: the slots that are edges (a self slot counts as one here; it joins nothing)"""
    idx = np.asarray(idx, np.int64)
    n = idx.shape[0]
    ok = (idx >= 0) & (idx < n)
    j = np.where(ok, idx, 0)
    if labels is not None:
        lab = np.asarray(labels, np.int64)
        ok &= (lab[:, None] >= 0) & (lab[j] >= 0) & (lab[:, None] == lab[j])
    if d2 is not None and max_d2 is not None:
        with np.errstate(invalid="ignore"):
            ok &= np.asarray(d2, np.float32) <= np.float32(max_d2)          # NaN on either side: False
    return ok


def components(idx, d2=None, max_d2=None, labels=None):
    """(comp int32 [n], count int32 [1], sizes int32 [n], first int32 [n]) as the header states them"""
    idx = np.asarray(idx, np.int64)
    n, K = idx.shape
    active = np.ones(n, bool) if labels is None else np.asarray(labels, np.int64) >= 0
    parent = np.arange(n, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    rows, cols = np.nonzero(edge_mask(idx, d2, max_d2, labels))
    for i, j in zip(rows.tolist(), idx[rows, cols].tolist()):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)                                  # the smallest member is the root
    root = np.array([find(i) for i in range(n)], np.int64).reshape(n)
    is_root = active & (root == np.arange(n))
    dense = np.cumsum(is_root) - 1
    comp = np.where(active, dense[root], -1).astype(np.int32)
    C = int(is_root.sum())
    sizes = np.zeros(n, np.int32)
    first = np.full(n, -1, np.int32)
    sizes[:C] = np.bincount(comp[active], minlength=C)[:C] if C else 0
    first[:C] = np.nonzero(is_root)[0]
    return comp, np.array([C], np.int32), sizes, first


def segment_instances(idx, d2, labels, max_dist=None, min_size=1, ignore=()):
    """(instance int32 [n], num, instance_label [num], instance_size int32 [num]) of query.segment_instances on a given table"""
    lab = np.asarray(labels, np.int64)
    lab = np.where((lab < 0) | np.isin(lab, np.asarray(list(ignore), np.int64)), -1, lab)
    max_d2 = None if max_dist is None else np.float32(max_dist) * np.float32(max_dist)
    comp, count, sizes, first = components(idx, d2, max_d2, lab)
    C = int(count[0])
    keep = np.append(sizes[:C] >= min_size, False)                         # one spare entry: an empty table indexes it
    new_id = np.cumsum(keep) - 1
    at = np.where(comp >= 0, comp, C)
    instance = np.where(keep[at], new_id[at], -1).astype(np.int32)
    return instance, int(keep.sum()), lab[first[:C][keep[:C]]], sizes[:C][keep[:C]]


def component_filter(idx, d2, group=None, num_groups=1, max_dist=None, min_share=None):
    """keep-mask bool [n] of query.component_filter on a given table"""
    n = len(idx)
    g = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64)
    g = np.where((g < 0) | (g >= num_groups), -1, g)
    max_d2 = None if max_dist is None else np.float32(max_dist) * np.float32(max_dist)
    comp, count, sizes, first = components(idx, d2, max_d2, g)
    C = int(count[0])
    keep_comp = np.zeros(max(C, 1), bool)
    cgroup = g[first[:C]]
    for grp in range(num_groups):
        cs = np.nonzero(cgroup == grp)[0]
        if len(cs) == 0:
            continue
        if min_share is None:
            keep_comp[cs[np.argmax(sizes[cs])]] = True                     # argmax: the first of equal sizes
        else:
            keep_comp[cs[sizes[cs].astype(np.float64) >= float(min_share) * float(sizes[cs].sum())]] = True
    return (comp >= 0) & keep_comp[np.maximum(comp, 0)]


def flood_fill(idx, d2=None, max_d2=None, labels=None):
    """The same four arrays by brute force: a symmetric adjacency matrix and a fill from every unvisited active row in order"""
    idx = np.asarray(idx, np.int64)
    n = idx.shape[0]
    active = np.ones(n, bool) if labels is None else np.asarray(labels, np.int64) >= 0
    adj = np.zeros((n, n), bool)
    rows, cols = np.nonzero(edge_mask(idx, d2, max_d2, labels))
    adj[rows, idx[rows, cols]] = True
    adj |= adj.T
    comp = np.full(n, -1, np.int32)
    sizes, first = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    C = 0
    for s in range(n):
        if not active[s] or comp[s] >= 0:
            continue
        comp[s] = C
        stack, members = [s], 1
        while stack:
            for v in np.nonzero(adj[stack.pop()])[0]:
                if comp[v] < 0:
                    comp[v] = C
                    members += 1
                    stack.append(int(v))
        sizes[C], first[C] = members, s
        C += 1
    return comp, np.array([C], np.int32), sizes, first


def canonical(comp):
    """a partition's labels renumbered by first occurrence (-1 stays): equal arrays mean equal partitions"""
    comp = np.asarray(comp)
    out = np.full(len(comp), -1, np.int64)
    seen = {}
    for i, c in enumerate(comp.tolist()):
        if c >= 0:
            out[i] = seen.setdefault(c, len(seen))
    return out
