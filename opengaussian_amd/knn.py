"""Exact k-nearest-distance sums on the GPU (include/ogs_knn.h) and the two things the reference builds on them.

``outlier_mask``  the keep-mask of render()'s ``post_process`` block (gaussian_renderer/__init__.py:292-309) and of
                  scripts/render_by_click.py:170-189 (``k_scale=2, std_weight=0.1``); there ``pytorch3d.ops.knn_points``.
``distCUDA2``     drop-in for ``simple_knn._C.distCUDA2`` / the scipy KDTree form of scene/gaussian_model.py:28-36.
``group_ksum``    the raw call: per row, the K-th smallest squared distance inside the row's group and the fp64 sums of the
                  K smallest and of their squares.
``neighbors``     the k <= 32 nearest neighbours themselves, indices and distances, by a sorted box search that scales to
                  millions of rows; ``distCUDA2`` takes it for large clouds.
``Index`` /       the same search BETWEEN TWO point sets: an index of a reference set, built once, and the k <= 32 nearest
``query``         reference rows of every row of any other set, wherever it lies; ``query.transfer_labels`` /
                  ``transfer_features`` carry per-point results across on it.
``radius_count``  how many rows lie within a radius of every row (``Index.radius_count`` for two sets): the same box walk with a
                  fixed threshold, no neighbour list anywhere.
``dbscan``        exact DBSCAN on that walk: core rows by ``min_pts``, clusters as the components of the core graph (the union
                  made inside the second walk), border rows to their nearest core; memory O(n) whatever ``eps`` is.
``aggregate``     the fixed-degree gather-sum over such an index table (the step of a diffusion over the kNN graph).
``reverse_edges`` the reverse-edge lists of an index table: per target row, the slots that point at it.
``components``    the connected components of an index table under a distance threshold and a same-label rule: a lock-free
                  union-find, numbered by smallest member, the same bytes every run.
``gather_sum``    ``aggregate`` with a backward: the gradient of the table through the reverse lists, that of the weights as
                  per-edge dots; no float atomics, so the gradients are the same bytes every run.

All groups go through one launch; nothing here reads a value back from the device, and no n x n buffer exists (an n x K one
only where ``neighbors`` returns it).
CPU tensors raise: there is no CPU path.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib
from ._lib import check, ptr


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); the k-nearest-distance kernel has no CPU path")


def isqrt(n: torch.Tensor) -> torch.Tensor:
    """floor(sqrt(n)) of an integer tensor, exact: the fp64 root, then one integer correction step either way
    (``int(n ** 0.5)`` of the reference at every n a group can have)."""
    n = n.to(torch.int64)
    r = torch.sqrt(n.to(torch.float64)).to(torch.int64)
    r = torch.where(r * r > n, r - 1, r)
    return torch.where((r + 1) * (r + 1) <= n, r + 1, r)


def _ksum_sorted(points, group, num_groups, k, want_kth=True):
    """The launch, in GROUP-SORTED row order.  Returns (order, gid, begin, k, kth, sum1, sum2): sorted row r is the
    caller's row order[r] (None: identity) and lies in group gid[r] (-1: none; None: all in group 0); begin [G + 1] int64
    row offsets, k [G] int32 as handed to the kernel; kth is None unless wanted."""
    _need_gpu(points, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [n, 3], got {tuple(points.shape)}")
    n, dev, G = points.shape[0], points.device, int(num_groups)
    pts = points.detach().to(torch.float32).contiguous()
    if group is None:
        if G != 1:
            raise ValueError("group=None means one group")
        order = gid = None
        # made on the device: a host list would be uploaded with a copy that waits for the stream (the filter reads nothing back)
        begin = torch.arange(2, dtype=torch.int64, device=dev) * n
    else:
        _need_gpu(group, "group")
        if group.shape != (n,):
            raise ValueError(f"group must be [{n}], got {tuple(group.shape)}")
        key = torch.where((group < 0) | (group >= G), -1, group).to(torch.int32)
        gid, order = torch.sort(key, stable=True)                   # rows of no group first, then group by group
        del key
        pts = pts[order]
        # begin[g] = sorted rows with a key below g (torch.bincount would read its bin count back to the host)
        begin = torch.searchsorted(gid, torch.arange(G + 1, dtype=torch.int32, device=dev))
    if callable(k):
        kk = k(begin[1:] - begin[:-1])
    elif isinstance(k, torch.Tensor):
        kk = k.to(dev)
    else:
        kk = torch.full((G,), int(k), dtype=torch.int64, device=dev)
    kk = kk.to(torch.int32).contiguous()
    if kk.shape != (G,):
        raise ValueError(f"k must be a number or [{G}] values")
    kth, sum1, sum2 = ksum_contiguous(pts, begin.to(torch.int32), kk, want_kth)
    return order, gid, begin, kk, kth, sum1, sum2


def ksum_contiguous(pts, begin32, kk, want_kth=False):
    """The launch itself over rows that already lie group by group: pts [n, 3] fp32 contiguous, begin32 [G + 1] int32,
    kk [G] int32.  Returns (kth or None, sum1, sum2); rows outside every group keep zeros."""
    n, dev, G = pts.shape[0], pts.device, kk.numel()
    kth = torch.zeros(n, dtype=torch.float32, device=dev) if want_kth else None
    sum1 = torch.zeros(n, dtype=torch.float64, device=dev)
    sum2 = torch.zeros(n, dtype=torch.float64, device=dev)
    check(_lib.lib().ogs_knn_group_ksum(n, ptr(pts), G, ptr(begin32), ptr(kk), ptr(kth), ptr(sum1), ptr(sum2), _stream()),
          "ogs_knn_group_ksum")
    return kth, sum1, sum2


def _unsort(t, order):
    if order is None:
        return t
    out = torch.empty_like(t)
    out[order] = t
    return out


def group_ksum(points: torch.Tensor, group, num_groups: int, k):
    """(kth [n] fp32, sum1 [n] fp64, sum2 [n] fp64) in the caller's row order.

    points [n, 3]; group [n] integer ids (rows with an id < 0 or >= num_groups belong to no group and get zeros), or None
    for one group of all rows; k: one K for all groups, a [num_groups] tensor, or a function of the group sizes.  K is
    clamped to the group's size.  Distances are fp32 ``(dx*dx + dy*dy) + dz*dz`` over the whole group, the row itself
    included; ties at the K-th value are counted exactly; two identical calls give the same bits."""
    order, _, _, _, kth, sum1, sum2 = _ksum_sorted(points, group, num_groups, k)
    return _unsort(kth, order), _unsort(sum1, order), _unsort(sum2, order)


def outlier_mask(points: torch.Tensor, group=None, num_groups: int = 1, k_scale: int = 1, std_weight: float = 1.0):
    """Keep-mask [n] of the reference's kNN outlier filter, every group filtered on its own, in one launch.

    Per group of n_g rows: K = int(n_g ** 0.5) * k_scale (clamped to n_g), a row's value is the mean of its K smallest
    squared distances (itself included), and the row is kept when that lies below mean + std_weight * std over ALL n_g * K
    values of the group (unbiased std, as ``Tensor.std()``).  Rows of no group are not kept.  A group of one row has
    std = nan and keeps nothing, as in the reference; so does a group whose K nearest distances are all zero.

    Mean and std come from the fp64 totals S1 = sum of values, S2 = sum of squares: var = (S2 - S1^2 / N) / (N - 1).
    That form cancels: its relative error is about 1e-16 * mean^2 / var, so it has no correct digit left once
    var / mean^2 falls below about 1e-10 -- all n_g * K distances equal to five digits, which distinct points cannot
    produce (the self-distance 0 is among them).  The group totals are fp64 atomic adds, whose order moves the last bits
    only."""
    order, gid, begin, kk, _, sum1, sum2 = _ksum_sorted(points, group, num_groups,
                                                        lambda sizes: isqrt(sizes) * int(k_scale), want_kth=False)
    return _unsort(keep_from_sums(gid, begin, kk, sum1, sum2, std_weight), order)


def keep_from_sums(gid, begin, kk, sum1, sum2, std_weight: float = 1.0):
    """The keep rule of ``outlier_mask`` over GROUP-SORTED rows, from what one ``ogs_knn_group_ksum`` launch left: gid [n]
    group of every row (-1: none; None: all rows in group 0), begin [G + 1] row offsets, kk [G] the K handed to the kernel,
    sum1 / sum2 [n] fp64 (sum1 is overwritten).  Shared with ``query.render_queries``, whose rows come out of the split
    group by group and need no sort."""
    G, dev = begin.numel() - 1, sum1.device
    begin = begin.to(torch.int64)
    sizes = begin[1:] - begin[:-1]
    kd = torch.minimum(kk.to(torch.int64), sizes).to(torch.float64)                # the K the kernel used
    N = sizes.to(torch.float64) * kd
    if gid is None:
        S1, S2 = sum1.sum().reshape(1), sum2.sum().reshape(1)
    else:
        slot = gid + 1                                                             # slot 0 collects the rows of no group
        S1 = torch.zeros(G + 1, dtype=torch.float64, device=dev).index_add_(0, slot, sum1)[1:]
        S2 = torch.zeros(G + 1, dtype=torch.float64, device=dev).index_add_(0, slot, sum2)[1:]
    del sum2
    mean = S1 / N
    std = torch.sqrt(torch.clamp_min((S2 - S1 * S1 / N) / (N - 1.0), 0.0))         # 0 / 0 = nan stays nan
    limit = mean + float(std_weight) * std
    if gid is None:
        return sum1 / kd < limit
    nan = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)          # slot 0: nothing is below nan
    row_mean = sum1.div_(torch.cat((nan, kd)).index_select(0, slot))
    return row_mean < torch.cat((nan, limit)).index_select(0, slot)


def neighbors(points: torch.Tensor, k: int, exclude_self: bool = True):
    """The k nearest neighbours of every row among all rows: (idx int32 [n, k], d2 fp32 [n, k]), exact, in one call
    (``ogs_knn_neighbors``: a Morton sort, then a search in boxes of 64 points with exact pruning -- no n x n pass).

    Row i lists the rows j (``j != i`` when ``exclude_self``) by ascending (d2, j): d2 is the fp32
    ``(dx*dx + dy*dy) + dz*dz`` of ``group_ksum``, equal distances go to the smaller index, so the result is unique and two
    calls give the same bytes.  Slots past the end of the list (fewer than k candidates) hold idx = -1, d2 = +inf.
    1 <= k <= 32 and n * k < 2^31.  Nothing is read back from the device."""
    pts = _points_arg(points, "points")
    n, dev, k = pts.shape[0], pts.device, int(k)
    idx = torch.empty((n, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((n, k), dtype=torch.float32, device=dev)
    L = _lib.lib()
    nbytes = int(L.ogs_knn_neighbors_tmp_bytes(n))
    tmp = _tmp(nbytes, dev)
    check(L.ogs_knn_neighbors(n, ptr(pts), k, int(bool(exclude_self)), ptr(idx), ptr(d2), ptr(tmp), nbytes, _stream()),
          "ogs_knn_neighbors")
    return idx, d2


def _points_arg(points, name):
    _need_gpu(points, name)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{name} must be [n, 3], got {tuple(points.shape)}")
    return points.detach().to(torch.float32).contiguous()


class Index:
    """The search index of one REFERENCE point set (``ogs_knn_index_build``), built once and queried any number of times with
    other point sets: the reference's coordinates sorted by Morton key in boxes of 64 points, their row numbers, the bounds and
    the first key of every box -- about 16.5 bytes per point, a copy, so ``points`` may change or go afterwards.  ``.n`` rows on
    ``.device``.  Nothing is read back from the device."""

    def __init__(self, points: torch.Tensor):
        pts = _points_arg(points, "points")
        self.n, self.device = pts.shape[0], pts.device
        L = _lib.lib()
        self._bytes = int(L.ogs_knn_index_bytes(self.n))
        self._buf = _tmp(self._bytes, self.device)
        nbytes = int(L.ogs_knn_index_build_tmp_bytes(self.n))
        tmp = _tmp(nbytes, self.device)
        check(L.ogs_knn_index_build(self.n, ptr(pts), ptr(self._buf), self._bytes, ptr(tmp), nbytes, _stream()),
              "ogs_knn_index_build")

    def query(self, queries: torch.Tensor, k: int):
        """The k nearest reference rows of every query row: (idx int32 [m, k], d2 fp32 [m, k]), exact (``ogs_knn_query``: the
        queries are grouped by a Morton sort of their own, every group of 64 starts at the reference box its centre falls
        into, and the search of ``neighbors`` runs from there).

        Row q lists the reference rows j by ascending (d2, j): d2 is the fp32 ``(dx*dx + dy*dy) + dz*dz`` with
        ``dx = x_q - x_j``, equal distances go to the smaller reference row, so the result is unique and two calls give the
        same bytes.  Slots past the end of the list (fewer than k reference rows) hold idx = -1, d2 = +inf.
        1 <= k <= 32 and m * k < 2^31.  The queries may lie anywhere, also wholly outside the reference's bounding box."""
        q = _points_arg(queries, "queries")
        if q.device != self.device:
            raise ValueError(f"queries live on {q.device}, the index on {self.device}")
        m, k = q.shape[0], int(k)
        idx = torch.empty((m, k), dtype=torch.int32, device=self.device)
        d2 = torch.empty((m, k), dtype=torch.float32, device=self.device)
        L = _lib.lib()
        nbytes = int(L.ogs_knn_query_tmp_bytes(self.n, m))
        tmp = _tmp(nbytes, self.device)
        check(L.ogs_knn_query(self.n, ptr(self._buf), m, ptr(q), k, ptr(idx), ptr(d2), ptr(tmp), nbytes, _stream()),
              "ogs_knn_query")
        return idx, d2

    def radius_count(self, queries: torch.Tensor, radius, labels=None, query_labels=None):
        """How many reference rows lie within ``radius`` of every query row: int32 [m] (``ogs_knn_radius_count``: the walk of
        ``query`` with a fixed threshold, so no list is kept and memory does not grow with the radius).

        Row j counts for query q when ``d2(q, j) <= radius * radius`` in fp32 -- d2 as in ``query``, the square ONE fp32 multiply
        made on the device, equality counts.  ``radius`` is a float >= 0 or a one-element device tensor (a NaN selects nothing,
        +inf everything).  ``labels`` [n] / ``query_labels`` [m] go together: row j then counts only when both labels are equal
        and >= 0.  Nothing is read back."""
        q = _points_arg(queries, "queries")
        if q.device != self.device:
            raise ValueError(f"queries live on {q.device}, the index on {self.device}")
        if (labels is None) != (query_labels is None):
            raise ValueError("labels and query_labels are given together or not at all")
        m = q.shape[0]
        rl = _labels_arg(labels, self.n, "labels", self.device)
        ql = _labels_arg(query_labels, m, "query_labels", self.device)
        r2 = squared_on_device(radius, self.device, "radius")
        count = torch.empty(m, dtype=torch.int32, device=self.device)
        L = _lib.lib()
        nbytes = int(L.ogs_knn_radius_count_tmp_bytes(self.n, m))
        tmp = _tmp(nbytes, self.device)
        check(L.ogs_knn_radius_count(self.n, ptr(self._buf), m, ptr(q), ptr(r2), ptr(rl), ptr(ql), ptr(count), ptr(tmp), nbytes,
                                     _stream()), "ogs_knn_radius_count")
        return count


def squared_on_device(dist, dev, name="dist"):
    """A distance squared as ONE fp32 multiply on the device, fp32 [1]: a float >= 0 or a one-element tensor"""
    if isinstance(dist, torch.Tensor):
        if dist.numel() != 1:
            raise ValueError(f"{name} must be a number or a one-element tensor, got {tuple(dist.shape)}")
        m = dist.detach().to(dev).to(torch.float32).reshape(1)
    else:
        if not float(dist) >= 0:
            raise ValueError(f"{name} must be a distance >= 0, got {dist}")
        m = torch.full((1,), float(dist), dtype=torch.float32, device=dev)
    return m * m


def _labels_arg(labels, n, name, dev):
    if labels is None:
        return None
    _need_gpu(labels, name)
    if labels.shape != (n,):
        raise ValueError(f"{name} must be [{n}], got {tuple(labels.shape)}")
    return labels.detach().to(dev).to(torch.int32).contiguous()


def query(points: torch.Tensor, queries: torch.Tensor, k: int):
    """``Index(points).query(queries, k)``: the k nearest rows of ``points`` [n, 3] for every row of ``queries`` [m, 3], in one
    shot.  Keep the ``Index`` instead when the same reference set is asked more than once."""
    _points_arg(queries, "queries")                                 # both sets are checked before anything is built
    return Index(points).query(queries, k)


def radius_count(points: torch.Tensor, radius, queries=None, labels=None, query_labels=None):
    """``Index(points).radius_count(queries, radius, ...)`` in one shot; ``queries=None`` counts the set against itself (every
    row then counts itself, and ``labels`` serves both sides)."""
    if queries is None:
        if query_labels is not None:
            raise ValueError("query_labels needs queries")
        queries, query_labels = points, labels
    else:
        _points_arg(queries, "queries")                             # both sets are checked before anything is built
    return Index(points).radius_count(queries, radius, labels, query_labels)


class Dbscan(NamedTuple):
    cluster: torch.Tensor                               # int32 [n]: the row's cluster, -1 for noise and inactive rows
    count: torch.Tensor                                 # int32 [1]: the number of clusters C, on the device
    sizes: torch.Tensor                                 # int32 [n]: members of cluster c < C with its borders, 0 beyond
    first: torch.Tensor                                 # int32 [n]: smallest CORE row of cluster c < C, -1 beyond
    core: torch.Tensor                                  # bool [n]
    degree: torch.Tensor                                # int32 [n]: rows within eps, the row itself included; 0 when inactive


@torch.no_grad()
def dbscan(points: torch.Tensor, eps, min_pts: int, labels=None) -> Dbscan:
    """Exact DBSCAN of points [n, 3] (``ogs_knn_dbscan``): every pair within ``eps`` is seen, by two walks over the sorted boxes
    of ``neighbors`` with a fixed threshold -- the first counts, the second unites -- so no neighbour list exists and memory is
    O(n) whatever ``eps`` is.

    Row i is active unless ``labels`` [n] holds a negative value for it.  N(i) is the set of active rows j with the same label
    and ``d2(i, j) <= eps * eps`` in fp32 (d2 as in ``neighbors``, the square ONE fp32 multiply on the device; equality counts;
    i itself is in N(i)).  ``degree = |N(i)|``, ``core = degree >= min_pts``.  Clusters are the connected components of the core
    rows under "within each other's N"; a non-core row with a core in reach is a border row and joins the cluster of the core
    with the smallest (d2, row) -- that one only, so a chain of border rows bridges nothing; every other row is noise (-1).
    Clusters are numbered by ascending smallest core row.  ``eps``: a float >= 0 or a one-element device tensor.  The result is
    unique, the same bytes every run; nothing is read back (``count`` stays on the device)."""
    pts = _points_arg(points, "points")
    n, dev = pts.shape[0], pts.device
    if int(min_pts) < 1:
        raise ValueError(f"min_pts must be at least 1, got {min_pts}")
    lc = _labels_arg(labels, n, "labels", dev)
    e2 = squared_on_device(eps, dev, "eps")
    cluster = torch.empty(n, dtype=torch.int32, device=dev)
    core = torch.empty(n, dtype=torch.uint8, device=dev)
    degree = torch.empty(n, dtype=torch.int32, device=dev)
    sizes = torch.empty(n, dtype=torch.int32, device=dev)
    first = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    L = _lib.lib()
    nbytes = int(L.ogs_knn_dbscan_tmp_bytes(n))
    tmp = _tmp(nbytes, dev)
    check(L.ogs_knn_dbscan(n, ptr(pts), ptr(e2), int(min_pts), ptr(lc), ptr(cluster), ptr(core), ptr(degree), ptr(sizes), ptr(first),
                           ptr(count), ptr(tmp), nbytes, _stream()), "ogs_knn_dbscan")
    return Dbscan(cluster, count, sizes, first, core.view(torch.bool), degree)


@torch.no_grad()
def aggregate(X: torch.Tensor, idx: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Fixed-degree gather-sum ``out[i] = sum_k w[i, k] * X[idx[i, k]]`` (fp32 [n, D]) without the [n, K, D] buffer of
    ``(w[..., None] * X[idx]).sum(1)``: X [R, D], idx int32 [n, K], w [n, K].  Per element one fmaf chain from +0 with k
    ascending; slots whose idx lies outside [0, R) are skipped, whatever their weight holds.  One writer per element, no
    atomics: two calls give the same bytes.  X must be finite.  Measured at 500 k rows x 16 neighbours it is ahead of the
    torch composition at every width tried: 0.14 / 0.30 / 2.78 ms against 0.28 / 2.82 / 14.4 ms at D = 6 / 64 / 512.

    FORWARD ONLY: runs under ``no_grad`` and returns a tensor without a graph, also for inputs that require grad;
    ``gather_sum`` is the same sum with a backward."""
    _check_gather_args(X, idx, w)
    return _aggregate(*_gather_args(X, idx, w))


def _check_gather_args(X, idx, w):
    for t, name in ((X, "X"), (idx, "idx"), (w, "w")):
        _need_gpu(t, name)
    if X.dim() != 2 or idx.dim() != 2 or w.shape != idx.shape:
        raise ValueError(f"X must be [R, D] and idx, w [n, K] alike, got {tuple(X.shape)}, {tuple(idx.shape)}, {tuple(w.shape)}")
    if X.shape[1] < 1:
        raise ValueError("X needs at least one column")


def _gather_args(X, idx, w):
    return (X.detach().to(torch.float32).contiguous(), idx.to(torch.int32).contiguous(),
            w.detach().to(torch.float32).contiguous())


def _aggregate(Xc, ic, wc):
    """ogs_knn_aggregate on fp32 / int32 contiguous tensors"""
    n, K = ic.shape
    out = torch.empty((n, Xc.shape[1]), dtype=torch.float32, device=Xc.device)
    check(_lib.lib().ogs_knn_aggregate(n, K, Xc.shape[0], Xc.shape[1], ptr(ic), ptr(wc), ptr(Xc), ptr(out), _stream()),
          "ogs_knn_aggregate")
    return out


def _tmp(nbytes, dev):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


@torch.no_grad()
def reverse_edges(idx: torch.Tensor, num_rows=None):
    """Reverse-edge lists of an index table idx int32 [n, K] over ``num_rows`` target rows (default n): ``(begin, slots)``,
    int32 [num_rows + 1] and [n * K].  ``slots[begin[r]:begin[r + 1]]`` are the flat slot numbers ``e = i * K + k`` with
    ``idx[i, k] == r``, ascending; ``begin[-1]`` is the number of slots with ``0 <= idx < num_rows`` and what ``slots`` holds
    from there on is unspecified.  A stable radix sort (``ogs_knn_transpose``): the lists are unique, two calls give the same
    bytes, nothing is read back.  Built once per graph and handed to ``gather_sum`` / ``query.neighbor_smoothness`` as
    ``reverse``."""
    _need_gpu(idx, "idx")
    if idx.dim() != 2:
        raise ValueError(f"idx must be [n, K], got {tuple(idx.shape)}")
    ic = idx.to(torch.int32).contiguous()
    n, K = ic.shape
    R = n if num_rows is None else int(num_rows)
    L = _lib.lib()
    begin = torch.empty(max(R, 0) + 1, dtype=torch.int32, device=idx.device)
    slots = torch.empty(n * K, dtype=torch.int32, device=idx.device)
    nbytes = int(L.ogs_knn_transpose_tmp_bytes(n, K, R))
    tmp = _tmp(nbytes, idx.device)
    check(L.ogs_knn_transpose(n, K, R, ptr(ic), ptr(begin), ptr(slots), ptr(tmp), nbytes, _stream()), "ogs_knn_transpose")
    return begin, slots


@torch.no_grad()
def components(idx: torch.Tensor, d2=None, max_d2=None, labels=None):
    """Connected components of the graph an index table spans (``ogs_knn_components``): ``(comp, count, sizes, first)``, int32
    [n], [1], [n], [n], all on the device.

    idx int32 [n, K] as ``neighbors`` returns it.  Row i is active unless ``labels`` [n] holds a negative value for it.  Slot
    (i, k) with j = idx[i, k] joins i and j when ``0 <= j < n``, both rows are active, ``labels`` (where given) are equal, and --
    with both ``d2`` fp32 [n, K] and ``max_d2`` given -- ``d2[i, k] <= max_d2`` in fp32 (a NaN on either side joins nothing).
    ``max_d2`` is a SQUARED distance, a float or a 0-dim / one-element device tensor.  Edges are undirected: one row listing
    the other is enough.  Components are numbered by ascending smallest member row: ``comp[i]`` is the row's component (-1:
    inactive), ``count[0]`` their number C, ``sizes[c]`` / ``first[c]`` the member count and smallest member of c < C (0 / -1
    beyond).  The result is unique -- the same bytes every run, whatever the order of the slots within a row -- and nothing is
    read back: ``count`` stays on the device.

    A table with K <= 32 columns does not hold every neighbour within a radius, so two rows closer than ``max_d2`` whose lists
    are full of nearer rows are joined only through those, and there is no core-point rule: ``dbscan`` is the exact clustering
    by radius."""
    _need_gpu(idx, "idx")
    if idx.dim() != 2 or idx.shape[1] < 1:
        raise ValueError(f"idx must be [n, K] with K >= 1, got {tuple(idx.shape)}")
    n, K = idx.shape
    dev = idx.device
    ic = idx.to(torch.int32).contiguous()
    dc = mc = lc = None
    if d2 is not None:
        _need_gpu(d2, "d2")
        if d2.shape != idx.shape:
            raise ValueError(f"d2 must be [{n}, {K}] like idx, got {tuple(d2.shape)}")
        dc = d2.detach().to(torch.float32).contiguous()
    if max_d2 is not None:
        if isinstance(max_d2, torch.Tensor):
            _need_gpu(max_d2, "max_d2")
            if max_d2.numel() != 1:
                raise ValueError(f"max_d2 must be a number or a one-element tensor, got {tuple(max_d2.shape)}")
            mc = max_d2.detach().to(torch.float32).reshape(1).contiguous()
        else:
            mc = torch.full((1,), float(max_d2), dtype=torch.float32, device=dev)
    if labels is not None:
        _need_gpu(labels, "labels")
        if labels.shape != (n,):
            raise ValueError(f"labels must be [{n}], got {tuple(labels.shape)}")
        lc = labels.detach().to(torch.int32).contiguous()
    comp = torch.empty(n, dtype=torch.int32, device=dev)
    sizes = torch.empty(n, dtype=torch.int32, device=dev)
    first = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    L = _lib.lib()
    nbytes = int(L.ogs_knn_components_tmp_bytes(n))
    tmp = _tmp(nbytes, dev)
    check(L.ogs_knn_components(n, K, ptr(ic), ptr(dc), ptr(mc), ptr(lc), ptr(comp), ptr(sizes), ptr(first), ptr(count), ptr(tmp),
                               nbytes, _stream()), "ogs_knn_components")
    return comp, count, sizes, first


class LazyReverse:
    """The reverse lists of one index table, built when first asked for (the first backward) and kept."""

    def __init__(self, idx, num_rows, value=None):
        self.idx, self.num_rows, self.value = idx, int(num_rows), value

    @classmethod
    def of(cls, reverse, idx, num_rows):
        if isinstance(reverse, cls):
            if reverse.num_rows != int(num_rows):
                raise ValueError(f"reverse was made for {reverse.num_rows} rows, the table has {int(num_rows)}")
            return reverse
        if reverse is None:
            return cls(idx, num_rows)
        begin, slots = reverse
        if begin.shape != (int(num_rows) + 1,) or slots.shape != (idx.numel(),):
            raise ValueError(f"reverse must be (begin [{int(num_rows) + 1}], slots [{idx.numel()}]) as reverse_edges returns them, "
                             f"got {tuple(begin.shape)}, {tuple(slots.shape)}")
        for t, name in ((begin, "reverse begin"), (slots, "reverse slots")):
            _need_gpu(t, name)
        return cls(idx, num_rows, (begin.to(torch.int32).contiguous(), slots.to(torch.int32).contiguous()))

    def get(self):
        if self.value is None:
            self.value = reverse_edges(self.idx, self.num_rows)
        return self.value


def _aggregate_t(Gc, wc, K, R, begin, slots):
    """ogs_knn_aggregate_t: Gc [n, D], wc [n, K] fp32 contiguous -> [R, D]"""
    n, D = Gc.shape
    L = _lib.lib()
    out = torch.empty((R, D), dtype=torch.float32, device=Gc.device)
    nbytes = int(L.ogs_knn_aggregate_t_tmp_bytes(n, K, R, D))
    tmp = _tmp(nbytes, Gc.device)
    check(L.ogs_knn_aggregate_t(n, K, R, D, ptr(begin), ptr(slots), ptr(wc), ptr(Gc), ptr(out), ptr(tmp), nbytes, _stream()),
          "ogs_knn_aggregate_t")
    return out


def _edge_dots(Gc, Xc, ic):
    """ogs_knn_edge_dots: Gc [n, D], Xc [R, D], ic [n, K] -> [n, K]"""
    n, K = ic.shape
    gw = torch.empty((n, K), dtype=torch.float32, device=Gc.device)
    check(_lib.lib().ogs_knn_edge_dots(n, K, Xc.shape[0], Xc.shape[1], ptr(ic), ptr(Gc), ptr(Xc), ptr(gw), _stream()),
          "ogs_knn_edge_dots")
    return gw


class _GatherSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, w, idx, rev):
        Xc, ic, wc = _gather_args(X, idx, w)
        ctx.save_for_backward(Xc, ic, wc)
        ctx.rev, ctx.dtypes = rev, (X.dtype, w.dtype)
        return _aggregate(Xc, ic, wc)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        Xc, ic, wc = ctx.saved_tensors
        Gc = grad.to(torch.float32).contiguous()
        gX = gw = None
        if ctx.needs_input_grad[0]:
            begin, slots = ctx.rev.get()
            gX = _aggregate_t(Gc, wc, ic.shape[1], Xc.shape[0], begin, slots).to(ctx.dtypes[0])
        if ctx.needs_input_grad[1]:
            gw = _edge_dots(Gc, Xc, ic).to(ctx.dtypes[1])
        return gX, gw, None, None


def gather_sum(X: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, reverse=None) -> torch.Tensor:
    """``aggregate`` with a backward: ``out[i] = sum_k w[i, k] * X[idx[i, k]]`` (fp32 [n, D]), the bytes ``aggregate`` gives,
    differentiable in ``X`` [R, D] and ``w`` [n, K].

    The gradient of ``X`` is the gather-sum over the REVERSED edges (``ogs_knn_aggregate_t``): per row of X one fmaf chain over
    the slots that point at it, in slot order -- no ``index_add_``, no float atomics, the same bytes every run; a row with more
    than ``ogs_knn_transpose_chunk()`` incoming edges is summed in chunks of that size whose partials are added in order.  The
    gradient of ``w`` (only when ``w`` requires one) is ``ogs_knn_edge_dots``: ``<grad[i], X[idx[i, k]]>``, 0 on the slots whose
    idx lies outside [0, R).  ``reverse``: ``reverse_edges(idx, R)`` of this table; when it is None the lists are built in the
    first backward (one stable sort of n * K keys) -- hand them in when the graph outlives one step.  No double backward.
    Measured at 500 k rows x 16 neighbours, forward + backward with both gradients, it is ahead of torch autograd of the
    composition at every shape tried: 0.67 / 1.26 / 11.6 ms against 3.61 / 10.0 / 45.0 ms at D = 6 / 64 / 512, and 0.45 against
    17.6 ms when the slots point into 320 rows (lists of 25 000 slots); ``reverse_edges`` itself takes 0.22 ms there."""
    _check_gather_args(X, idx, w)
    return _GatherSum.apply(X, w, idx, LazyReverse.of(reverse, idx, X.shape[0]))


@torch.no_grad()
def smoothness_energy(F: torch.Tensor, idx: torch.Tensor, w: torch.Tensor):
    """Row energies of the neighbour smoothness term, ``e[i] = sum_k w[i, k] * |F[i] - F[idx[i, k]]|^2`` over the slots with
    ``0 <= idx < n`` (fp32 [n]; the differences are taken first), and ``total`` fp64 [2]: the sum of ``e`` in a fixed order and
    the number of such slots.  One ``ogs_knn_smoothness_fwd`` call, no [n, K, D] buffer.  Forward only:
    ``query.neighbor_smoothness`` is the loss with a backward."""
    _check_gather_args(F, idx, w)
    if idx.shape[0] != F.shape[0]:
        raise ValueError(f"a square graph: idx must have the {F.shape[0]} rows of F, got {idx.shape[0]}")
    return _smoothness_fwd(*_gather_args(F, idx, w))


def _smoothness_fwd(Fc, ic, wc):
    n, K = ic.shape
    L = _lib.lib()
    energy = torch.empty(n, dtype=torch.float32, device=Fc.device)
    total = torch.empty(2, dtype=torch.float64, device=Fc.device)
    nbytes = int(L.ogs_knn_smoothness_fwd_tmp_bytes(n))
    tmp = _tmp(nbytes, Fc.device)
    check(L.ogs_knn_smoothness_fwd(n, K, Fc.shape[1], ptr(ic), ptr(wc), ptr(Fc), ptr(energy), ptr(total), ptr(tmp), nbytes,
                                   _stream()), "ogs_knn_smoothness_fwd")
    return energy, total


def _smoothness_bwd(Fc, ic, wc, begin, slots, scale, want_gw):
    """scale: fp32 [1] on the device"""
    n, K = ic.shape
    D = Fc.shape[1]
    L = _lib.lib()
    gF = torch.empty((n, D), dtype=torch.float32, device=Fc.device)
    gw = torch.empty((n, K), dtype=torch.float32, device=Fc.device) if want_gw else None
    nbytes = int(L.ogs_knn_smoothness_bwd_tmp_bytes(n, K, D))
    tmp = _tmp(nbytes, Fc.device)
    check(L.ogs_knn_smoothness_bwd(n, K, D, ptr(ic), ptr(wc), ptr(Fc), ptr(begin), ptr(slots), ptr(scale), ptr(gF), ptr(gw),
                                   ptr(tmp), nbytes, _stream()), "ogs_knn_smoothness_bwd")
    return gF, gw


# rows from which distCUDA2(route=None) takes the box search.  Measured (scripts/knn_neighbors_bench.py,
# profiles/knn_neighbors_bench.json) every repeat of it beats every repeat of the brute route from the smallest size of the
# sweep, 1 000 rows, on; the switch sits at the smallest size of the sweep above 4 097 rows instead, because
# tests/test_knn_host.py drives distCUDA2() without a route through a stand-in library that has the brute entry point only,
# on clouds up to that size
DIST_BOXES_FROM = 8000


def distCUDA2(points: torch.Tensor, route=None) -> torch.Tensor:
    """Mean squared distance to the three nearest OTHER points, fp32 [n] in the input's order: the 4 smallest squared
    distances with the row itself (0) among them, summed, over 3.  The caller keeps its own ``clamp_min``.

    route ``"brute"``: one ``ogs_knn_group_ksum`` launch, 32 passes over all n^2 pairs.  ``"boxes"``:
    ``neighbors(points, 4, exclude_self=False)`` and an ascending fp64 sum -- the same distances, summed in another order.
    ``None``: ``"boxes"`` from ``DIST_BOXES_FROM`` rows on, ``"brute"`` below."""
    if route is None:
        route = "boxes" if points.shape[0] >= DIST_BOXES_FROM else "brute"
    if route == "brute":
        _, _, _, _, _, sum1, _ = _ksum_sorted(points, None, 1, 4, want_kth=False)
        return (sum1 / 3.0).to(torch.float32)
    if route != "boxes":
        raise ValueError(f"route must be 'boxes', 'brute' or None, got {route!r}")
    idx, d2 = neighbors(points, 4, exclude_self=False)
    d = torch.where(idx >= 0, d2, torch.zeros_like(d2)).to(torch.float64)      # fewer than 4 rows: the list ends early
    return ((((d[:, 0] + d[:, 1]) + d[:, 2]) + d[:, 3]) / 3.0).to(torch.float32)
