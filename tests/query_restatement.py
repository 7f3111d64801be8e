"""NumPy restatements of the open-vocabulary query step (include/ogs_query.h), in fp64 unless the reference's own arithmetic
is fp32: what tests/test_query_host.py holds against goldens made by the reference's code and tests/test_38_query_gpu.py
holds the kernels against."""
import numpy as np


def normalize(x):
    """F.normalize(x, dim=1, p=2): x / max(|x|, 1e-12); a zero row stays zero"""
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


def similarity(text, leaf, occu=None, min_occu=5):
    """sim [Q, K] fp64; leaves with occu < min_occu are zero rows"""
    leaf = np.array(leaf, np.float64)
    if occu is not None:
        leaf[np.asarray(occu) < min_occu] = 0.0
    return normalize(text) @ normalize(leaf).T


def rank_desc(row, top):
    """indices of the min(top, K) highest values, descending, ties to the lowest index"""
    return np.argsort(-np.asarray(row), kind="stable")[:min(int(top), len(row))]


def select_row(sim_row, centers, leaf_num, top=10, max_dist=0.9):
    """(ids, decisive centre distances): best first, then the ranked candidates that pass both conditions of
    render_lerf_by_text.py:110-114 -- `candidate - best < leaf_num` signed, centre distance below max_dist"""
    rank = rank_desc(sim_row, top)
    best = int(rank[0])
    ids, dists = [best], []
    c = np.asarray(centers, np.float32)
    for cand in rank[1:]:
        if np.float32(int(cand) - best) < np.float32(leaf_num):
            d = float(np.linalg.norm((c[best] - c[int(cand)]).astype(np.float64)))
            dists.append(d)
            if d < max_dist:
                ids.append(int(cand))
    return ids, dists


def select_leaves(text, leaf, occu, centers, leaf_num, min_occu=5, top=10, max_dist=0.9):
    """(sim [Q, K] fp64, selected [Q, top] int32 padded with -1, count [Q] int32)"""
    sim = similarity(text, leaf, occu, min_occu)
    Q = sim.shape[0]
    selected = np.full((Q, int(top)), -1, np.int32)
    count = np.zeros(Q, np.int32)
    for q in range(Q):
        ids, _ = select_row(sim[q], centers, leaf_num, top, max_dist)
        selected[q, :len(ids)] = ids
        count[q] = len(ids)
    return sim, selected, count


def row_margins(sim, top):
    """per row of sim: (gap between the two highest, gap between rank top and rank top + 1; inf where there is no such rank)"""
    s = -np.sort(-np.asarray(sim, np.float64), axis=1)
    K = s.shape[1]
    first = s[:, 0] - s[:, 1] if K > 1 else np.full(len(s), np.inf)
    cut = s[:, top - 1] - s[:, top] if K > top else np.full(len(s), np.inf)
    return first, cut


def rank_margin(sim, top):
    """smallest gap between neighbouring ranks among the first min(top + 1, K) of every row: the ranked ORDER decides the order
    of the appended ids, so every one of these gaps has to be clear"""
    s = -np.sort(-np.asarray(sim, np.float64), axis=1)[:, :top + 1]
    return np.inf if s.shape[1] < 2 else float((s[:, :-1] - s[:, 1:]).min())


def merge_margin(sim, centers, leaf_num, top=10, max_dist=0.9):
    """smallest |distance - max_dist| over every centre distance that decides a merge (inf when none does)"""
    worst = np.inf
    for row in sim:
        _, dists = select_row(row, centers, leaf_num, top, max_dist)
        if dists:
            worst = min(worst, float(np.abs(np.asarray(dists) - max_dist).min()))
    return worst


def decided_rows(sim, zeroed, centers, leaf_num, top, margin, order_margin, max_dist=0.9):
    """bool [Q]: the rows of `sim` in which every decision of the selection is clear, so that fp32 similarities within the
    bar give the same `selected` / `count`.  Neighbouring ranks among the first min(top + 1, K) lie further apart than
    `margin` (rank 0 / 1, and rank top / top + 1: the cut) or `order_margin` (the ranks in between), OR both are similarities
    that are exactly 0 on either side -- a zeroed leaf (`zeroed` [K] bool), any leaf of an all-zero text row -- whose tie goes
    to the lowest index on either side.  Every centre distance that decides a merge lies further than `margin` from
    `max_dist`."""
    sim, zeroed = np.asarray(sim, np.float64), np.asarray(zeroed, bool)
    Q, K = sim.shape
    ok = np.ones(Q, bool)
    for q in range(Q):
        order = np.argsort(-sim[q], kind="stable")[:top + 1]
        exact0 = zeroed[order] | (not sim[q].any())
        gap = sim[q][order][:-1] - sim[q][order][1:]
        need = np.full(len(gap), order_margin)
        need[:1] = margin
        if K > top:
            need[top - 1] = margin
        ok[q] = bool(((gap > need) | (exact0[:-1] & exact0[1:] & (gap == 0))).all())
        ok[q] &= merge_margin(sim[q:q + 1], centers, leaf_num, top, max_dist) > margin
    return ok


def classify(text, leaf, occu, leaf_ind, min_occu=2):
    """(pred [N] int64, class_of_leaf [K], sim [T, K]) of eval_scannet.py:143-144,158-163"""
    sim = similarity(text, leaf, occu, min_occu)
    cls = np.argmax(sim, axis=0)                          # the first maximum: lowest class on ties
    K = sim.shape[1]
    return cls[np.clip(np.asarray(leaf_ind), 0, K - 1)].astype(np.int64) + 1, cls, sim


def confusion(gt, pred, C, ignore=None):
    """[C, C] int64 after gt[ignore] = 0 and pred[gt == 0] = 0"""
    gt, pred = np.array(gt, np.int64), np.array(pred, np.int64)
    if ignore is not None:
        gt[np.asarray(ignore, bool)] = 0
    pred[gt == 0] = 0
    return np.bincount(gt * C + pred, minlength=C * C).reshape(C, C).astype(np.int64)


def _mean32(v):
    """Tensor.mean() of fp32 values as the reference takes it (torch's own fp32 summation; nan for none)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).mean().item() if len(v) else float("nan")


def metrics(conf):
    """calculate_metrics from the table, fp32 where the reference holds fp32 tensors -> (ious fp32 [C], mIoU, acc, mAcc)"""
    conf = np.asarray(conf, np.int64)
    C = conf.shape[0]
    diag, row, col = np.diag(conf), conf.sum(1), conf.sum(0)
    inter, union, total = np.zeros(C, np.float32), np.zeros(C, np.float32), np.zeros(C, np.float32)
    inter[1:], union[1:], total[1:] = diag[1:], (row + col - diag)[1:], row[1:]
    ious = np.zeros(C, np.float32)
    ok = union != 0
    ious[ok] = inter[ok] / union[ok]
    present = np.nonzero(row[1:] > 0)[0] + 1
    nan = float("nan")
    mean_iou = _mean32(ious[present])
    valid = int(row[1:].sum())
    acc = int(diag[1:].sum()) / valid if valid > 0 else nan
    with np.errstate(invalid="ignore", divide="ignore"):
        class_acc = inter / total
    macc = _mean32(class_acc[present])
    return ious, mean_iou, acc, macc


def reference_loop_metrics(gt, pred, C):
    """The reference's own route -- 4 x (C - 1) full-length reductions -- restated one to one (the baseline of
    scripts/query_bench.py and the cross-check that the table route gives the same ious)."""
    gt, pred = np.array(gt, np.int64), np.array(pred, np.int64)
    pred[gt == 0] = 0
    inter, union, total = np.zeros(C, np.float32), np.zeros(C, np.float32), np.zeros(C, np.float32)
    for cls in range(1, C):
        inter[cls] = int(((gt == cls) & (pred == cls)).sum())
        union[cls] = int(((gt == cls) | (pred == cls)).sum())
        total[cls] = int((gt == cls).sum())
    ious = np.zeros(C, np.float32)
    ok = union != 0
    ious[ok] = inter[ok] / union[ok]
    present = np.unique(gt)
    present = present[present != 0]
    nan = float("nan")
    mean_iou = _mean32(ious[present])
    valid = gt != 0
    acc = int(((gt == pred) & valid).sum()) / int(valid.sum()) if valid.any() else nan
    with np.errstate(invalid="ignore", divide="ignore"):
        class_acc = inter / total
    macc = _mean32(class_acc[present])
    return ious, mean_iou, acc, macc


def membership(leaf_ind, words, Q, row_ok=None, group_keep=None):
    """member [N, Q] bool: bit q of words[leaf_ind[p]] & row_ok[p] & group_keep[q]; ids outside [0, K) are in no group"""
    leaf_ind, words = np.asarray(leaf_ind, np.int64), np.asarray(words, np.uint64)
    K = len(words)
    inside = (leaf_ind >= 0) & (leaf_ind < K)
    w = np.where(inside, words[np.clip(leaf_ind, 0, max(K - 1, 0))] if K else np.uint64(0), np.uint64(0))
    member = ((w[:, None] >> np.arange(Q, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    if row_ok is not None:
        member &= np.asarray(row_ok, bool)[:, None]
    if group_keep is not None:
        member &= np.asarray(group_keep, bool)[None, :]
    return member


def multi_split(leaf_ind, words, Q, row_ok=None, group_keep=None):
    """(begin [Q + 1], rows, counts [Q] before group_keep): np.nonzero per group, ascending"""
    member = membership(leaf_ind, words, Q, row_ok, group_keep)
    per = [np.nonzero(member[:, q])[0] for q in range(Q)]
    begin = np.concatenate([[0], np.cumsum([len(r) for r in per])]).astype(np.int64)
    rows = np.concatenate(per).astype(np.int64) if per else np.zeros(0, np.int64)
    return begin, rows, membership(leaf_ind, words, Q, row_ok, None).sum(0).astype(np.int64)
