"""Generate tests/golden/query_golden.npz by RUNNING THE REFERENCE's own code on the CPU.

Run in the build container only (``python tests/golden/make_query_golden.py``): /root/reference never travels, only the
arrays do, and none of its text is stored.

(a) ``calculate_metrics`` of scripts/eval_scannet.py:55-93, the module loaded by path with a stub registered as `plyfile`.
(b) lines 158-163 of scripts/eval_scannet.py (normalise, similarity, argmax over the texts, gather per point), read from the
    source, dedented and executed in a namespace that holds the inputs.
(c) the block of render_lerf_by_text.py from its ``F.normalize(text_feat...`` line to its ``torch.cat`` line (the text-to-leaf
    selection, :102-115), the same way, once per query text.
A token of the first and of the last line of (b) and (c) is asserted first, so that a shifted file is noticed.

The inputs come from tests/query_cases.py; the features are stored as the int8 multiples of 1 / 16 they were drawn as.  Every
stored case is asserted to be tie-free with margins (tests/query_cases.MARGIN = 1e-3): the argmax gap and the rank-top /
rank-top+1 gap of every similarity row, the argmax gap of every similarity column, and every centre distance that decides a
merge against 0.9; the gaps between the ranks in between, which only order the appended ids, exceed ORDER_MARGIN = 2e-4.
"""
import importlib.util
import os
import sys
import textwrap
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import query_cases as qc            # noqa: E402
from tests import query_restatement as qr      # noqa: E402

REF_EVAL = "/root/reference/scripts/eval_scannet.py"
REF_TEXT = "/root/reference/render_lerf_by_text.py"
EVAL_BLOCK = (158, 163)                        # 1-based, inclusive
TOP = 10


def load_eval_module():
    sys.modules.setdefault("plyfile", types.SimpleNamespace(PlyData=None, PlyElement=None))
    spec = importlib.util.spec_from_file_location("ref_eval_scannet", REF_EVAL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def eval_block():
    lines = open(REF_EVAL).read().splitlines()[EVAL_BLOCK[0] - 1:EVAL_BLOCK[1]]
    assert "F.normalize(query_text_feats" in lines[0] and "max_id[leaf_ind] + 1" in lines[-1], (lines[0], lines[-1])
    return compile(textwrap.dedent("\n".join(lines)), "eval_scannet_block", "exec")


def text_block():
    lines = open(REF_TEXT).read().splitlines()
    first = next(i for i, l in enumerate(lines) if "F.normalize(text_feat" in l)
    last = next(i for i in range(first, len(lines)) if "torch.cat(" in lines[i])
    assert "text_feat = F.normalize(text_feat.unsqueeze(0)" in lines[first] and "candidate_id.unsqueeze(0)" in lines[last]
    assert last - first == 13, (first, last)
    return compile(textwrap.dedent("\n".join(lines[first:last + 1])), "render_lerf_by_text_block", "exec")


def main():
    ref = load_eval_module()
    ev, tx = eval_block(), text_block()
    out = {"seeds": np.array(qc.GOLD_SEEDS), "top": np.array(TOP)}
    for seed in qc.GOLD_SEEDS:
        c, p = qc.text_case(seed), qc.point_case(seed)
        K, T = c["leaf"].shape[0], c["text"].shape[0]
        k = f"s{seed}"
        # ---- (c) text -> leaves, occupancy threshold 5 (:62) ----------------------------------------------------------
        leaf5 = torch.from_numpy(c["leaf"].copy())
        leaf5[torch.from_numpy(c["occu"]) < 5] *= 0.0
        book = {"ins_feat": torch.from_numpy(c["centers"])}
        leaf_num = K / torch.tensor(qc.GOLD_ROOTS)                      # `leaf_lang_feat.shape[0] / root_num`, :66
        assert float(leaf_num) == float(c["leaf_num"])
        sims, sel, cnt = [], np.full((T, TOP), -1, np.int32), np.zeros(T, np.int32)
        for q in range(T):
            ns = {"torch": torch, "F": F, "text_feat": torch.from_numpy(c["text"][q].copy()), "leaf_lang_feat": leaf5.clone(),
                  "leaf_code_book": book, "leaf_num": leaf_num}
            exec(tx, ns)
            ids = ns["text_leaf_indices"].numpy()
            sel[q, :len(ids)], cnt[q] = ids, len(ids)
            sims.append(ns["cosine_similarity"][0].numpy())
        sim5 = np.stack(sims)
        s64 = qr.similarity(c["text"], c["leaf"], c["occu"], 5)
        assert np.abs(s64 - sim5).max() < 1e-6
        first, cut = qr.row_margins(s64, TOP)
        assert min(first.min(), cut.min()) > qc.MARGIN, (seed, first.min(), cut.min())
        assert qr.rank_margin(s64, TOP) > qc.ORDER_MARGIN, (seed, qr.rank_margin(s64, TOP))
        assert qr.merge_margin(s64, c["centers"], c["leaf_num"], TOP) > qc.MARGIN, seed
        assert cnt.max() > 1 and cnt.min() == 1, (seed, cnt)                # merges happen, and not everywhere
        assert (c["occu"] < 2).any() and ((c["occu"] >= 2) & (c["occu"] < 5)).any()
        # ---- (b) leaves -> point classes, occupancy threshold 2 (:143-144) -------------------------------------------
        leaf2 = torch.from_numpy(c["leaf"].copy())
        leaf2[torch.from_numpy(c["occu"]) < 2] *= 0.0
        ns = {"torch": torch, "F": F, "query_text_feats": torch.from_numpy(c["text"].copy()), "leaf_lang_feat": leaf2,
              "leaf_ind": torch.from_numpy(p["leaf_ind"]).clamp(max=K - 1)}
        exec(ev, ns)
        pred = ns["pred_pts_cls_id"].numpy()
        s2 = qr.similarity(c["text"], c["leaf"], c["occu"], 2)
        col = -np.sort(-s2, axis=0)
        live = c["occu"] >= 2
        assert (col[0] - col[1])[live].min() > qc.MARGIN, seed              # a zeroed leaf ties at 0 by design: class 0
        assert (p["leaf_ind"] == K).any()
        # ---- (a) metrics, with and without the ignore mask ------------------------------------------------------------
        for tag, ign in (("plain", None), ("ignore", p["ignore"])):
            gt = torch.from_numpy(p["gt"].copy())
            if ign is not None:
                gt[torch.from_numpy(ign)] = 0                               # `updated_gt_labels[ignored_pts] = 0`, :132
            ious, miou, acc, macc = ref.calculate_metrics(gt, torch.from_numpy(pred.copy()), T + 1)
            out[f"{k}/{tag}/ious"] = ious.numpy()
            out[f"{k}/{tag}/scalars"] = np.array([miou, acc, macc], np.float64)
        out[f"{k}/text_q"], out[f"{k}/leaf_q"] = c["text_q"], c["leaf_q"]
        out[f"{k}/occu"], out[f"{k}/centers"] = c["occu"].astype(np.int16), c["centers"]
        out[f"{k}/leaf_ind"], out[f"{k}/gt"], out[f"{k}/ignore"] = p["leaf_ind"].astype(np.uint8), p["gt"].astype(np.uint8), p["ignore"]
        out[f"{k}/sim5"], out[f"{k}/selected"], out[f"{k}/count"], out[f"{k}/pred"] = sim5, sel, cnt, pred.astype(np.uint8)
    # labels all zero: every mean is over nothing
    gt0 = torch.zeros(300, dtype=torch.int64)
    ious, miou, acc, macc = ref.calculate_metrics(gt0, torch.randint(1, 20, (300,), generator=torch.Generator().manual_seed(1)), 20)
    out["allzero/ious"], out["allzero/scalars"] = ious.numpy(), np.array([miou, acc, macc], np.float64)
    path = os.path.join(HERE, "query_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
