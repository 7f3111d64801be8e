"""Generate tests/golden/separation_golden.npz by RUNNING THE REFERENCE's own separation_loss body on the CPU.

Run in the build container only (``python tests/golden/make_separation_golden.py``): /root/reference never travels, only
the vectors do.  The function is compiled from train.py's source text (ast), as make_mask_golden.py does; no text is
stored.

For every (N, C) of CASES and both weightings -- early (iteration 1000) and late (iteration 40000: weights below 0.9
become 0.1) -- the file holds the reference's value and its autograd gradient w.r.t. the means in float64, and e32, the
largest deviation of its float32 gradient from the float64 one relative to the largest float64 entry: what the
reference's own arithmetic is good to, which the GPU test takes as the scale of its gradient bar.

The means are regenerated from the seed by ``case_means`` (shared with the tests): uniform in [0, 1), redrawn until every
row's float64 inverse distances lie at least GAP apart (tests/test_31_label_masks_gpu.py has the reasoning for 2e-6), so
that no float32 evaluation can rank two of them the other way round and argsort()'s order among equals never matters.
N = 10, 19, 37 have N - 1 divisible by 9: rank 8 (N-1) / 9 sits exactly on the late threshold, where
(8/9) * 0.9 + 0.1 rounds to 0.90000004 in float32 and is kept.
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_TRAIN = "/root/reference/train.py"

CASES = [(N, C) for N in (2, 3, 10, 19, 37) for C in (1, 6, 16)]
ITERATIONS = {"early": 1000, "late": 40000}
GAP = 2e-6


def rank_gap(mean):
    """per row, the smallest distance between two of the float64 inverse distances the loss ranks (diagonal = 0)"""
    m = mean.double()
    N = m.shape[0]
    inv = 1.0 / ((m[:, None] - m[None]).pow(2).sum(2) + 1)
    s = inv.masked_fill(torch.eye(N, dtype=torch.bool), 0).sort(dim=1).values
    return (s[:, 1:] - s[:, :-1]).min(dim=1).values


def case_means(N, C):
    """float32 means [N, C], uniform in [0, 1), the first draw of the seeded generator whose ranks are well conditioned"""
    g = torch.Generator().manual_seed(3400 + 100 * N + C)
    for _ in range(1000):
        m = torch.rand(N, C, generator=g)
        if float(rank_gap(m).min()) >= GAP:
            return m
    raise AssertionError(f"no well-separated means for N = {N}, C = {C}")


def main():
    from make_mask_golden import load_functions
    sep = load_functions(REF_TRAIN, ["separation_loss"])["separation_loss"]
    out = {}
    for N, C in CASES:
        base = case_means(N, C)
        assert float(rank_gap(base).min()) >= GAP
        for mode, it in ITERATIONS.items():
            res = {}
            for dtype in (torch.float64, torch.float32):
                m = base.clone().to(dtype).requires_grad_(True)
                loss = sep(m, it)
                loss.backward()
                res[dtype] = (loss.detach(), m.grad)
            v64, g64 = res[torch.float64]
            g32 = res[torch.float32][1]
            k = f"n{N}_c{C}_{mode}"
            out[k + "_value"] = np.float64(v64.item())
            out[k + "_grad"] = g64.numpy()
            out[k + "_e32"] = np.float64(((g32.double() - g64).abs().max() / g64.abs().max()).item())
    np.savez_compressed(os.path.join(HERE, "separation_golden.npz"), **out)
    print("wrote", len(out), "arrays; largest e32", max(float(v) for k, v in out.items() if k.endswith("_e32")))


if __name__ == "__main__":
    main()
