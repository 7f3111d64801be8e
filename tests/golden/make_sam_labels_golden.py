"""Generate tests/golden/sam_labels_golden.npz by RUNNING THE REFERENCE's own get_SAM_mask_and_feat on the CPU.

Run in the build container only (``python tests/golden/make_sam_labels_golden.py``): /root/reference never travels,
only the vectors do.  As in make_mask_golden.py the function is compiled from its source text (ast) into a namespace
holding only torch / F, because utils/opengs_utlis.py imports the absent `bitarray`.

Inputs are regenerated from the seed by ``case_inputs`` (shared with the tests): a [4, H, W] stack of SAM mask ids in
the layout of the reference's data loader -- level l's ids start after level l-1's maximum, -1 = no mask -- where one
of the levels 0 / 3 is entirely -1 (num_mask = 0) and the other one misses an id below its maximum (an empty mask row),
and a [total ids, 8] table of per-mask features.  The file stores, for levels 0 and 3, mask_id, invalid_pix, mask_bool
(as uint8) and mask_feat.
"""
import os

import numpy as np
import torch

try:
    from tests.golden.make_mask_golden import load_functions
except ImportError:                                     # run as a script from the repository root
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from tests.golden.make_mask_golden import load_functions

HERE = os.path.dirname(os.path.abspath(__file__))
REF_UTILS = "/root/reference/utils/opengs_utlis.py"
LEVELS = (0, 3)
PER_LEVEL = (5, 7, 9, 11)                               # ids per level before one is taken out

# (seed, H, W, dtype name, the level that is entirely -1)
CASES = [(0, 20, 28, "int64", 3), (1, 20, 28, "float32", 0), (2, 31, 29, "int64", 0), (3, 31, 29, "float32", 3)]


def case_id(case):
    seed, H, W, dtype, none_level = case
    return f"s{seed}_{H}x{W}_{dtype}"


def case_inputs(seed, H, W, dtype, none_level):
    """-> (gt_sam_mask [4,H,W] of `dtype`, mask features [total, 8] float32)"""
    g = torch.Generator().manual_seed(900 + seed)
    absent_level = LEVELS[0] if none_level == LEVELS[1] else LEVELS[1]
    levels, start = [], 0
    for lvl, n in enumerate(PER_LEVEL):
        coarse = torch.randint(-1, n, ((H + 3) // 4, (W + 3) // 4), generator=g)
        local = coarse.repeat_interleave(4, 0).repeat_interleave(4, 1)[:H, :W].clone()
        noise = torch.rand(H, W, generator=g) < 0.1
        local = torch.where(noise, torch.randint(-1, n, (H, W), generator=g), local)
        local[0, :4] = n - 1                            # the level's largest id is present
        if lvl == absent_level:
            local[local == n // 2] = -1                 # an id below the maximum with no pixel: an empty mask row
        if lvl == none_level:
            local[:] = -1
        levels.append(torch.where(local >= 0, local + start, local))
        start = max(start, int(levels[-1].max()) + 1)
    feats = torch.rand(start, 8, generator=g)
    return torch.stack(levels).to(getattr(torch, dtype)), feats


def main():
    fn = load_functions(REF_UTILS, ["get_SAM_mask_and_feat"])["get_SAM_mask_and_feat"]
    out = {}
    for case in CASES:
        gt, feats = case_inputs(*case)
        for level in LEVELS:
            k = f"{case_id(case)}_L{level}"
            mask_id, mask_bool, mask_feat, invalid = fn(gt.clone(), level=level, original_mask_feat=feats.clone())
            three = fn(gt.clone(), level=level)
            assert len(three) == 3 and torch.equal(three[0], mask_id) and torch.equal(three[2], invalid)
            out[k + "_mask_id"] = mask_id.numpy()
            out[k + "_invalid_pix"] = invalid.numpy()
            out[k + "_mask_bool"] = mask_bool.contiguous().numpy().astype(np.uint8)
            out[k + "_mask_feat"] = mask_feat.numpy()
            print(k, "num_mask", mask_bool.shape[0], "empty rows", int((mask_bool.flatten(1).sum(1) == 0).sum()),
                  "mask_feat", tuple(mask_feat.shape), mask_id.dtype)
    path = os.path.join(HERE, "sam_labels_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
