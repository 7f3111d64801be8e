"""Generate tests/golden/loss_golden*.npz by RUNNING THE REFERENCE's own function bodies on the CPU.

Run in the build container only (``python tests/golden/make_loss_golden.py``): /root/reference never travels, only the
vectors do.  l1_loss, l2_loss, gaussian, create_window, ssim, _ssim are compiled one by one from the text of
utils/loss_utils.py (ast) into a namespace holding torch / F / Variable / exp; none of that text is stored.

Inputs are regenerated from a seed by ``photo_inputs`` / ``masked_inputs`` (``case_inputs`` dispatches; shared with the tests).
Per photometric case pK the file holds, from an fp64 run, the L1, the SSIM, the loss with lambda = 0.2 and d loss / d image
(``pK_l1``, ``_ssim``, ``_loss``, ``_grad``), the same four from an fp32 run (``pK_f32_...``) and ``pK_e32``: the fp32 run's
largest gradient deviation from the fp64 run over the largest fp64 gradient entry.  Per masked case mK_<mask> and loss
l1 / l2: the fp64 value and dx and the matching e32.

No committed file may pass 1 MiB and fp64 noise does not compress, so the arrays are spread over loss_golden.npz,
loss_golden_1.npz, ...; ``load_golden`` reads them back as one dict.
"""
import ast
import glob
import os
from math import exp

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF_LOSS = "/root/reference/utils/loss_utils.py"
WANT = ["l1_loss", "l2_loss", "gaussian", "create_window", "ssim", "_ssim"]
LAMBDA = 0.2
SHARD_BYTES = 880 * 1024

# (H, W, kind): smaller than the window, one more / one less than 16 / 32 / 64 / 128, long thin strips
PHOTO_CASES = [(7, 9, "near"), (16, 16, "far"), (33, 47, "near"), (31, 63, "near"), (70, 131, "near"), (17, 300, "far"),
               (15, 257, "far"), (129, 65, "near"), (40, 40, "flat"), (40, 40, "same")]
MASKED_SHAPES = [(6, 33, 47), (3, 17, 300)]
MASK_KINDS = ["one_hw", "hw", "chw", "empty", "weight", "none"]
MASKED_CASES = [(s, k) for s in MASKED_SHAPES for k in MASK_KINDS]


def photo_inputs(index):
    """(img, gt) fp32 [3,H,W] of PHOTO_CASES[index]"""
    H, W, kind = PHOTO_CASES[index]
    g = torch.Generator().manual_seed(900 + index)
    if kind == "flat":
        return torch.full((3, H, W), 0.5), torch.full((3, H, W), 0.25)
    coarse = torch.rand(1, 3, H // 8 + 2, W // 8 + 2, generator=g)
    gt = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[0]
    gt = (gt + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    if kind == "near":
        img = (gt + 0.03 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    elif kind == "far":
        img = torch.rand(3, H, W, generator=g)
    else:
        assert kind == "same"
        img = gt.clone()
    return img.contiguous(), gt.contiguous()


def masked_inputs(index):
    """(x, t, mask or None, weight or None) of MASKED_CASES[index]; masks bool, about half set"""
    (C, H, W), kind = MASKED_CASES[index]
    g = torch.Generator().manual_seed(950 + index)
    x, t = torch.rand(C, H, W, generator=g), torch.rand(C, H, W, generator=g)
    half = lambda *s: torch.rand(*s, generator=g) < 0.5
    mask = {"one_hw": lambda: half(1, H, W), "hw": lambda: half(H, W), "chw": lambda: half(C, H, W),
            "empty": lambda: torch.zeros(1, H, W, dtype=torch.bool), "weight": lambda: half(1, H, W),
            "none": lambda: None}[kind]()
    weight = torch.rand(1, H, W, generator=g) if kind == "weight" else None
    return x, t, mask, weight


def case_inputs(family, index):
    return photo_inputs(index) if family == "photo" else masked_inputs(index)


def masked_key(index):
    (C, H, W), kind = MASKED_CASES[index]
    return f"m{MASKED_SHAPES.index((C, H, W))}_{kind}"


def load_golden():
    out = {}
    for path in sorted(glob.glob(os.path.join(HERE, "loss_golden*.npz"))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def load_functions(path, names):
    from torch.autograd import Variable
    tree = ast.parse(open(path).read())
    ns = {"torch": torch, "F": F, "Variable": Variable, "exp": exp}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    missing = [n for n in names if n not in ns]
    assert not missing, missing
    return ns


def _rel_dev(g32, g64):
    top = np.abs(g64).max()
    return np.float64(0.0 if top == 0 else np.abs(g32.astype(np.float64) - g64).max() / top)


def main():
    ref = load_functions(REF_LOSS, WANT)
    out = {}

    def photo(img, gt):
        x = img.clone().requires_grad_(True)
        l1 = ref["l1_loss"](x, gt)
        ss = ref["ssim"](x, gt)
        loss = (1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - ss)            # train.py:385-386
        loss.backward()
        return l1.item(), ss.item(), loss.item(), x.grad.numpy()

    for i in range(len(PHOTO_CASES)):
        img, gt = photo_inputs(i)
        r64, r32 = photo(img.double(), gt.double()), photo(img, gt)
        for pre, r in ((f"p{i}_", r64), (f"p{i}_f32_", r32)):
            out[pre + "l1"], out[pre + "ssim"], out[pre + "loss"] = (np.asarray(v, r[3].dtype) for v in r[:3])
            out[pre + "grad"] = r[3]
        out[f"p{i}_e32"] = _rel_dev(r32[3], r64[3])
        print(PHOTO_CASES[i], "l1 %.6g ssim %.6g loss %.6g e32 %.2e  value dev %.1e" % (
            *r64[:3], out[f"p{i}_e32"], max(abs(a - b) / max(abs(b), 1e-30) for a, b in zip(r32[:3], r64[:3]) if b)))

    def masked(fn, x, t, mask, weight):
        xx = x.clone().requires_grad_(True)
        v = fn(xx, t, mask, weight)
        v.backward()
        return v.item(), xx.grad.numpy()

    for i in range(len(MASKED_CASES)):
        x, t, mask, weight = masked_inputs(i)
        for name in ("l1", "l2"):
            fn = ref[name + "_loss"]
            v64, g64 = masked(fn, x.double(), t.double(), mask, None if weight is None else weight.double())
            v32, g32 = masked(fn, x, t, mask, weight)
            k = f"{masked_key(i)}_{name}"
            out[k], out[k + "_dx"], out[k + "_e32"] = np.float64(v64), g64, _rel_dev(g32, g64)
            print(k, "%.6g e32 %.2e" % (v64, out[k + "_e32"]))

    for old in glob.glob(os.path.join(HERE, "loss_golden*.npz")):
        os.remove(old)
    shards, size = [{}], 0
    for k in sorted(out):
        n = np.asarray(out[k]).nbytes
        if size + n > SHARD_BYTES and shards[-1]:
            shards.append({})
            size = 0
        shards[-1][k] = out[k]
        size += n
    for j, sh in enumerate(shards):
        path = os.path.join(HERE, "loss_golden.npz" if j == 0 else f"loss_golden_{j}.npz")
        np.savez_compressed(path, **sh)
        print("wrote", path, len(sh), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
