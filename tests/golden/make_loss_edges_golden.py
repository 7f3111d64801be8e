"""Generate tests/golden/loss_edges_golden*.npz by RUNNING THE REFERENCE's own function bodies on the CPU, for the edge
cases of tests/test_36_losses_edges_gpu.py and tests/test_losses_edges_host.py.

Run in the build container only (``python tests/golden/make_loss_edges_golden.py``).  The functions come from
``make_loss_golden.load_functions`` (compiled from the reference's text at generation time; none of it is stored).  The
file names do not match ``loss_golden*.npz``, which ``make_loss_golden.main()`` deletes and ``load_golden()`` reads.

Inputs are regenerated from seeds by ``photo_inputs`` / ``masked_inputs`` / ``extreme_inputs`` (shared with the tests).

Photometric case pK (PHOTO_CASES[K]), from an fp64 run: ``pK_l1``, ``pK_ssim`` and ``pK_grad_ssim`` = d ssim / d img.  The L1
gradient is exactly sign(img - gt) / N and is not stored.  From an fp32 run of the same functions:
  pK_v32_l1, _v32_ssim, _v32_loss02, _v32_loss10   relative deviation from fp64 of L1, SSIM, the loss at lambda 0.2 and 1
  pK_e32_ssim, pK_e32_loss02                       largest deviation of the fp32 gradient from the fp64 gradient over the
                                                   largest fp64 entry: the SSIM gradient alone, the lambda = 0.2 loss
  pK_e32_ssim_<band>, pK_e32_loss02_<band>         the same restricted to a band of ``bands(H, W)``, over the band's own
                                                   largest fp64 entry
Masked case (``masked_key``): the fp64 value per loss l1 / l2; ``_dx`` and ``_e32`` only for HW in DX_STORED.
Extreme case (``extreme_key``): the fp64 value per loss; ``_dx`` and ``_e32`` only for the kind "negw".
"""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

try:
    from tests.golden import make_loss_golden as mg
except ImportError:                                   # run as a script from anywhere
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from tests.golden import make_loss_golden as mg

HERE = os.path.dirname(os.path.abspath(__file__))
PATTERN = "loss_edges_golden*.npz"
SHARD_BYTES = mg.SHARD_BYTES

# (H, W, kind): a dimension of 1, at and below the window radius, the window size +- 1, whole tiles only, one past a tile in
# both directions, overshooting / constant / almost identical images
PHOTO_CASES = [(1, 1, "near"), (1, 40, "near"), (40, 1, "near"), (5, 5, "near"), (6, 6, "near"), (10, 10, "near"),
               (11, 11, "near"), (12, 12, "near"), (32, 32, "near"), (33, 33, "near"), (32, 65, "near"), (64, 96, "near"),
               (70, 70, "over"), (45, 70, "black"), (45, 70, "white"), (70, 75, "delta")]
PHOTO_IDS = ["%dx%d-%s" % c for c in PHOTO_CASES]
DELTA = 0.25
BANDS = ("border", "seam", "corners")
TILE, RADIUS = 32, 5
# (lambda, u, v): u on `loss`, v on `Ll1`
UPSTREAM = [(0.0, 1.0, 0.0), (1.0, 1.0, 0.0), (0.2, 0.0, 1.0), (0.2, 1.0, 0.5), (0.2, -2.0, 0.0), (0.2, 1e-3, 0.0)]

# H*W -> (H, W), as tests/test_35_mask_edges_gpu.py: around the float4, wave and workgroup sizes
MASKED_HW = {1: (1, 1), 3: (1, 3), 4: (2, 2), 5: (1, 5), 255: (15, 17), 256: (16, 16), 257: (1, 257), 1023: (31, 33),
             1024: (32, 32), 1025: (25, 41), 1028: (4, 257)}
MASKED_KINDS = ["one_hw", "chw", "none", "weight", "weight_chw"]
MASKED_CASES = [(hw, C, kind) for hw in MASKED_HW for C in (3, 6) for kind in MASKED_KINDS]
DX_STORED = (5, 1028)
EXTREME_SHAPES = [(6, 33, 47), (3, 16, 20)]
EXTREME_KINDS = ["all_true", "last_only", "zero_weight", "negw", "equal_tenth"]
EXTREME_CASES = [(s, k) for s in EXTREME_SHAPES for k in EXTREME_KINDS]


def delta_pixels(H, W):
    return [(0, 31, 31), (1, 32, 32), (2, 0, 0), (0, H - 1, W - 1), (1, 31, W - 1)]


def photo_inputs(index):
    """(img, gt) fp32 [3,H,W] of PHOTO_CASES[index]; gt as in make_loss_golden.photo_inputs"""
    H, W, kind = PHOTO_CASES[index]
    g = torch.Generator().manual_seed(1900 + index)
    coarse = torch.rand(1, 3, H // 8 + 2, W // 8 + 2, generator=g)
    gt = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[0]
    gt = (gt + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    if kind == "black":
        gt = torch.zeros(3, H, W)
    elif kind == "white":
        gt = torch.ones(3, H, W)
    if kind == "over":
        img = 1.6 * gt - 0.2 + 0.05 * torch.randn(3, H, W, generator=g)         # unclamped: below 0 and above 1
    elif kind == "delta":
        img = gt.clone()
        for c, y, x in delta_pixels(H, W):
            img[c, y, x] += DELTA
    else:
        img = (gt + 0.03 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    return img.contiguous(), gt.contiguous()


def bands(H, W):
    """name -> bool [H, W]: `border` within 5 pixels of an image edge, `seam` within 5 pixels of a 32-pixel tile edge,
    `corners` the four 5 x 5 corner blocks"""
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    ey, ex = (y < RADIUS) | (y >= H - RADIUS), (x < RADIUS) | (x >= W - RADIUS)
    near_seam = lambda v: (v % TILE < RADIUS) | (v % TILE >= TILE - RADIUS)
    out = {"border": ey | ex, "seam": near_seam(y) | near_seam(x), "corners": ey & ex}
    return {k: np.broadcast_to(v, (H, W)).copy() for k, v in out.items()}


def l1_gradient(img, gt):
    """d mean|img - gt| / d img in fp64: exactly sign(img - gt) / N"""
    return torch.sign(img.double() - gt.double()).numpy() / img.numel()


def random_masked(C, H, W, kind, seed):
    """(x, t, mask or None, weight or None); masks bool, about half set; weights uniform in [0, 1)"""
    g = torch.Generator().manual_seed(seed)
    x, t = torch.rand(C, H, W, generator=g), torch.rand(C, H, W, generator=g)
    half = lambda *s: torch.rand(*s, generator=g) < 0.5
    if kind == "none":
        return x, t, None, None
    per_channel = kind in ("chw", "weight_chw")
    mask = half(C, H, W) if per_channel else half(1, H, W)
    weight = torch.rand(*mask.shape, generator=g) if kind.startswith("weight") else None
    return x, t, mask, weight


def masked_inputs(index):
    hw, C, kind = MASKED_CASES[index]
    return random_masked(C, *MASKED_HW[hw], kind, 2000 + index)


def masked_key(index):
    hw, C, kind = MASKED_CASES[index]
    return f"e{hw}_c{C}_{kind}"


def extreme_inputs(index):
    """(x, t, mask [1,H,W], weight [1,H,W] or None) of EXTREME_CASES[index]"""
    (C, H, W), kind = EXTREME_CASES[index]
    g = torch.Generator().manual_seed(2500 + index)
    x, t = torch.rand(C, H, W, generator=g), torch.rand(C, H, W, generator=g)
    mask, weight = torch.rand(1, H, W, generator=g) < 0.5, None
    if kind == "all_true":
        mask = torch.ones(1, H, W, dtype=torch.bool)
    elif kind == "last_only":                                       # denominator 1
        mask = torch.zeros(1, H, W, dtype=torch.bool)
        mask[0, H - 1, W - 1] = True
    elif kind == "zero_weight":
        weight = torch.zeros(1, H, W)
    elif kind == "negw":                                            # about half the weights are negative
        weight = torch.randn(1, H, W, generator=g)
    else:
        assert kind == "equal_tenth"
        same = (torch.rand(C, H, W, generator=g) < 0.1) & mask
        x = torch.where(same, t, x)
    return x.contiguous(), t, mask, weight


def extreme_key(index):
    (C, H, W), kind = EXTREME_CASES[index]
    return f"x{EXTREME_SHAPES.index((C, H, W))}_{kind}"


def load_golden():
    out = {}
    for path in sorted(glob.glob(os.path.join(HERE, PATTERN))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def rel_dev(g32, g64, where=None):
    """largest |g32 - g64| over the largest |g64|, both taken over `where` (bool [H, W]) when given"""
    g32, g64 = np.asarray(g32, np.float64), np.asarray(g64, np.float64)
    if where is not None:
        g32, g64 = g32[..., where], g64[..., where]
    top = np.abs(g64).max()
    return np.float64(0.0 if top == 0 else np.abs(g32 - g64).max() / top)


def photo_run(fns, img, gt):
    """l1, ssim, the losses at lambda 0.2 and 1 (train.py:385-386), d ssim / d img and d loss02 / d img, in img's dtype.
    `fns` maps "l1_loss" and "ssim" to the functions to run."""
    x = img.clone().requires_grad_(True)
    ss = fns["ssim"](x, gt)
    ss.backward()
    g_ssim = x.grad.numpy().copy()
    x = img.clone().requires_grad_(True)
    l1, s2 = fns["l1_loss"](x, gt), fns["ssim"](x, gt)
    loss02 = (1.0 - 0.2) * l1 + 0.2 * (1.0 - s2)
    loss02.backward()
    loss10 = (1.0 - 1.0) * l1 + 1.0 * (1.0 - s2)
    return {"l1": l1.item(), "ssim": ss.item(), "loss02": loss02.item(), "loss10": loss10.item(), "grad_ssim": g_ssim,
            "grad_loss02": x.grad.numpy().copy()}


def photo_record(fns, index):
    """every array and scalar stored for PHOTO_CASES[index], from an fp64 and an fp32 run of `fns`"""
    H, W, _ = PHOTO_CASES[index]
    img, gt = photo_inputs(index)
    r64, r32 = photo_run(fns, img.double(), gt.double()), photo_run(fns, img, gt)
    k, out = f"p{index}_", {}
    out[k + "l1"], out[k + "ssim"], out[k + "grad_ssim"] = np.float64(r64["l1"]), np.float64(r64["ssim"]), r64["grad_ssim"]
    for name in ("l1", "ssim", "loss02", "loss10"):
        out[k + "v32_" + name] = np.float64(abs(r32[name] - r64[name]) / abs(r64[name]))
    for name in ("ssim", "loss02"):
        out[k + "e32_" + name] = rel_dev(r32["grad_" + name], r64["grad_" + name])
        for band, where in bands(H, W).items():
            out[f"{k}e32_{name}_{band}"] = rel_dev(r32["grad_" + name], r64["grad_" + name], where)
    return out


def masked_run(fn, x, t, mask, weight):
    xx = x.clone().requires_grad_(True)
    v = fn(xx, t, mask, weight)
    v.backward()
    return v.item(), xx.grad.numpy()


def masked_record(fns, key, inputs, with_dx):
    x, t, mask, weight = inputs
    out = {}
    for name in ("l1", "l2"):
        fn = fns[name + "_loss"]
        v64, g64 = masked_run(fn, x.double(), t.double(), mask, None if weight is None else weight.double())
        out[f"{key}_{name}"] = np.float64(v64)
        if with_dx:
            _, g32 = masked_run(fn, x, t, mask, weight)
            out[f"{key}_{name}_dx"], out[f"{key}_{name}_e32"] = g64, rel_dev(g32, g64)
    return out


def all_records(fns):
    out = {}
    for i in range(len(PHOTO_CASES)):
        out.update(photo_record(fns, i))
    for i, (hw, _, _) in enumerate(MASKED_CASES):
        out.update(masked_record(fns, masked_key(i), masked_inputs(i), hw in DX_STORED))
    for i, (_, kind) in enumerate(EXTREME_CASES):
        out.update(masked_record(fns, extreme_key(i), extreme_inputs(i), kind == "negw"))
    return out


def main():
    out = all_records(mg.load_functions(mg.REF_LOSS, mg.WANT))
    for i, c in enumerate(PHOTO_CASES):
        k = f"p{i}_"
        print(c, " ".join("%s %.2e" % (n, out[k + n]) for n in sorted(x[len(k):] for x in out if x.startswith(k))
                          if n[:3] in ("v32", "e32")))
    for old in glob.glob(os.path.join(HERE, PATTERN)):
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
        path = os.path.join(HERE, "loss_edges_golden.npz" if j == 0 else f"loss_edges_golden_{j}.npz")
        np.savez_compressed(path, **sh)
        print("wrote", path, len(sh), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
