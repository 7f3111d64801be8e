"""Seeded scenes and pixel-label images for the label-votes tests, at the smallest shapes at which the kernel can go wrong.

Scenes: those of tests/label_map_cases.py (image 40 x 24: 3 x 2 tiles, 5 x 3 quadrants of 8 x 8 pixels, the last tile column and
row partial, tile (0, 0) empty, 1 % of the points behind the near plane; P = 300 and 1500 on either side of the single-workgroup
geometry path) and `wide`: the P = 300 scene plus 24 Gaussians with a footprint sigma of 3-9 px and opacity 0.1-0.5, each
spanning several tiles and many labels.

Label images (int64 [H, W]); `fold` is the number of local labels of one column block of the kernel's fold, `cap` the number of
distinct labels one quadrant can hold (64 = its pixels):
    blocks8   one label per 8 x 8 quadrant
    blocks4   four labels per quadrant (4 x 4 blocks)
    noise     uniform per pixel in [0, L), a third of the pixels -1, four values out of range (L, L + 3, -2, -7)
    fold_k    noise with L = 5, but ONE quadrant of tile (1, 0) holds k distinct labels: k = fold - 1, fold, fold + 1, 2 fold + 1
    cap_64    the same with all 64 pixels of the quadrant distinct
    null      all pixels -1
    L0        num_labels = 0: one column
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from opengaussian_amd.synthetic import Scene
from tests import label_map_cases as lmc

W, H, F = lmc.W, lmc.H, lmc.F
GRAD_BAR = 2e-4            # the project's gradient bar, relative to the table's maximum
DECIDED = 2 * GRAD_BAR     # a row is decided when the oracle's weight - second exceeds this share of the table's maximum
NUM_WIDE = 24
NOISE_LS = (1, 5, 70, 700)
LEAF_ROWS = 7
QUAD_X0, QUAD_Y0 = 24, 0   # the many-label quadrant: quadrant 1 of tile (1, 0)


@functools.lru_cache(maxsize=None)
def scene(name):
    """'P300', 'P1500' or 'wide' -> (Scene, camera)"""
    if name != "wide":
        c = lmc.scene_case(int(name[1:]), 5)
        return c["sc"], c["cam"]
    base, cam = scene("P300")
    g = torch.Generator().manual_seed(4242)
    n = NUM_WIDE
    px = torch.rand(n, generator=g) * W
    py = torch.rand(n, generator=g) * H
    z = torch.rand(n, generator=g) * 8.0 + 2.0
    means = torch.stack([(px + 0.5 - W / 2) * z / F, (py + 0.5 - H / 2) * z / F, z], dim=1)
    sigma_px = torch.rand(n, 3, generator=g) * 6.0 + 3.0
    scales = sigma_px * z[:, None] / F
    q = torch.randn(n, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    opac = torch.rand(n, 1, generator=g) * 0.4 + 0.1
    cat = lambda a, b: torch.cat([a, b]).contiguous()
    sc = Scene(cat(base.means3D, means), cat(base.scales, scales), cat(base.rotations, q), cat(base.opacities, opac),
               torch.zeros(300 + n, 16, 3), torch.zeros(300 + n, 6))
    return sc, cam


def _noise(L, g):
    lab = torch.randint(0, max(L, 1), (H, W), generator=g, dtype=torch.int64)
    lab[torch.rand(H, W, generator=g) < 1.0 / 3.0] = -1
    flat = lab.view(-1)
    flat[torch.randperm(H * W, generator=g)[:4]] = torch.tensor([L, L + 3, -2, -7])
    return lab


@functools.lru_cache(maxsize=None)
def label_image(kind, L, k=0):
    """(int64 [H, W] image, L)"""
    g = torch.Generator().manual_seed(9000 + 31 * L + k + sum(map(ord, kind)))
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    if kind == "blocks8":
        return ((7 * ((y // 8) * 5 + x // 8) + 3) % L).to(torch.int64), L
    if kind == "blocks4":
        return ((5 * ((y // 4) * 10 + x // 4) + 1) % L).to(torch.int64), L
    if kind == "noise":
        return _noise(L, g), L
    if kind == "null":
        return torch.full((H, W), -1, dtype=torch.int64), L
    if kind == "many":
        # k distinct labels, 3, 10, 17, ... in a random order over the quadrant's 64 pixels, every one of them at least once
        lab = _noise(5, g)
        which = torch.cat([torch.randperm(k, generator=g), torch.randint(0, k, (64 - k,), generator=g)])
        which = which[torch.randperm(64, generator=g)]
        lab[QUAD_Y0:QUAD_Y0 + 8, QUAD_X0:QUAD_X0 + 8] = (which * 7 + 3).reshape(8, 8)
        return lab, 7 * k + 3
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def leaf_rows(P):
    """leaf-like rows: ids in [0, LEAF_ROWS), a tenth -1, a few >= LEAF_ROWS"""
    g = torch.Generator().manual_seed(77 + P)
    r = torch.randint(0, LEAF_ROWS, (P,), generator=g, dtype=torch.int64)
    r[torch.rand(P, generator=g) < 0.1] = -1
    r[torch.randperm(P, generator=g)[:5]] = torch.tensor([LEAF_ROWS, LEAF_ROWS + 2, 1000, -3, 2 ** 40])
    return r


def many_counts(fold, cap):
    ks = [fold - 1, fold, fold + 1, 2 * fold + 1] if cap >= 64 else [cap - 1, cap, cap + 1]
    return [k for k in ks if 1 <= k < 64] + [64]


CASE_NAMES = ([f"{s}_{kind}" for s in ("P300", "P1500") for kind in ("blocks8", "blocks4") + tuple(f"noise{L}" for L in NOISE_LS)]
              + ["wide_blocks8", "wide_noise70", "P300_null", "P300_L0"] + [f"P1500_many{i}" for i in range(5)])
LABEL_CHECK = [n for n in CASE_NAMES if n not in ("wide_noise70", "P300_null", "P300_L0")]


@functools.lru_cache(maxsize=None)
def case(name, fold=16, cap=64):
    """name -> dict(name, sc, cam, image [H, W] int64, L, many = number of labels of the many-label quadrant or 0)"""
    s, kind = name.split("_", 1)
    sc, cam = scene(s)
    many = 0
    if kind.startswith("noise"):
        img, L = label_image("noise", int(kind[5:]))
    elif kind == "blocks8":
        img, L = label_image("blocks8", 11)
    elif kind == "blocks4":
        img, L = label_image("blocks4", 23)
    elif kind == "null":
        img, L = label_image("null", 5)
    elif kind == "L0":
        img, L = label_image("noise", 5)[0], 0
    elif kind.startswith("many"):
        counts = many_counts(fold, cap)
        many = counts[min(int(kind[4:]), len(counts) - 1)]
        img, L = label_image("many", 5, many)
    else:
        raise KeyError(name)
    return dict(name=name, sc=sc, cam=cam, image=img, L=int(L), many=many)


def clamp_labels(image, L):
    """lab(p): the image's value inside [0, L), else L"""
    img = np.asarray(image, np.int64)
    return np.where((img >= 0) & (img < L), img, L)


@functools.lru_cache(maxsize=None)
def oracle(name, fold=16, cap=64):
    """float64 restatement of a case (rows = None), computed once per process and read-only"""
    from tests import label_votes_restatement as vr
    c = case(name, fold, cap)
    table = vr.vote_table(c["sc"], c["cam"], c["image"].numpy(), c["L"])
    table.setflags(write=False)
    return table


@functools.lru_cache(maxsize=None)
def oracle_fp32(name, fold=16, cap=64):
    """the same graph evaluated in fp32: what attributes a threshold flip"""
    from tests import label_votes_restatement as vr
    c = case(name, fold, cap)
    table = vr.vote_table(c["sc"], c["cam"], c["image"].numpy(), c["L"], dtype=torch.float32)
    table.setflags(write=False)
    return table


def tanfovs(cam):
    return math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
