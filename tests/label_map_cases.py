"""Seeded scenes for the label-map tests, at the smallest shapes at which the kernel can go wrong.

Image 40 x 24: 3 x 2 tiles, the last column 8 and the last row 8 pixels wide (partial in both axes).  Tile (0, 0) sees no
Gaussian.  P = 300 and 1500 lie on either side of the 1024 single-workgroup geometry path (and above the 256 of the tiny path).
A third of the points is unlabelled (-1), wherever they lie in depth; a few labels are >= L or < -1.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from opengaussian_amd.synthetic import Scene, make_camera

W, H, F = 40, 24, 30.0
HOLE = 21.0            # no centre with px < HOLE and py < HOLE: with footprints of at most 3 px tile (0, 0) stays empty
DECIDED = 2e-4         # a pixel is decided when the oracle's weight - second exceeds this: twice the 1e-4 image bar
BAR = 1e-4             # the project's image bar

SCENE_PS = (300, 1500)
SCENE_LS = (1, 5, 70, 700)


def _scene(px, py, z, g):
    P = px.shape[0]
    means = torch.stack([(px + 0.5 - W / 2) * z / F, (py + 0.5 - H / 2) * z / F, z], dim=1)
    scales = torch.exp(torch.randn(P, 3, generator=g) * 0.5 - 3.6).clamp(max=0.05)
    q = torch.randn(P, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    opac = torch.sigmoid(torch.randn(P, 1, generator=g) * 2.0 - 0.5)
    return Scene(means.contiguous(), scales.contiguous(), q.contiguous(), opac.contiguous(), torch.zeros(P, 16, 3),
                 torch.zeros(P, 6))


def _scatter(P, g):
    px = torch.rand(4 * P, generator=g) * (W + 4) - 2
    py = torch.rand(4 * P, generator=g) * (H + 4) - 2
    keep = torch.nonzero(~((px < HOLE) & (py < HOLE))).flatten()[:P]
    assert keep.numel() == P
    z = torch.rand(P, generator=g) * 8.0 + 2.0
    n_cull = P // 100
    z[:n_cull] = torch.rand(n_cull, generator=g) * 1.2 - 1.0            # behind the near plane
    return px[keep], py[keep], z


@functools.lru_cache(maxsize=None)
def scene_case(P, L, null=False, wide=False):
    """dict(sc, cam, labels [P] int64, L): labels random in [0, L), a third -1, four out of range.  null: all unlabelled.
    wide: L = 2^31 - 1 and labels all over that range (every label its own dictionary window), the largest one included."""
    g = torch.Generator().manual_seed(1000 * P + L % 997 + (7 if null else 0) + (13 if wide else 0))
    px, py, z = _scatter(P, g)
    sc = _scene(px, py, z, g)
    if wide:
        L = 2 ** 31 - 1
    labels = torch.randint(0, L, (P,), generator=g, dtype=torch.int64)
    labels[torch.rand(P, generator=g) < 1.0 / 3.0] = -1
    labels[torch.randperm(P, generator=g)[:4]] = torch.tensor([L, L + 3, -2, -7])
    if wide:
        labels[torch.randperm(P, generator=g)[0]] = L - 1
    if null:
        labels = torch.full((P,), -1, dtype=torch.int64)
    return dict(sc=sc, cam=make_camera(W, H, F, F), labels=labels, L=int(L))


@functools.lru_cache(maxsize=None)
def capacity_case(n, stride):
    """n small Gaussians with pairwise distinct labels (a permutation times `stride`, plus 3) on a jittered 1-pixel grid inside
    tile (1, 0), in random depth order but for the highest label: more labels than table rows in ONE tile when n exceeds the tile capacity."""
    g = torch.Generator().manual_seed(50_000 + n)
    assert n <= 12 * 11
    cell = torch.randperm(12 * 11, generator=g)[:n]
    px = 18.5 + (cell % 12).to(torch.float32) + (torch.rand(n, generator=g) - 0.5) * 0.6
    py = 2.5 + (cell // 12).to(torch.float32) + (torch.rand(n, generator=g) - 0.5) * 0.6
    z = torch.rand(n, generator=g) * 8.0 + 2.0
    labels = torch.randperm(n, generator=g).to(torch.int64) * stride + 3
    # the highest label -- alone in the last sub-pass when n is one past a multiple of the capacity -- lies in front of the
    # others and is nearly opaque: it wins the pixels around its centre, so every sub-pass decides some pixel
    top = int(labels.argmax())
    z[top] = 1.9
    sc = _scene(px, py, z, g)
    sc.opacities[top] = 0.95
    return dict(sc=sc, cam=make_camera(W, H, F, F), labels=labels, L=int(labels.max()) + 1)


def capacity_counts(cap):
    """(n, stride): below, at, just above the capacity, and past twice the capacity with labels spread over several windows"""
    return [(cap - 1, 7), (cap, 7), (cap + 1, 7), (2 * cap + 1, 150)]


def all_cases(cap):
    """name -> case, every case of the suite"""
    out = {}
    for P in SCENE_PS:
        for L in SCENE_LS:
            out[f"P{P}_L{L}"] = scene_case(P, L)
    out["null"] = scene_case(300, 5, null=True)
    out["wide"] = scene_case(300, 0, wide=True)
    for n, stride in capacity_counts(cap):
        out[f"cap_{n}"] = capacity_case(n, stride)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_cached(name, cap):
    from tests import label_map_restatement as lr
    c = all_cases(cap)[name]
    used, Wl, alpha, binning = lr.label_weights(c["sc"], c["cam"], c["labels"].numpy(), c["L"])
    label, weight, second = lr.map_from_weights(used, Wl)
    for a in (used, Wl, alpha, label, weight, second):
        a.setflags(write=False)
    return dict(used=used, W=Wl, alpha=alpha, label=label, weight=weight, second=second, ranges=binning.ranges,
                decided=(weight - second) > np.float32(DECIDED))


def oracle(name, cap):
    """the restatement's maps of a case, computed once per process and read-only"""
    return _oracle_cached(name, int(cap))
