"""Seeded feature tables for the feature-map tests over the scenes of tests/label_votes_cases.py (image 40 x 24: 3 x 2 tiles,
5 x 3 quadrants, the last tile column and row partial; `P300`, `P1500`, `wide`), at the smallest shapes at which the kernel can
go wrong, and of `odd`: the P300 Gaussians seen by a 37 x 21 camera, so that the last quadrant column and row are cut inside a
quadrant (5 of 8 pixels) and neither W nor H * W is a multiple of four (the planar stores take their 4-byte form).

A case is named ``<scene>_<channels>[_rows]`` with the channel count spelled in terms of the two hooks (`f-1`, `b`, `2b+1`, ...),
so that the names exist before the library is loaded.  `fold` is the number of columns of one MFMA block, `block` the number of
columns a wave accumulates per walk (the two hooks of the library): D columns take ceil(D / block) walks, so D = block fills a
walk exactly, block + 1 puts one column alone into a second walk, and 2 block + 1 ends a third walk's first MFMA block after one
column.  Features: seeded standard normal fp32 [R, D]; R = P without rows, else the 7 leaf-like rows of
label_votes_cases.leaf_rows (a tenth -1, a few >= R, one 2^40).
"""
from __future__ import annotations

import functools

import torch

from tests import label_votes_cases as vc

W, H = vc.W, vc.H
LEAF_ROWS = vc.LEAF_ROWS
GRAD_BAR = vc.GRAD_BAR
MAP_BAR = 1e-4             # the project's image bar of a forward pass, relative to the map's largest magnitude

# 2f / 2f+1: two whole MFMA blocks of a walk, and one column into the third
CHANNELS = ("1", "3", "f-1", "f", "f+1", "2f", "2f+1", "b-1", "b", "b+1", "2b+1")
# every channel count with and without rows on P1500; the other two scenes at a small and a multi-walk count
SCENES = ("P300", "P1500", "wide", "odd")
CASE_NAMES = ([f"P1500_{d}{r}" for d in CHANNELS for r in ("", "_rows")]
              + [f"{s}_{d}{r}" for s in ("P300", "wide", "odd") for d in ("3", "b+1") for r in ("", "_rows")])
ODD_W, ODD_H = 37, 21


@functools.lru_cache(maxsize=None)
def scene(name):
    """'P300', 'P1500', 'wide' (tests/label_votes_cases.py) or 'odd' -> (Scene, camera)"""
    if name != "odd":
        return vc.scene(name)
    from opengaussian_amd.synthetic import make_camera
    return vc.scene("P300")[0], make_camera(ODD_W, ODD_H, vc.F, vc.F)


def channels_of(spec, fold, block):
    """'3' -> 3, 'f-1' -> fold - 1, '2b+1' -> 2 * block + 1"""
    if spec.isdigit():
        return int(spec)
    head, sign, tail = spec.partition("+") if "+" in spec else spec.partition("-")
    base = {"f": fold, "2f": 2 * fold, "b": block, "2b": 2 * block}[head]
    return base + (int(tail) if sign == "+" else -int(tail) if sign == "-" else 0)


@functools.lru_cache(maxsize=None)
def features(R, D, seed=0):
    """seeded standard normal fp32 [R, D]"""
    g = torch.Generator().manual_seed(47000 + 13 * D + 7 * R + seed)
    return torch.randn(R, D, generator=g, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def upstream(D, seed=0, H=H, W=W):
    """seeded standard normal fp32 [D, H, W]: an upstream gradient, the F of the adjoint identity"""
    g = torch.Generator().manual_seed(53000 + 11 * D + seed + 3 * W)
    return torch.randn(D, H, W, generator=g, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def case(name, fold=16, block=32):
    """name -> dict(name, sc, cam, D, R, features [R, D] fp32, rows int64 [P] or None)"""
    parts = name.split("_")
    sc, cam = scene(parts[0])
    D = channels_of(parts[1], fold, block)
    P = sc.means3D.shape[0]
    by_rows = len(parts) > 2 and parts[2] == "rows"
    R = LEAF_ROWS if by_rows else P
    return dict(name=name, scene=parts[0], sc=sc, cam=cam, W=cam.image_width, H=cam.image_height, D=D, R=R, P=P, features=features(R, D), rows=vc.leaf_rows(P) if by_rows else None)


def _image(name, fold, block, dtype):
    from tests import feature_map_restatement as mr
    c = case(name, fold, block)
    m, a = mr.feature_image(c["sc"], c["cam"], c["features"].numpy(), None if c["rows"] is None else c["rows"].numpy(), dtype=dtype)
    m.setflags(write=False)
    a.setflags(write=False)
    return m, a


@functools.lru_cache(maxsize=None)
def oracle(name, fold=16, block=32):
    """(map [D, H, W], alpha [H, W]) of the float64 restatement, computed once per process and read-only"""
    return _image(name, fold, block, torch.float64)


@functools.lru_cache(maxsize=None)
def oracle_fp32(name, fold=16, block=32):
    """the same graph evaluated in fp32: what attributes a threshold flip"""
    return _image(name, fold, block, torch.float32)
