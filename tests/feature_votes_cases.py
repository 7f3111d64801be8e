"""Seeded feature images for the feature-votes tests over the scenes of tests/label_votes_cases.py (image 40 x 24: 3 x 2 tiles,
5 x 3 quadrants, the last tile column and row partial; `P300`, `P1500`, `wide`), at the smallest shapes at which the kernel can
go wrong.

A case is named ``<scene>_<channels>[_masked]`` with the channel count spelled in terms of the two hooks (`f-1`, `b`, `2b+1`, ...),
so that the names exist before the library is loaded.  Features: seeded standard normal fp32 [D, H, W].  `fold` is the number of
columns of one MFMA block of the kernel's fold, `block` the number of columns a wave holds per walk (the two hooks of the
library): D + 1 columns take ceil((D + 1) / block) walks, so D = block - 1 fills a walk exactly with the weight column last,
D = block puts the weight column alone into a second walk, and 2 block + 1 ends a third walk's first MFMA block after two
columns.  The mask: a checkerboard of 4 x 4 pixel blocks (every quadrant half valid) plus one fully invalid quadrant.
"""
from __future__ import annotations

import functools

import torch

from tests import label_votes_cases as vc

W, H = vc.W, vc.H
GRAD_BAR = vc.GRAD_BAR
LEAF_ROWS = vc.LEAF_ROWS


CHANNELS = ("1", "3", "f-1", "f", "f+1", "b-1", "b", "b+1", "2b+1")
# every channel count with and without the mask on P1500; the other two scenes at a small and a multi-walk count
CASE_NAMES = ([f"P1500_{d}{m}" for d in CHANNELS for m in ("", "_masked")]
              + [f"{s}_{d}{m}" for s in ("P300", "wide") for d in ("3", "b+1") for m in ("", "_masked")])


def channels_of(spec, fold, block):
    """'3' -> 3, 'f-1' -> fold - 1, '2b+1' -> 2 * block + 1"""
    if spec.isdigit():
        return int(spec)
    head, sign, tail = spec.partition("+") if "+" in spec else spec.partition("-")
    base = {"f": fold, "b": block, "2b": 2 * block}[head]
    return base + (int(tail) if sign == "+" else -int(tail) if sign == "-" else 0)


@functools.lru_cache(maxsize=None)
def valid_mask():
    """bool [H, W]: 4 x 4 checkerboard, the quadrant of tests/label_votes_cases.py's many-label cases fully invalid"""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    v = ((y // 4 + x // 4) % 2) == 0
    v[vc.QUAD_Y0:vc.QUAD_Y0 + 8, vc.QUAD_X0:vc.QUAD_X0 + 8] = False
    return v


@functools.lru_cache(maxsize=None)
def features(D, seed=0):
    """seeded standard normal fp32 [D, H, W]"""
    g = torch.Generator().manual_seed(31000 + 17 * D + seed)
    return torch.randn(D, H, W, generator=g, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def case(name, fold=16, block=32):
    """name -> dict(name, sc, cam, features [D, H, W] fp32, valid bool [H, W] or None, D)"""
    parts = name.split("_")
    sc, cam = vc.scene(parts[0])
    D = channels_of(parts[1], fold, block)
    masked = len(parts) > 2 and parts[2] == "masked"
    return dict(name=name, sc=sc, cam=cam, features=features(D), valid=valid_mask() if masked else None, D=D)


def _table(name, fold, block, dtype):
    from tests import feature_votes_restatement as fr
    c = case(name, fold, block)
    t = fr.feature_table(c["sc"], c["cam"], c["features"].numpy(), None if c["valid"] is None else c["valid"].numpy(), dtype=dtype)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def oracle(name, fold=16, block=32):
    """float64 restatement of a case (rows = None), computed once per process and read-only"""
    return _table(name, fold, block, torch.float64)


@functools.lru_cache(maxsize=None)
def oracle_fp32(name, fold=16, block=32):
    """the same graph evaluated in fp32: what attributes a threshold flip"""
    return _table(name, fold, block, torch.float32)
