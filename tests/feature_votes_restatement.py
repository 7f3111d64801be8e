"""Restatement of the feature votes (include/ogs_query.h: ogs_raster_feature_votes) and of query.features_from_votes, for the
tests.

The table is a gradient of the project's own oracle, as the label votes are (tests/label_votes_restatement.py): with colours
``zeros [P, D + 1]``, a zero background and the upstream colour gradient set to the planes v * F[c] (c < D) and v,
d(loss)/d(colour[g, c]) = sum over the pixels of v(p) * alpha * T of g's entry * F[c, p] -- float64 autograd through
oracle.raster_oracle (preprocess, bin_tiles, render_backward_f64).  ``dtype=torch.float32`` evaluates the same graph in fp32,
skip decisions included: what attributes a row to a threshold flip.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import label_votes_restatement as vr


def upstream_planes(features, valid):
    """[D + 1, H, W] float64: v * F[c] for c < D, then v; v = 1 where `valid` is None or non-zero"""
    F = np.asarray(features, np.float64)
    v = np.ones(F.shape[1:], np.float64) if valid is None else (np.asarray(valid) != 0).astype(np.float64)
    return np.concatenate([F * v[None], v[None]], axis=0)


def feature_table(sc, cam, features, valid=None, dtype=torch.float64):
    """[P, D + 1] float64 table of rows = None, in units of blend weight times feature"""
    from oracle import raster_oracle as ro
    W, H = cam.image_width, cam.image_height
    _, b = vr.binning_of(sc, cam)
    planes = upstream_planes(features, valid)
    zeros = np.zeros((1, H, W), np.float64)
    grads = ro.render_backward_f64(vr._inputs(sc, cam, planes.shape[0]), b, W, H, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5),
                                   np.zeros(planes.shape[0], np.float64), planes, zeros, zeros, dtype=dtype)
    return np.ascontiguousarray(grads["colors_precomp"], dtype=np.float64)


def feature_table_by_loops(sc, cam, features, valid=None):
    """the same table from a direct per-tile loop over the weights w = alpha * T in float64: no autograd, no upstream planes"""
    from oracle import raster_oracle as ro
    _, b = vr.binning_of(sc, cam)
    W, H = cam.image_width, cam.image_height
    F = np.asarray(features, np.float64)
    D = F.shape[0]
    ok = np.ones((H, W), bool) if valid is None else np.asarray(valid) != 0
    P = sc.means3D.shape[0]
    table = np.zeros((P, D + 1), np.float64)
    gx = (W + 15) // 16
    d = lambda t: t.double()
    xy, conic, op, _, _ = ro.preprocess_t(d(sc.means3D), torch.zeros(P, 3, dtype=torch.float64), d(sc.opacities),
                                          d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center), W, H,
                                          math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), d(sc.scales), d(sc.rotations),
                                          colors_precomp=torch.zeros(P, 1, dtype=torch.float64))
    xy, conic, op = xy.numpy(), conic.numpy(), op.numpy()
    ranges, pl = np.asarray(b.ranges).astype(np.int64), np.asarray(b.point_list).astype(np.int64)
    for t in range(ranges.shape[0]):
        ty, tx = divmod(t, gx)
        for py in range(ty * 16, min(ty * 16 + 16, H)):
            for px in range(tx * 16, min(tx * 16 + 16, W)):
                T = 1.0
                for i in pl[ranges[t, 0]:ranges[t, 1]]:
                    dx, dy = xy[i, 0] - px, xy[i, 1] - py
                    power = -0.5 * (conic[i, 0] * dx * dx + conic[i, 2] * dy * dy) - conic[i, 1] * dx * dy
                    if power > 0:
                        continue
                    alpha = min(0.99, op[i] * math.exp(power))
                    if alpha < 1.0 / 255.0:
                        continue
                    if T * (1 - alpha) < 1e-4:
                        break
                    if ok[py, px]:                      # valid gates the contribution only: the occlusion below is untouched
                        table[i, :D] += alpha * T * F[:, py, px]
                        table[i, D] += alpha * T
                    T *= 1 - alpha
    return table


def features_from_table(table, min_weight=0.0):
    """(feat [R, D], weight [R]) of a table [R, D + 1] in float64, one row at a time: sums / weight, zeros where the weight is
    not above `min_weight`"""
    table = np.asarray(table, np.float64)
    R, D = table.shape[0], table.shape[1] - 1
    feat, weight = np.zeros((R, D)), np.zeros(R)
    for r in range(R):
        weight[r] = table[r, D]
        if weight[r] > min_weight:
            feat[r] = table[r, :D] / weight[r]
    return feat, weight
