"""Restatement of the label votes (include/ogs_query.h: ogs_raster_label_votes) and of the table helpers of
opengaussian_amd/query.py, for the tests.

The table is a gradient of the project's own oracle: with colours ``zeros [P, L + 1]``, a zero background and the upstream colour
gradient set to the one-hot planes of lab(p), d(loss)/d(colour[g, l]) = sum over the pixels with lab(p) = l of alpha * T of g's
entry -- float64 autograd through oracle.raster_oracle (preprocess, bin_tiles, render_backward_f64).  ``dtype=torch.float32``
evaluates the same graph in fp32, skip decisions included: what attributes a row to a threshold flip.
"""
from __future__ import annotations

import math

import numpy as np
import torch


def _inputs(sc, cam, channels):
    P = sc.means3D.shape[0]
    return dict(means3D=sc.means3D.numpy(), opacities=sc.opacities.numpy(), viewmatrix=cam.world_view_transform.numpy(),
                projmatrix=cam.full_proj_transform.numpy(), campos=cam.camera_center.numpy(), scales=sc.scales.numpy(),
                rotations=sc.rotations.numpy(), colors_precomp=np.zeros((P, channels), np.float32))


def binning_of(sc, cam):
    """(geometry, binning) of the oracle's fp32 pipeline"""
    from oracle import raster_oracle as ro
    W, H = cam.image_width, cam.image_height
    g = ro.preprocess(sc.means3D.numpy(), sc.opacities.numpy(), cam.world_view_transform.numpy(), cam.full_proj_transform.numpy(),
                      cam.camera_center.numpy(), W, H, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5),
                      scales=sc.scales.numpy(), rotations=sc.rotations.numpy(),
                      colors_precomp=np.zeros((sc.means3D.shape[0], 1), np.float32))
    return g, ro.bin_tiles(g, W, H)


def one_hot_planes(pixel_labels, L):
    """[L + 1, H, W] float64: plane l is 1 where lab(p) = l; lab(p) = the pixel's value inside [0, L), else L"""
    img = np.asarray(pixel_labels, np.int64)
    lab = np.where((img >= 0) & (img < L), img, L)
    planes = np.zeros((L + 1,) + img.shape, np.float64)
    np.put_along_axis(planes, lab[None], 1.0, 0)
    return planes


def vote_table(sc, cam, pixel_labels, L, dtype=torch.float64):
    """[P, L + 1] float64 table of rows = None, in units of blend weight"""
    from oracle import raster_oracle as ro
    W, H = cam.image_width, cam.image_height
    _, b = binning_of(sc, cam)
    zeros = np.zeros((1, H, W), np.float64)
    grads = ro.render_backward_f64(_inputs(sc, cam, L + 1), b, W, H, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5),
                                   np.zeros(L + 1, np.float64), one_hot_planes(pixel_labels, L), zeros, zeros, dtype=dtype)
    return np.ascontiguousarray(grads["colors_precomp"], dtype=np.float64)


def vote_table_by_loops(sc, cam, pixel_labels, L):
    """the same table from a direct per-tile loop over the weights w = alpha * T in float64: no autograd, no one-hot planes"""
    from oracle import raster_oracle as ro
    _, b = binning_of(sc, cam)
    W, H = cam.image_width, cam.image_height
    img = np.asarray(pixel_labels, np.int64)
    lab = np.where((img >= 0) & (img < L), img, L)
    P = sc.means3D.shape[0]
    table = np.zeros((P, L + 1), np.float64)
    gx = (W + 15) // 16
    # the geometry in float64 from the fp32 inputs, as the autograd route computes it; rows the binning never lists may be NaN
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
                    table[i, lab[py, px]] += alpha * T
                    T *= 1 - alpha
    return table


def rows_table(table, rows, R):
    """index_add of a rows = None table over `rows`; a row outside [0, R) is dropped"""
    rows = np.asarray(rows, np.int64)
    out = np.zeros((R,) + table.shape[1:], table.dtype)
    ok = (rows >= 0) & (rows < R)
    np.add.at(out, rows[ok], table[ok])
    return out


def labels_from_votes(table, min_weight=0.0, min_share=0.0):
    """(label, weight, second, total) per row of a table [R, L + 1] (any numeric dtype, one row at a time): the largest of the
    columns 0..L-1, the lowest label on an exact tie, -1 without labelled weight or below a threshold; total includes column L"""
    table = np.asarray(table)
    R, L = table.shape[0], table.shape[1] - 1
    label, weight, second, total = np.full(R, -1, np.int64), np.zeros(R), np.zeros(R), np.zeros(R)
    for r in range(R):
        total[r] = float(table[r].sum())
        best = -1
        for l in range(L):
            if table[r, l] > 0 and (best < 0 or table[r, l] > table[r, best]):
                best = l
        if best < 0:
            continue
        weight[r] = float(table[r, best])
        others = [float(table[r, l]) for l in range(L) if l != best]
        second[r] = max(others + [0.0])
        if weight[r] >= min_weight and weight[r] / total[r] >= min_share:
            label[r] = best
    return label, weight, second, total
