"""Restatement of the feature map (include/ogs_query.h: ogs_raster_feature_map) and of query.relevancy_maps, for the tests.

The map is the colour image of the project's own oracle (oracle.raster_oracle preprocess, bin_tiles, blend) run with
``feats = X[rows]`` (a zero row where the Gaussian's row is not counted) and a zero background, as
tests/label_map_restatement.py::label_weights does with one-hot columns: channel c of the blended image is the sum of
alpha_i * T_i * X[row(g_i), c] over the entries of the pixel.  ``dtype=torch.float64`` evaluates the oracle's differentiable
geometry (preprocess_t) and blend in float64 over the fp32 binning, ``torch.float32`` the same graph in fp32, skip decisions
included: what attributes a pixel to a threshold flip.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import label_votes_restatement as vr


def row_features(X, rows, P):
    """[P, D] float64: X[rows[g]] where the row lies in [0, R), zeros elsewhere; rows = None: X itself"""
    X = np.asarray(X, np.float64)
    if rows is None:
        assert X.shape[0] == P
        return X
    rows = np.asarray(rows, np.int64)
    ok = (rows >= 0) & (rows < X.shape[0])
    out = np.zeros((P, X.shape[1]), np.float64)
    out[ok] = X[rows[ok]]
    return out


def _geometry(sc, cam, dtype):
    """(xy, conic, opacity, depth) of the Gaussians some tile lists, in `dtype`, the binning with its list renumbered to them, and
    their indices"""
    from oracle import raster_oracle as ro
    W, H = cam.image_width, cam.image_height
    _, b = vr.binning_of(sc, cam)
    P = sc.means3D.shape[0]
    pl = np.asarray(b.point_list).astype(np.int64)
    used = np.unique(pl)                                   # culled rows never reach a list: keep their NaNs out
    remap = np.full(P, -1, np.int64)
    remap[used] = np.arange(len(used))
    t = lambda a: a[torch.as_tensor(used)].to(dtype)
    c = lambda a: a.to(dtype)
    xy, conic, op, _, depth = ro.preprocess_t(t(sc.means3D), torch.zeros(len(used), 3, dtype=dtype), t(sc.opacities),
                                              c(cam.world_view_transform), c(cam.full_proj_transform), c(cam.camera_center).reshape(3),
                                              W, H, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), t(sc.scales), t(sc.rotations),
                                              colors_precomp=torch.zeros(len(used), 1, dtype=dtype))
    return xy, conic, op, depth, b, remap[pl], used


def feature_image(sc, cam, X, rows=None, dtype=torch.float64):
    """(map [D, H, W], alpha [H, W]) float64 arrays"""
    from oracle import raster_oracle as ro
    W, H = cam.image_width, cam.image_height
    xy, conic, op, depth, b, pl, used = _geometry(sc, cam, dtype)
    feats = torch.as_tensor(row_features(X, rows, sc.means3D.shape[0])[used]).to(dtype)
    color, _, alpha, _ = ro.blend(xy, conic, op, feats, depth, b.ranges, pl, W, H, torch.zeros(feats.shape[1], dtype=dtype))
    return color.double().numpy(), alpha[0].double().numpy()


def tile_weights(sc, cam, dtype=torch.float64):
    """per tile: (ids [n] Gaussian indices in depth order, w [n, 16, 16] float64 blend weights alpha * T of every entry on every
    pixel of the tile, pixels outside the image included) -- the oracle's blend, one tile at a time"""
    xy, conic, op, depth, b, pl, used = _geometry(sc, cam, dtype)
    W = cam.image_width
    gx = (W + 15) // 16
    ranges = np.asarray(b.ranges).astype(np.int64)
    out = []
    for t in range(ranges.shape[0]):
        ids = torch.as_tensor(pl[ranges[t, 0]:ranges[t, 1]])
        ty, tx = divmod(t, gx)
        ax = torch.arange(16, dtype=dtype)
        X = (tx * 16 + ax)[None, :].expand(16, 16).reshape(-1)
        Y = (ty * 16 + ax)[:, None].expand(16, 16).reshape(-1)
        dx, dy = xy[ids, 0][:, None] - X[None], xy[ids, 1][:, None] - Y[None]
        power = -0.5 * (conic[ids, 0][:, None] * dx * dx + conic[ids, 2][:, None] * dy * dy) - conic[ids, 1][:, None] * dx * dy
        alpha = torch.clamp(op[ids][:, None] * torch.exp(torch.clamp(power, min=-80.0)), max=0.99)
        valid = (power <= 0) & (alpha >= 1.0 / 255.0)
        a = torch.where(valid, alpha, torch.zeros_like(alpha))
        Tincl = torch.cumprod(1.0 - a, dim=0)
        stopped = torch.cummax((valid & (Tincl < 1e-4)).to(torch.int8), dim=0)[0].bool() if len(ids) else valid
        Texcl = torch.cat([torch.ones_like(Tincl[:1]), Tincl[:-1]], dim=0)
        w = torch.where(valid & ~stopped, a * Texcl, torch.zeros_like(a))
        out.append((used[ids.numpy()], w.double().numpy().reshape(-1, 16, 16)))
    return out


def feature_image_by_loops(sc, cam, X, rows=None):
    """the same map from a direct per-pixel loop in float64: no matrix product, no oracle blend"""
    from oracle import raster_oracle as ro
    W, H = cam.image_width, cam.image_height
    P = sc.means3D.shape[0]
    feats = row_features(X, rows, P)
    _, b = vr.binning_of(sc, cam)
    d = lambda t: t.double()
    xy, conic, op, _, _ = ro.preprocess_t(d(sc.means3D), torch.zeros(P, 3, dtype=torch.float64), d(sc.opacities),
                                          d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center), W, H,
                                          math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), d(sc.scales), d(sc.rotations),
                                          colors_precomp=torch.zeros(P, 1, dtype=torch.float64))
    xy, conic, op = xy.numpy(), conic.numpy(), op.numpy()
    ranges, pl = np.asarray(b.ranges).astype(np.int64), np.asarray(b.point_list).astype(np.int64)
    out, alpha = np.zeros((feats.shape[1], H, W)), np.zeros((H, W))
    gx = (W + 15) // 16
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
                    a = min(0.99, op[i] * math.exp(power))
                    if a < 1.0 / 255.0:
                        continue
                    if T * (1 - a) < 1e-4:
                        break
                    out[:, py, px] += a * T * feats[i]
                    alpha[py, px] += a * T
                    T *= 1 - a
    return out, alpha


def relevancy_by_loops(fmap, text, canon=None):
    """[Q, H, W] float64 from a [D, H, W] map, one pixel at a time: cosine similarities with F.normalize's clamp at 1e-12 on
    both sides; with `canon`, min over the canonicals of softmax(10 * [sim_q, sim_k])[0]"""
    fmap, text = np.asarray(fmap, np.float64), np.asarray(text, np.float64)
    unit = lambda v: v / max(np.sqrt((v * v).sum()), 1e-12)
    D, H, W = fmap.shape
    out = np.zeros((text.shape[0], H, W))
    for y in range(H):
        for x in range(W):
            f = unit(fmap[:, y, x])
            sims = [float((unit(t) * f).sum()) for t in text]
            if canon is None:
                out[:, y, x] = sims
                continue
            neg = [float((unit(np.asarray(k, np.float64)) * f).sum()) for k in canon]
            for q, s in enumerate(sims):
                out[q, y, x] = min(math.exp(10 * s) / (math.exp(10 * s) + math.exp(10 * k)) for k in neg)
    return out
