"""NumPy restatement of the label map and of the click helpers (opengaussian_amd/query.py), for the tests.

The per-label weights W_l are the colour channels of the oracle's own pipeline (oracle.raster_oracle preprocess, bin_tiles, blend)
run with ONE-HOT features and a zero background: channel l of the blended image is the sum of alpha_i * T_i over the entries
whose Gaussian carries label l.  The one-hot columns are the labels the scene USES, ascending (a label nobody carries has W = 0
everywhere and can neither win nor be the runner-up), so "lowest column on a tie" is "lowest label on a tie".
The click helpers restate what scripts/render_by_click.py:35-66 and :143-161 compute, one click at a time.
"""
from __future__ import annotations

import math

import numpy as np
import torch


def label_weights(sc, cam, labels, num_labels):
    """(used [K] ascending labels in [0, num_labels) that some Gaussian carries, W [K, H, W] fp32, alpha [H, W] fp32, the
    oracle's binning)"""
    from oracle import raster_oracle as ro
    W, H = cam.image_width, cam.image_height
    labels = np.asarray(labels, np.int64)
    valid = (labels >= 0) & (labels < num_labels)
    used = np.unique(labels[valid])
    P = labels.shape[0]
    onehot = np.zeros((P, max(len(used), 1)), np.float32)
    onehot[np.nonzero(valid)[0], np.searchsorted(used, labels[valid])] = 1.0
    g = ro.preprocess(sc.means3D.numpy(), sc.opacities.numpy(), cam.world_view_transform.numpy(),
                      cam.full_proj_transform.numpy(), cam.camera_center.numpy(), W, H, math.tan(cam.FoVx * 0.5),
                      math.tan(cam.FoVy * 0.5), scales=sc.scales.numpy(), rotations=sc.rotations.numpy(), colors_precomp=onehot)
    b = ro.bin_tiles(g, W, H)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    color, _, alpha, _ = ro.blend(t(g.xy), t(g.conic), t(g.opacity), t(onehot), t(g.depth), b.ranges, b.point_list, W, H,
                                  torch.zeros(onehot.shape[1]))
    Wl = color.numpy().astype(np.float32)
    if len(used) == 0:
        Wl = Wl[:0]
    return used, Wl, alpha[0].numpy().astype(np.float32), b


def map_from_weights(used, Wl):
    """(label [H, W] int32, weight, second [H, W] fp32) from W [K, H, W]: the largest W_l > 0, lowest label on a tie, -1 / 0
    where nothing labelled contributes; second = the largest weight of any OTHER label (0 if there is none)"""
    K, H, W = Wl.shape
    label = np.full((H, W), -1, np.int32)
    weight = np.zeros((H, W), np.float32)
    second = np.zeros((H, W), np.float32)
    if K == 0:
        return label, weight, second
    arg = Wl.argmax(0)                                   # first maximum: lowest label
    top = np.take_along_axis(Wl, arg[None], 0)[0]
    won = top > 0
    label[won] = used[arg[won]].astype(np.int32)
    weight[won] = top[won]
    if K > 1:
        rest = Wl.copy()
        np.put_along_axis(rest, arg[None], -1.0, 0)
        second = np.maximum(rest.max(0), 0.0).astype(np.float32)
        second[~won] = 0.0
    return label, weight, second


def labels_at_pixels(label, weight, pixels_xy, radius=0):
    """per click: the label with the largest summed weight over the window clamped to the image, lowest label on a tie, -1 when
    the window holds none"""
    H, W = label.shape
    out = []
    for x, y in np.asarray(pixels_xy, np.int64):
        left, right = max(x - radius, 0), min(x + radius + 1, W)
        top, bottom = max(y - radius, 0), min(y + radius + 1, H)
        sums = {}
        for xx in range(left, right):
            for yy in range(top, bottom):
                l = int(label[yy, xx])
                if l >= 0:
                    sums[l] = np.float32(sums.get(l, np.float32(0)) + np.float32(weight[yy, xx]))
        best = -1
        for l in sorted(sums):
            if best < 0 or sums[l] > sums[best]:
                best = l
        out.append(best)
    return np.array(out, np.int64)


def click_features(ins_feat_map, pixels_xy, radius=5, quantize=True):
    """What the reference's click reads (render_by_click.py:35-53, :61): the feature map as the 8-bit image save_image writes
    (x * 255 + 0.5, clamped to [0, 255], truncated), its mean over the window cut at the image border in float64, that mean as
    an fp32 tensor divided by 255, doubled, minus one.  Without `quantize`: the mean of the map itself, doubled, minus one."""
    m = np.asarray(ins_feat_map, np.float32)
    C, H, W = m.shape
    img = np.clip(m * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8) if quantize else m
    rows = []
    for cx, cy in np.asarray(pixels_xy, np.int64):
        x0, x1 = max(cx - radius, 0), min(cx + radius + 1, W)
        y0, y1 = max(cy - radius, 0), min(cy + radius + 1, H)
        window = img[:, y0:y1, x0:x1].reshape(C, -1).astype(np.float64)
        val = torch.tensor([float(v) for v in window.mean(axis=1)])            # python floats -> an fp32 tensor, as the reference
        rows.append(((val / 255) * 2 - 1 if quantize else val * 2 - 1).numpy())
    return np.stack(rows).astype(np.float32)


def select_leaves_by_click(root_feats, leaf_feats, root_centers, leaf_centers):
    """Option (2) of the reference's click selection (render_by_click.py:143-161), one click at a time: fp32 Euclidean distances
    to the root centres without their last three columns and to the leaf centres without the last row, 999 for a leaf whose row
    sums to zero, the nearest root r, then the nearest leaf among [int(r * n), int((r + 1) * n)) with n = leaves / roots."""
    roots = torch.as_tensor(root_centers)[:, :-3]
    leaves = torch.as_tensor(leaf_centers)[:-1]
    per_root = leaves.shape[0] / roots.shape[0]
    picked = []
    for rv, lv in zip(torch.as_tensor(root_feats), torch.as_tensor(leaf_feats)):
        d_leaf = (lv - leaves).norm(dim=1)
        d_leaf[leaves.sum(-1) == 0] = 999
        r = int((rv - roots).norm(dim=1).argmin())
        lo, hi = int(r * per_root), int((r + 1) * per_root)
        picked.append(lo + int(d_leaf[lo:hi].argmin()))
    return np.array(picked, np.int64)
