"""Which lists of a bench workload does the one-wave depth sort rank inside buckets, and which take the LSD passes?

Applies the kernel's digit rule (binning.hip::wave_bucket_rank) on the host to the exported binning of a default pass: for every
tile list of 2 .. capacity(0) entries the digit is (key - smallest key) >> shift, the shift that leaves 8 bits of the list's key
range (the ids' when the list has one key); a list whose largest bucket holds more than capacity(2) entries falls back.  Prints one JSON line per workload:
list counts by path, the fallback count, and the distribution of the largest bucket.

usage: python scripts/tile_sort_bucket_stats.py [workload ...]      (default: S1M-1080p C3-500k-988 C2-100k-800 C4-2M-648)"""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import WORKLOADS  # noqa: E402
from opengaussian_amd import _lib  # noqa: E402
from opengaussian_amd.rasterizer import GaussianRasterizationSettings, rasterize_fused  # noqa: E402
from opengaussian_amd.synthetic import make_scene, orbit_camera  # noqa: E402
from tests import helpers  # noqa: E402

BUCKET_BITS = 8


def largest_bucket(words):
    lo, hi = int(words.min()), int(words.max())
    if lo == hi:
        return None
    shift = max(0, (hi - lo).bit_length() - BUCKET_BITS)
    digit = (words.astype(np.int64) - lo) >> shift
    return int(np.bincount(digit, minlength=1 << BUCKET_BITS).max()), (hi - lo).bit_length()


def stats(workload, dev, view):
    wl = WORKLOADS[workload]
    P, W, H, f = wl["P"], wl["W"], wl["H"], wl["f"]
    sc = make_scene(P, W, H, f, f, seed=0).to(dev)
    cam = orbit_camera(W, H, f, f, view_index=view, num_views=8).to(dev)
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=3, campos=cam.camera_center, prefiltered=False, debug=False)
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    color, radii, depth, alpha = rasterize_fused(sc.means3D, m2, sc.opacities, sc.shs, sc.ins_feat, rs, scales=sc.scales,
                                                 rotations=sc.rotations)
    ctx = color.grad_fn
    (_m3, _shs, _cols, _op, _scl, _rot, _cov, _bg, _v, _p, _cp, _radii, _alpha, geom, image, point_list, sorted_rec,
     quad_list) = ctx.saved_tensors
    a = _lib.OgsRasterFwdArgs()
    a.P, a.W, a.H, a.C = ctx.P, W, H, ctx.Cn
    a.geom_buffer, a.image_buffer, a.point_list = _lib.ptr(geom), _lib.ptr(image), _lib.ptr(point_list)
    a.sorted_rec, a.quad_list = _lib.ptr(sorted_rec), _lib.ptr(quad_list)
    keys, ranges, ncontrib, raw = helpers._export_binning_of(a, ctx.num_rendered, point_list, W, H, dev)
    lib = _lib.lib()
    wave, block, cap = (int(lib.ogs_raster_tile_sort_capacity(l)) for l in (0, 1, 2))
    depth_bits = (np.asarray(keys, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ids = (np.asarray(raw, dtype=np.uint32) & np.uint32(0x7FFFFFFF))
    lens = ranges[:, 1].astype(np.int64) - ranges[:, 0].astype(np.int64)
    big, spans, by_id = [], [], 0
    for t in np.nonzero((lens >= 2) & (lens <= wave))[0]:
        r0, r1 = int(ranges[t, 0]), int(ranges[t, 1])
        lb = largest_bucket(depth_bits[r0:r1])
        if lb is None:
            by_id += 1
            lb = largest_bucket(ids[r0:r1])
        big.append(lb[0]); spans.append(lb[1])
    big, spans = np.asarray(big), np.asarray(spans)
    pct = lambda q: float(np.percentile(big, q)) if len(big) else 0.0
    return {"workload": workload, "view": view, "tiles": int(len(lens)), "bucket_cap": cap,
            "lists_short": int((lens < 2).sum()), "lists_one_wave": int(len(big)),
            "lists_four_waves_lds": int(((lens > wave) & (lens <= block)).sum()), "lists_global": int((lens > block).sum()),
            "one_wave_mean_len": float(lens[(lens >= 2) & (lens <= wave)].mean()) if len(big) else 0.0,
            "one_wave_one_key_lists": by_id, "one_wave_fallback_lists": int((big > cap).sum()),
            "largest_bucket": {"mean": float(big.mean()) if len(big) else 0.0, "p50": pct(50), "p90": pct(90), "p99": pct(99),
                               "max": int(big.max()) if len(big) else 0},
            "lists_with_largest_bucket_above": {str(c): int((big > c).sum()) for c in (8, 16, 32, 64, 128, 256)},
            "key_range_bits": {"mean": float(spans.mean()) if len(big) else 0.0, "max": int(spans.max()) if len(big) else 0}}


def main():
    dev = torch.device("cuda:0")
    names = sys.argv[1:] or ["S1M-1080p", "C3-500k-988", "C2-100k-800", "C4-2M-648"]
    for n in names:
        for view in (0, 3):
            print(json.dumps(stats(n, dev, view)), flush=True)


if __name__ == "__main__":
    main()
