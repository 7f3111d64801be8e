"""What a trainable camera costs: forward + backward of one pass with the camera's tensors requiring grad (the two launches of
csrc/pose_bwd.hip behind the backward) against the route a user had before -- the se(3) delta applied to the scene in torch.

  python scripts/pose_grad_bench.py [--iters 40] [--repeats 3] [--warmup 8] [--sizes S1M,C4] [--out profiles/pose_grad_bench.json]
                                    [--parent-tree DIR [--bench-steps 60 --bench-warmup 10]]

Sizes: S1M (1 M Gaussians, 1920 x 1080) and C4-class (2 M, 648 x 484) as bench.py builds them, SH degree 3, one camera.  Legs,
alternating in one process after a warm-up of all three, each --iters passes between two device events (the second one waited
for), the triple repeated --repeats times, every repeat in the file:
  (0) forward + backward with every per-Gaussian input requiring grad and a constant camera: today's step;
  (a) the same with the camera a pose.CameraPose whose delta requires grad;
  (b) the same gradients of the same six numbers without the feature: T = C2W exp(delta) W2C applied to means3D [P, 3] and
      composed with rotations [P, 4] in torch, autograd back through them, the camera constant.
Recorded besides: the times of the two pose kernels and of preprocess_backward from the library's own per-kernel events
(ogs_prof_*, a run of its own), and whether (a) - (0) < (b) - (0) holds in every repeat.
--parent-tree DIR: a built checkout of the parent commit.  `bench.py --gpus 1` runs there and here alternately, three times each,
in fresh processes; every repeat of this build must be no slower than the parent's slowest repeat plus the parent's own
max - min.  Both sets go into the file.  Nothing is measured without a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opengaussian_amd import _lib  # noqa: E402
from opengaussian_amd.pose import CameraPose, se3_exp  # noqa: E402
from opengaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from opengaussian_amd.synthetic import make_camera, make_scene  # noqa: E402

# name -> (W, H, Gaussians, focal): bench.py's S1M-1080p and C4-2M-648
SIZES = {"S1M": (1920, 1080, 1_000_000, 1000.0), "C4": (648, 484, 2_000_000, 500.0), "toy": (160, 120, 20_000, 120.0)}


def settings(cam, bg):
    import math
    return GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=3, campos=cam.camera_center, prefiltered=False, debug=False)


def quat_of_near_identity(Rm):
    w = torch.sqrt(1.0 + Rm[0, 0] + Rm[1, 1] + Rm[2, 2]) / 2
    return torch.stack([w, (Rm[2, 1] - Rm[1, 2]) / (4 * w), (Rm[0, 2] - Rm[2, 0]) / (4 * w), (Rm[1, 0] - Rm[0, 1]) / (4 * w)])


def quat_mul(a, b):
    ar, ax, ay, az = a
    br, bx, by, bz = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return torch.stack([ar * br - ax * bx - ay * by - az * bz, ar * bx + ax * br + ay * bz - az * by,
                        ar * by - ax * bz + ay * br + az * bx, ar * bz + ax * by - ay * bx + az * br], dim=1)


def make_legs(sc, cam, dev):
    leaf = lambda t: t.to(dev).contiguous().requires_grad_(True)
    L = {k: leaf(getattr(sc, k)) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    m2 = torch.zeros_like(L["means3D"])
    bg = torch.zeros(3, device=dev)
    gen = torch.Generator().manual_seed(0)
    gC = torch.randn(3, cam.image_height, cam.image_width, generator=gen).to(dev)
    pose = CameraPose(cam)
    delta_b = torch.zeros(6, device=dev, requires_grad=True)
    W2C = cam.world_view_transform.t().contiguous()
    C2W = torch.linalg.inv(W2C.double().cpu()).float().to(dev)

    def zero():
        for t in L.values():
            t.grad = None
        pose.delta.grad = None
        delta_b.grad = None

    def run(cam_like, means, rots):
        out = GaussianRasterizer(settings(cam_like, bg))(means3D=means, means2D=m2, opacities=L["opacities"], shs=L["shs"],
                                                         scales=L["scales"], rotations=rots)
        (out[0] * gC).sum().backward()

    def leg0():
        zero()
        run(cam, L["means3D"], L["rotations"])

    def leg_a():
        zero()
        run(pose, L["means3D"], L["rotations"])

    def leg_b():
        zero()
        T = C2W @ se3_exp(delta_b) @ W2C
        run(cam, L["means3D"] @ T[:3, :3].t() + T[:3, 3][None], quat_mul(quat_of_near_identity(T[:3, :3]), L["rotations"]))

    return {"0": leg0, "a": leg_a, "b": leg_b}, pose, delta_b


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def kernel_times(fn, steps):
    _lib.prof_enable(1)
    try:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        prof = _lib.prof_collect()
    finally:
        _lib.prof_enable(0)
    pick = lambda prefix: round(sum(v["total_ms"] for k, v in prof.items() if k.startswith(prefix)) / steps, 4)
    return {"pose_partials_kernel_ms": pick("pose_partials_kernel"), "pose_fold_kernel_ms": pick("pose_fold_kernel"),
            "preprocess_backward_kernel_ms": pick("preprocess_backward_kernel"),
            "blend_backward_kernel_ms": pick("blend_backward_kernel")}


def bench_ab(parent_tree, steps, warmup, repeats=3):
    """bench.py in fresh processes, the parent's tree and this one alternately"""
    def one(tree):
        env = {k: v for k, v in os.environ.items() if k != "OGS_LIB_PATH"}
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                           env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"bench.py failed in {tree}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        return json.loads(line)
    runs = {"parent": [], "this": []}
    for _ in range(repeats):
        runs["parent"].append(one(parent_tree))
        runs["this"].append(one(ROOT))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--sizes", default="S1M,C4")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--bench-steps", type=int, default=60)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_grad_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_grad_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "ogs_version": int(_lib.lib().ogs_version()), "iters_per_leg": args.iters,
              "repeats": args.repeats, "legs": {"0": "constant camera", "a": "CameraPose delta requires grad",
                                               "b": "se(3) delta applied to means3D and rotations in torch"}, "sizes": []}
    for name in args.sizes.split(","):
        W, H, P, f = SIZES[name]
        sc = make_scene(P, W, H, f, f, seed=0)
        cam = make_camera(W, H, f, f).to(dev)
        legs, pose, delta_b = make_legs(sc, cam, dev)
        for _ in range(args.warmup):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        # the two routes compute the same six numbers (the SH view-direction term apart, which the moved scene does not model)
        legs["a"](); ga = pose.delta.grad.clone()
        legs["b"](); gb = delta_b.grad.clone()
        times = {k: [] for k in legs}
        for _ in range(args.repeats):
            for k, fn in legs.items():
                times[k].append(timed(fn, args.iters))
        med = lambda v: sorted(v)[len(v) // 2]
        extra_a = [a - z for a, z in zip(times["a"], times["0"])]
        extra_b = [b - z for b, z in zip(times["b"], times["0"])]
        entry = {"size": name, "W": W, "H": H, "gaussians": P,
                 "ms_per_pass": {k: [round(v, 4) for v in t] for k, t in times.items()},
                 "ms_median": {k: round(med(t), 4) for k, t in times.items()},
                 "ms_spread": {k: [round(min(t), 4), round(max(t), 4)] for k, t in times.items()},
                 "a_minus_0_ms": [round(v, 4) for v in extra_a], "b_minus_0_ms": [round(v, 4) for v in extra_b],
                 "a_cheaper_than_b_in_every_repeat": bool(all(a < b for a, b in zip(extra_a, extra_b))),
                 "delta_grad_pose_kernels": [float(v) for v in ga], "delta_grad_moved_scene": [float(v) for v in gb],
                 "kernels_ms_per_pass_leg_a": kernel_times(legs["a"], 8)}
        result["sizes"].append(entry)
        print(json.dumps(entry), flush=True)
        del legs, pose, delta_b, sc
        torch.cuda.empty_cache()
    if args.parent_tree:
        runs = bench_ab(os.path.abspath(args.parent_tree), args.bench_steps, args.bench_warmup)
        key = "ms_per_step" if "ms_per_step" in runs["this"][0] else None
        result["bench_ab"] = {"steps": args.bench_steps, "warmup": args.bench_warmup, **runs}
        if key:
            par = [r[key] for r in runs["parent"]]
            limit = max(par) + (max(par) - min(par))
            result["bench_ab"]["limit_ms_per_step"] = limit
            result["bench_ab"]["every_repeat_within_limit"] = bool(all(r[key] <= limit for r in runs["this"]))
        print(json.dumps({k: v for k, v in result["bench_ab"].items() if k not in ("parent", "this")}), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("written:", args.out)


if __name__ == "__main__":
    main()
