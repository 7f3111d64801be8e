"""dev/bench helper: the stage-1 loss (train.py:450-456) on a 1080p feature map with 96 SAM-like masks:
mask_feature_mean + cohesion_loss + separation_loss forward and backward through the HIP segmented reductions --
first with the [N,H,W] mask stack (the dense kernels), then A-B in ONE process against the label image
(mask_ops.LabelMasks, the label kernels) on the same inputs, at N = 96, 32 and 200, the two paths alternating.
`--json PATH` also writes the A-B rows to a file."""
import json
import statistics
import sys, time
import torch
sys.path.insert(0, ".")
from opengaussian_amd import mask_ops as mk, _lib
dev = torch.device("cuda:0")
H, W, C = 1080, 1920, 6
ROUNDS = 5


def inputs(N):
    g = torch.Generator().manual_seed(0)
    feat = torch.rand(C, H, W, generator=g).to(dev).requires_grad_(True)
    coarse = torch.randint(0, N + 1, ((H + 31) // 32, (W + 31) // 32), generator=g)
    labels = coarse.repeat_interleave(32, 0).repeat_interleave(32, 1)[:H, :W].to(dev)
    masks = torch.stack([labels == (n + 1) for n in range(N)])            # [N,H,W] bool
    sil = torch.rand(1, H, W, generator=g).to(dev)
    return feat, masks, mk.LabelMasks(labels, N), sil


def make_step(feat, masks, sil):
    def step():
        feat.grad = None
        mean = mk.mask_feature_mean(feat, masks, image_mask=sil)
        loss = mk.separation_loss(mean, 1000) + 0.1 * mk.cohesion_loss(feat, masks, mean)
        loss.backward()
        return loss
    return step


def timed(step, K=50):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / K


def profiled(step, K=10):
    """{kernel base name: us per call} from the library's own per-launch events"""
    _lib.prof_enable(1)
    for _ in range(K):
        step()
    torch.cuda.synchronize()
    prof = _lib.prof_collect(); _lib.prof_enable(0)
    out = {}
    for k, v in prof.items():
        base = k.strip("()").split("<")[0]
        out[base] = out.get(base, 0.0) + v["total_ms"] / K * 1e3          # one call of each per step
    return out


def alg_bytes(N):
    stack = N * H * W; lab = 4 * H * W; fmap = C * H * W * 4; wmap = H * W * 4
    return {"mask_feature_sums_kernel": fmap + wmap + stack, "mask_feature_sums_backward_kernel": wmap + stack + fmap,
            "mask_cohesion_kernel": fmap + stack, "mask_cohesion_backward_kernel": 2 * fmap + stack,
            "label_feature_sums_kernel": fmap + wmap + lab, "label_feature_sums_backward_kernel": wmap + lab + fmap,
            "label_cohesion_kernel": fmap + lab, "label_cohesion_backward_kernel": 2 * fmap + lab}


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


N = 96
feat, masks, lm, sil = inputs(N)
step = make_step(feat, masks, sil)
for _ in range(5):
    step()
dt = timed(step)
print(f"stage-1 loss fwd+bwd, {W}x{H}, {N} masks: {dt * 1e3:.3f} ms/step", flush=True)
alg = alg_bytes(N)
for k, us in sorted(profiled(step).items(), key=lambda kv: -kv[1]):
    extra = f"  {alg[k] / us / 1e3:7.0f} GB/s algorithmic" if k in alg else ""
    print(f"  {k:50s} {us:8.1f} us{extra}", flush=True)

# ---- stack against labels, same process, same inputs, alternating -------------------------------------------------------
report = {"size": [W, H], "C": C, "rounds": ROUNDS, "steps_per_round": 50, "profiled_steps_per_round": 10, "rows": []}
for N in (96, 32, 200):
    if N != 96:
        del feat, masks, lm, sil
        feat, masks, lm, sil = inputs(N)
    steps = {"stack": make_step(feat, masks, sil), "labels": make_step(feat, lm, sil)}
    la, lb = float(steps["stack"]()), float(steps["labels"]())
    assert abs(la - lb) <= 2e-5 * abs(la), (la, lb)                   # same loss either way
    for s in steps.values():
        for _ in range(5):
            s()
    e2e = {m: [] for m in steps}
    kern = {m: {} for m in steps}
    for _ in range(ROUNDS):
        for m, s in steps.items():
            e2e[m].append(timed(s) * 1e3)
            for k, us in profiled(s).items():
                kern[m].setdefault(k, []).append(us)
    alg = alg_bytes(N)
    print(f"N = {N}: stage-1 loss fwd+bwd ms/step (median [min, max] of {ROUNDS} alternating rounds)", flush=True)
    for m in steps:
        sp = spread(e2e[m])
        print(f"  {m:7s} {sp['median']:.3f} [{sp['min']:.3f}, {sp['max']:.3f}]", flush=True)
        row = {"N": N, "masks": m, "step_ms": sp, "kernels_us": {}}
        for k, xs in sorted(kern[m].items()):
            sp = spread(xs)
            gbs = alg[k] / sp["median"] / 1e3 if k in alg else None
            row["kernels_us"][k] = dict(sp, alg_GBps=gbs)
            extra = f"  {gbs:7.0f} GB/s algorithmic" if gbs else ""
            print(f"    {k:46s} {sp['median']:7.1f} us [{sp['min']:.1f}, {sp['max']:.1f}]{extra}", flush=True)
        report["rows"].append(row)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
        json.dump(report, fh, indent=1)
