"""dev/bench helper: the stage-1 loss (train.py:450-456) on a 1080p feature map with 96 SAM-like masks:
mask_feature_mean + cohesion_loss + separation_loss forward and backward through the HIP segmented reductions --
first with the [N,H,W] mask stack (the dense kernels), then A-B in ONE process against the label image
(mask_ops.LabelMasks, the label kernels) on the same inputs, at N = 96, 32 and 200, the two paths alternating.
`--json PATH` also writes the A-B rows to a file.  `--variance` runs only the A-B of mask_feature_mean(return_var=True):
the variance from raw moments in one pass (ogs_*_feature_sums with_squares, as the binding had it) against the two-pass
form it takes now (sums, then ogs_*_feature_sqdev), error against the float64 oracle and ms per call."""
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


def one_pass_var(f, m):
    """(mean, variance, counts) as sum f^2 - 2 mean sum f + n mean^2 from ONE pass, through the C ABI's with_squares"""
    lib, ptr = _lib.lib(), _lib.ptr
    Cc, Hh, Ww = f.shape
    lab = isinstance(m, mk.LabelMasks)
    N = m.num_mask if lab else m.shape[0]
    table = torch.empty(N, mk.TABLE_STRIDE, device=f.device)
    call = lib.ogs_label_feature_sums if lab else lib.ogs_mask_feature_sums
    _lib.check(call(ptr(f), ptr(m.labels if lab else m.view(torch.uint8)), None, Cc, N, Hh * Ww, 1, ptr(table),
                    torch.cuda.current_stream().cuda_stream), "feature_sums")
    counts = table[:, Cc].clamp(min=1)
    mean = table[:, :Cc] / counts[:, None]
    var_c = (table[:, Cc + 1:2 * Cc + 1] - 2.0 * mean * table[:, :Cc] + table[:, Cc, None] * mean * mean) / counts[:, None]
    return mean, var_c.clamp_min(0).mean(dim=1), counts


def variance_ab():
    from oracle import mask_oracle as mo
    rows = []
    # accuracy: smooth features (a constant per channel + 0.05 of noise), one mask of 85 % of 360 x 640, one of 300 pixels
    g = torch.Generator().manual_seed(3601)
    f = torch.tensor([0.9, -0.8, 0.5, 0.7, -0.6, 0.3])[:, None, None] + 0.05 * torch.randn(6, 360, 640, generator=g)
    lab = torch.zeros(360, 640, dtype=torch.long); lab[:, :544] = 1; lab[100:115, 600:620] = 2
    stack = torch.stack([lab == 1, lab == 2, lab == 3])
    ref = mo.mask_feature_mean(f, stack, return_var=True, dtype=torch.float64)[1][:2]
    fd = f.to(dev)
    for name, m in (("stack", stack.to(dev)), ("labels", mk.LabelMasks(lab.to(dev), 3))):
        for form, fn in (("one_pass", one_pass_var), ("two_pass", lambda a, b: mk.mask_feature_mean(a, b, return_var=True))):
            errs = [((fn(fd, m)[1][:2].double().cpu() - ref).abs() / ref).tolist() for _ in range(8)]
            worst = [max(e[i] for e in errs) for i in range(2)]
            print(f"variance error vs float64, 360x640 smooth, {name:6s} {form}: 196 k pixel mask {worst[0]:.2e} "
                  f"(8 calls: {min(e[0] for e in errs):.2e} .. {worst[0]:.2e}), 300 pixel mask {worst[1]:.2e}", flush=True)
            rows.append({"what": "error", "masks": name, "form": form, "rel_err_large": [e[0] for e in errs],
                         "rel_err_small": [e[1] for e in errs]})
    # cost: 1080p, 96 masks, the two forms alternating
    feat, masks, lm, _ = inputs(96)
    feat = feat.detach()
    for name, m in (("stack", masks), ("labels", lm)):
        forms = {"one_pass": lambda m=m: one_pass_var(feat, m), "two_pass": lambda m=m: mk.mask_feature_mean(feat, m, return_var=True)}
        for fn in forms.values():
            for _ in range(5):
                fn()
        ms = {k: [] for k in forms}
        for _ in range(ROUNDS):
            for k, fn in forms.items():
                ms[k].append(timed(fn, 500) * 1e3)
        for k in forms:
            sp = spread(ms[k])
            print(f"return_var=True, {W}x{H}, 96 masks, {name:6s} {k}: {sp['median']:.3f} ms/call [{sp['min']:.3f}, {sp['max']:.3f}]", flush=True)
            rows.append({"what": "ms_per_call", "masks": name, "form": k, **sp})
    return rows


if "--variance" in sys.argv:
    rows = variance_ab()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump({"size": [W, H], "C": C, "rounds": ROUNDS, "calls_per_round": 500, "rows": rows}, fh, indent=1)
    sys.exit(0)

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
