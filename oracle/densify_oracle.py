"""CPU restatement of the reference's densification bookkeeping -- TEST INFRASTRUCTURE ONLY.

Only tests/ and tests/golden/ may import this module; the product path (opengaussian_amd/densify.py ->
include/ogs_optim.h) never does.

PINNED: tests/test_oracle_densify.py holds every function below to the vectors produced by running the reference's
own GaussianModel methods (tests/golden/make_densify_golden.py, make_densify_edges_golden.py).  With that it is
the reference for state that only exists at run time (chained densification rounds on the device).

The restatement is written from the algorithm (scene/gaussian_model.py:300-303,372-514, train.py:597-598), not
from the reference's tensor surgery: one table of working rows (parent, kind, sample, scaling, opacity) goes
through the three stages -- append clones, append two children per split parent and drop the parents, final
prune -- and every tensor is gathered once at the end.  It is NOT the device's one-pass formulation either (that
decides per old row and scans); agreement of the two is what the GPU tests check.

A `state` is a dict of CPU tensors:
    params, exp_avg, exp_avg_sq : {group name: [N, ...] fp32}
    accum [N,1], denom [N,1], max_radii2D [N]
Functions return a NEW state (inputs are left untouched) plus, where rows move, the row map `src` (int64, the
row of the input each output row comes from) and `kind` (uint8: 0 old row, 1 clone, 2 / 3 first / second split
child), in the reference's order [surviving old rows | clones | first children | second children].
"""
import torch

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "ins_feat")


def _gather(state, src, kind):
    """every tensor through the row map; new rows (kind != 0) get zero moments"""
    old = (kind == 0)
    out = {"params": {}, "exp_avg": {}, "exp_avg_sq": {}}
    for n, p in state["params"].items():
        out["params"][n] = p[src].clone()
        w = old.reshape(-1, *([1] * (p.dim() - 1))).to(p.dtype)
        for m in ("exp_avg", "exp_avg_sq"):
            out[m][n] = state[m][n][src] * w
    return out


def rotation_matrices(q):
    """unit-normalised (r, x, y, z) quaternions [M,4] -> rotation matrices [M,3,3]"""
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1)
    return R.reshape(-1, 3, 3)


def prune_points(state, mask):
    """remove the rows where `mask` is set (bool or integer), statistics included"""
    src = torch.nonzero(mask.reshape(-1) == 0).flatten()
    kind = torch.zeros(len(src), dtype=torch.uint8)
    out = _gather(state, src, kind)
    out["accum"], out["denom"], out["max_radii2D"] = state["accum"][src].clone(), state["denom"][src].clone(), state["max_radii2D"][src].clone()
    return out, src, kind


def add_densification_stats(state, viewspace_grad, update_filter=None, radii=None):
    """accum += |grad[:, :2]|, denom += 1 on the visible rows; with `radii` also max_radii2D = max(., radii) there.
    update_filter None: visible = radii > 0."""
    vis = (radii > 0) if update_filter is None else update_filter.reshape(-1).bool()
    out = dict(state)
    norm = torch.norm(viewspace_grad[:, :2].float(), dim=-1, keepdim=True)
    out["accum"] = torch.where(vis[:, None], state["accum"] + norm, state["accum"])
    out["denom"] = torch.where(vis[:, None], state["denom"] + 1, state["denom"])
    if radii is not None:
        out["max_radii2D"] = torch.where(vis, torch.maximum(state["max_radii2D"], radii.to(state["max_radii2D"].dtype)), state["max_radii2D"])
    return out


def reset_opacity(state):
    """opacity <- logit(min(sigmoid(opacity), 0.01)), its moments zeroed"""
    out = {k: (dict(v) if isinstance(v, dict) else v) for k, v in state.items()}
    a = torch.sigmoid(state["params"]["opacity"])
    a = torch.min(a, torch.ones_like(a) * 0.01)
    out["params"]["opacity"] = torch.log(a / (1 - a))
    out["exp_avg"]["opacity"] = torch.zeros_like(a)
    out["exp_avg_sq"]["opacity"] = torch.zeros_like(a)
    return out


def densify_and_prune(state, max_grad, min_opacity, extent, max_screen_size, percent_dense, samples):
    """clone, split (two children per parent, offsets `samples` [2S,3]: rows [0,S) first copies, [S,2S) second), final
    prune.  Returns (new state, src, kind, S).  samples None: zeros (a first call that only asks for S and the row map)."""
    P = state["params"]
    N = P["xyz"].shape[0]
    grad = (state["accum"] / state["denom"]).reshape(-1)
    grad = torch.where(grad.isnan(), torch.zeros_like(grad), grad)
    dense = percent_dense * extent
    # the table of working rows
    src = torch.arange(N)
    kind = torch.zeros(N, dtype=torch.uint8)
    scaling = P["scaling"].clone()
    opacity = P["opacity"].reshape(-1).clone()
    xyz = P["xyz"].clone()
    # 1. clones: selected rows that are small; appended as they are
    size = torch.exp(scaling).max(dim=1).values
    c = torch.nonzero((grad >= max_grad) & (size <= dense)).flatten()
    src, kind = torch.cat((src, c)), torch.cat((kind, torch.ones(len(c), dtype=torch.uint8)))
    scaling, opacity, xyz = torch.cat((scaling, scaling[c])), torch.cat((opacity, opacity[c])), torch.cat((xyz, xyz[c]))
    # 2. split: the clones count as rows with zero gradient
    grad2 = torch.cat((grad, torch.zeros(len(c))))
    size = torch.exp(scaling).max(dim=1).values
    sel = (grad2 >= max_grad) & (size > dense)
    s = torch.nonzero(sel).flatten()
    S = len(s)
    samples = torch.zeros(2 * S, 3) if samples is None else samples.reshape(2 * S, 3).float()
    parent_scale = torch.exp(scaling[s])
    R = rotation_matrices(P["rotation"][src[s]])
    child_scaling = torch.log(parent_scale / (0.8 * 2))
    first = torch.bmm(R, samples[:S].unsqueeze(-1)).squeeze(-1) + xyz[s]
    second = torch.bmm(R, samples[S:].unsqueeze(-1)).squeeze(-1) + xyz[s]
    src = torch.cat((src, src[s], src[s]))
    kind = torch.cat((kind, torch.full((S,), 2, dtype=torch.uint8), torch.full((S,), 3, dtype=torch.uint8)))
    scaling = torch.cat((scaling, child_scaling, child_scaling))
    opacity = torch.cat((opacity, opacity[s], opacity[s]))
    xyz = torch.cat((xyz, first, second))
    keep = torch.cat((~sel, torch.ones(2 * S, dtype=torch.bool)))
    # 3. final prune: faint rows; with a screen-size limit also rows that are large in the world (the screen-size
    #    statistic itself was reset to zero by the appends and cannot exceed a positive limit)
    drop = torch.sigmoid(opacity) < min_opacity
    if max_screen_size:
        drop = drop | (torch.zeros(len(src)) > max_screen_size) | (torch.exp(scaling).max(dim=1).values > 0.1 * extent)
    keep = keep & ~drop
    src, kind = src[keep], kind[keep]
    out = _gather(state, src, kind)
    child = kind >= 2
    out["params"]["xyz"][child] = xyz[keep][child]
    out["params"]["scaling"][child] = scaling[keep][child]
    n = len(src)
    out["accum"], out["denom"], out["max_radii2D"] = torch.zeros(n, 1), torch.zeros(n, 1), torch.zeros(n)
    return out, src, kind, S


def near_threshold(state, min_opacity, extent, max_screen_size, percent_dense, rel=1e-5):
    """Rows whose decision in densify_and_prune lies within `rel` (relative) of a threshold, evaluated in float64 from
    the fp32 state: max exp(scaling) against the dense limit and (with a screen-size limit) the world-size limit,
    sigmoid(opacity) against min_opacity, and a child's size max exp(scaling) / 1.6 against the world-size limit.
    exp / log on the device are good to a few ulp and the chained forms to ~1e-6, so a row outside this band is
    decided alike by every correct implementation.  The gradient ratio is one correctly rounded division on both
    sides and has no band."""
    size = torch.exp(state["params"]["scaling"].double()).max(dim=1).values
    alpha = torch.sigmoid(state["params"]["opacity"].double()).reshape(-1)

    def close(v, t):
        return (v - t).abs() <= rel * abs(t)
    bad = close(size, percent_dense * extent) | close(alpha, min_opacity)
    if max_screen_size:
        bad = bad | close(size, 0.1 * extent) | close(size / 1.6, 0.1 * extent)
    return bad
