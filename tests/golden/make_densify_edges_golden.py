"""Generate tests/golden/densify_edges_golden.npz by RUNNING THE REFERENCE's own GaussianModel methods on the CPU, at
the sizes, populations and decision thresholds that densify_golden.npz does not reach.

Run in the build container only (``python tests/golden/make_densify_edges_golden.py``); the machinery (the
reference's methods compiled from their source at run time, "cuda" mapped to the CPU, the recorded torch.normal
draws, the compact fixture) is make_densify_golden.py's.  Only the vectors are committed.

Cases (seven groups, moments populated by ADAM_STEPS steps of torch.optim.Adam; `edge_state` rebuilds the state a
case starts from, for the generator and the tests alike):

  n255 .. n4097    the random recipe of make_densify_golden.case_inputs either side of the 256-thread block, the
                   2048-element scan tile and the 1024-float gather chunk: prune_points, add_densification_stats +
                   densify_and_prune, reset_opacity
  populations      N = 2049: nothing selected; everything cloned; everything split; everything pruned (zero rows);
                   split parents whose children are all pruned by the world-size limit (S > 0, no child); a single
                   surviving row (the reference's prune mask is still 1-D there: it squeezes a [rows,1] mask taken
                   before the prune, so the reference runs this case like any other);
                   size_threshold None / 0 / 20 on one state (the reference tests its truthiness)
  thresholds       N = 512, 16 groups of 32 rows on, above and below every comparison (THRESHOLD_GROUPS)
  radii3, radii2   add_densification_stats in the form training uses: update_filter = radii > 0 plus the
                   max_radii2D update of train.py:597, with a [N,3] and a [N,2] gradient

Every row that is not placed on a threshold on purpose is decided away from one: oracle.densify_oracle.
near_threshold (1e-5 relative) must be empty on the state each densify_and_prune starts from; the random recipes are
redrawn (next seed) until it is, and the seed used is stored in the fixture.

The fixture is compact like densify_golden.npz, with the kind of every row (0 old, 1 clone, 2 / 3 first / second
child) instead of a new-row flag, xyz of the CHILDREN only (a clone's equals its parent's) and their scaling once
per parent (the first children's; the second children's is asserted equal).  thr_zero shares thr_none's float vectors.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden.make_densify_golden import (ADAM_STEPS, ATTR, GROUPS, _CudaToCpu, build_model, case_inputs,  # noqa: E402
                                              load_reference, snapshot)

SIZES = (255, 256, 257, 2047, 2048, 2049, 4097)
NPOP = 2049
# name -> dict(N, seed0, max_grad, min_opacity, extent, size_threshold, percent_dense, full): `full` cases also run
# prune_points and reset_opacity
CASES = {}
for _i, _n in enumerate(SIZES):
    CASES[f"n{_n}"] = dict(N=_n, seed0=20 + _i, max_grad=0.6, min_opacity=0.005, extent=4.0, size_threshold=20,
                           percent_dense=0.01, full=True)
for _i, (_name, _mg, _thr) in enumerate([("none_selected", 100.0, 20), ("clone_all", 0.0, 20), ("split_all", 0.0, 20),
                                         ("all_faint", 0.6, 20), ("split_no_child", 0.6, 20), ("single_survivor", 0.6, 20)]):
    CASES[_name] = dict(N=NPOP, seed0=40 + _i, max_grad=_mg, min_opacity=0.005, extent=4.0, size_threshold=_thr,
                        percent_dense=0.01, full=False)
for _name, _thr in (("thr_none", None), ("thr_zero", 0), ("thr_value", 20)):
    CASES[_name] = dict(N=NPOP, seed0=50, max_grad=0.6, min_opacity=0.005, extent=4.0, size_threshold=_thr,
                        percent_dense=0.01, full=False)
CASES["thresholds"] = dict(N=512, seed0=60, max_grad=1.5, min_opacity=0.5, extent=10.0, size_threshold=20,
                           percent_dense=0.1, full=False)
STATS_CASES = {"radii3": dict(N=2049, seed=70, width=3), "radii2": dict(N=257, seed=71, width=2)}

# The threshold case: row i belongs to group perm[i] // 32.  Per group: gradient, largest scale, opacity relative
# to their thresholds ("on" = exactly on it), and what the reference makes of such a row: (old row kept, clone
# kept, children kept [0 or 2]).  max_grad = 1.5; percent_dense * extent = 0.1 * extent = 1.0 (both products are 1.0f
# in fp32 as well); min_opacity = 0.5.
#   gradient: "on" accum / denom == 1.5 exactly, "nan" 0 / 0 -> 0 (not selected), "inf" a / 0 (selected)
#   scale:    "on" largest log-scale exactly 0; "above" in (1.1, 1.5): split, children (/ 1.6) below the world limit;
#             "far" in (1.8, 2.7): split, children above the world limit
#   opacity:  "on" logit exactly 0 -> sigmoid == 0.5, not below min_opacity
THRESHOLD_GROUPS = [
    ("on", "below", "keep", (1, 1, 0)),
    ("above", "below", "keep", (1, 1, 0)),
    ("below", "below", "keep", (1, 0, 0)),
    ("above", "on", "keep", (1, 1, 0)),        # <= dense: cloned, not split; not > world limit: kept
    ("above", "above", "keep", (0, 0, 2)),
    ("above", "far", "keep", (0, 0, 0)),       # split parent, both children pruned
    ("below", "on", "keep", (1, 0, 0)),        # on the world limit: kept
    ("below", "above", "keep", (0, 0, 0)),     # above the world limit: pruned
    ("above", "below", "on", (1, 1, 0)),       # sigmoid == min_opacity: kept
    ("above", "below", "faint", (0, 0, 0)),
    ("below", "below", "on", (1, 0, 0)),
    ("below", "below", "faint", (0, 0, 0)),
    ("nan", "below", "keep", (1, 0, 0)),
    ("inf", "below", "keep", (1, 1, 0)),
    ("on", "on", "on", (1, 1, 0)),             # every comparison on its threshold at once
    ("on", "above", "keep", (0, 0, 2)),
]


def threshold_groups(N=512):
    """group of every row of the threshold case"""
    g = torch.Generator().manual_seed(6000)
    return torch.randperm(N, generator=g) // 32


def _overrides(name, c, seed, base):
    """What a constructed case replaces in the random recipe: (scaling, opacity) installed AFTER the Adam steps (so the
    values are the ones the decision sees), accum, denom."""
    params, grads, accum, denom, radii, vs_grad, vis, prune_mask = base
    N = c["N"]
    g = torch.Generator().manual_seed(8000 + seed)
    scaling = opacity = None
    u = lambda *shape: torch.rand(*shape, generator=g)
    if name == "none_selected":
        denom = torch.randint(1, 4, (N, 1), generator=g).float()          # no 0 denominators: no +inf gradients
    elif name == "clone_all":
        scaling = -3.6 - 2.0 * u(N, 3)                                    # sizes <= exp(-3.6) = 0.027 < 0.04
        opacity = -4.0 + 8.0 * u(N, 1)                                    # sigmoid >= 0.018 > 0.005: nothing pruned
        accum = accum.clone(); accum[::5] = 0.0                           # with denom 0: NaN -> 0 >= 0, selected
    elif name == "split_all":
        scaling = -3.0 + 2.0 * u(N, 3)                                    # sizes in (0.0498, 0.368): > 0.04, children < 0.4
        opacity = -4.0 + 8.0 * u(N, 1)
        accum = accum.clone(); accum[::5] = 0.0
    elif name == "all_faint":
        opacity = -8.0 - 2.0 * u(N, 1)                                    # sigmoid <= 3.4e-4 < 0.005
    elif name == "single_survivor":
        opacity = -8.0 - 2.0 * u(N, 1)
        opacity[1000] = 2.0                                               # one row survives, not selected and small
        scaling = -5.0 + 3.0 * u(N, 3)
        accum, denom = accum.clone(), denom.clone()
        accum[1000], denom[1000] = 0.1, 1.0
    elif name == "split_no_child":
        sel = ((accum / denom).nan_to_num(nan=0.0).reshape(-1) >= c["max_grad"])     # one fp32 division, as decided
        big = 0.3 + 0.7 * u(N, 3)                                         # sizes >= 1.35: children >= 0.84 > 0.4
        small = -5.0 + 3.0 * u(N, 3)                                      # sizes <= 0.135: never above 0.4
        scaling = torch.where(sel[:, None], big, small)
    elif name == "thresholds":
        grp = threshold_groups(N)
        scaling, opacity = torch.empty(N, 3), torch.empty(N, 1)
        accum, denom = torch.empty(N, 1), torch.empty(N, 1)
        for i in range(N):
            gk, sk, ok, _ = THRESHOLD_GROUPS[int(grp[i])]
            d = float(torch.randint(1, 5, (1,), generator=g))
            r = float(u(1))
            accum[i], denom[i] = {"on": (1.5 * d, d), "above": ((2.0 + r) * d, d), "below": ((0.1 + 1.3 * r) * d, d),
                                  "nan": (0.0, 0.0), "inf": (0.5 + r, 0.0)}[gk]
            s = -3.0 + 2.5 * u(3)                                         # below: sizes <= 0.61
            k = int(torch.randint(0, 3, (1,), generator=g))
            if sk != "below":
                s[k] = {"on": 0.0, "above": 0.1 + 0.3 * r, "far": 0.6 + 0.4 * r}[sk]
            scaling[i] = s
            opacity[i] = {"keep": 0.5 + 2.5 * r, "on": 0.0, "faint": -0.5 - 2.5 * r}[ok]
    return scaling, opacity, accum, denom


def edge_state(name, seed):
    """CPU state a case starts from: ({group: (param, exp_avg, exp_avg_sq)}, accum, denom, radii, vs_grad, vis,
    prune_mask) -- the random recipe stepped ADAM_STEPS times by torch.optim.Adam, then the case's overrides."""
    c = CASES[name]
    base = case_inputs(seed, c["N"])
    params, grads, accum, denom, radii, vs_grad, vis, prune_mask = base
    cpu = {n: torch.nn.Parameter(params[n].clone()) for n, _, _ in GROUPS}
    opt = torch.optim.Adam([{"params": [cpu[n]], "lr": lr, "name": n} for n, _, lr in GROUPS], lr=0.0, eps=1e-15)
    for gr in grads:
        for n, _, _ in GROUPS:
            cpu[n].grad = gr[n].clone()
        opt.step()
    scaling, opacity, accum, denom = _overrides(name, c, seed, base)
    with torch.no_grad():
        if scaling is not None:
            cpu["scaling"].copy_(scaling)
        if opacity is not None:
            cpu["opacity"].copy_(opacity)
    groups = {n: (cpu[n].detach().clone(), opt.state[cpu[n]]["exp_avg"].clone(), opt.state[cpu[n]]["exp_avg_sq"].clone())
              for n, _, _ in GROUPS}
    return groups, accum, denom, radii, vs_grad, vis, prune_mask


def exact_rows(name):
    """rows placed on a threshold on purpose (exempt from the margin condition)"""
    N = CASES[name]["N"]
    if name != "thresholds":
        return torch.zeros(N, dtype=torch.bool)
    grp = threshold_groups(N)
    on = torch.tensor([("on" in g[:3]) for g in THRESHOLD_GROUPS])
    return on[grp]


def oracle_state(groups, accum, denom, radii):
    return {"params": {n: groups[n][0] for n in groups}, "exp_avg": {n: groups[n][1] for n in groups},
            "exp_avg_sq": {n: groups[n][2] for n in groups}, "accum": accum, "denom": denom, "max_radii2D": radii}


def stats_inputs(name):
    c = STATS_CASES[name]
    g = torch.Generator().manual_seed(7500 + c["seed"])
    N = c["N"]
    accum = torch.rand(N, 1, generator=g) * 3.0
    denom = torch.randint(0, 4, (N, 1), generator=g).float()
    max_radii = torch.rand(N, generator=g) * 40.0
    radii = torch.randint(-20, 60, (N,), generator=g).clamp_min(0).to(torch.int32)     # about a quarter zeros
    vs_grad = torch.randn(N, c["width"], generator=g)
    return accum, denom, max_radii, radii, vs_grad


def golden_densify(gold, name):
    """a case's densify_and_prune vectors from the loaded fixture: (src, kind, children's xyz, children's scaling
    [both halves], samples)"""
    f = "thr_none" if name == "thr_zero" else name                        # shared float vectors, see main()
    sc = gold[f + "_densify_scaling"]
    return (gold[name + "_densify_src"], gold[name + "_densify_kind"], gold[f + "_densify_xyz"],
            np.concatenate([sc, sc]), gold[f + "_samples"])


def _install(m, groups):
    """the reference model `m` (stepped by build_model) takes the case's overridden parameters"""
    with torch.no_grad():
        for n, _, _ in GROUPS:
            getattr(m, ATTR[n]).copy_(groups[n][0])
    for n, _, _ in GROUPS:                                                # same state as edge_state built, bit for bit
        st = m.optimizer.state[getattr(m, ATTR[n])]
        assert torch.equal(st["exp_avg"], groups[n][1]) and torch.equal(st["exp_avg_sq"], groups[n][2])


def describe(snap, before, prefix, store):
    tag = snap["ins_feat"][0][:, 0]
    src = tag.round().to(torch.int64)
    assert torch.equal(src.float(), tag)
    is_new = torch.ones(len(src), dtype=torch.bool)
    for n, _, _ in GROUPS:                                                # a new row: every moment zero
        for t in snap[n][1:]:
            is_new &= (t.flatten(1).abs().sum(dim=1) == 0)
    same = (snap["xyz"][0] == before["xyz"][0][src]).all(dim=1) & (snap["scaling"][0] == before["scaling"][0][src]).all(dim=1)
    child = is_new & ~same
    nch = int(child.sum())
    assert nch % 2 == 0 and bool(child[len(src) - nch:].all())              # children are the tail, two equal halves
    kind = torch.zeros(len(src), dtype=torch.uint8)
    kind[is_new & same] = 1
    kind[len(src) - nch:len(src) - nch // 2] = 2
    kind[len(src) - nch // 2:] = 3
    assert torch.equal(src[kind == 2], src[kind == 3])
    store[prefix + "_src"] = src.numpy().astype(np.int32)
    store[prefix + "_kind"] = kind.numpy()
    store[prefix + "_xyz"] = snap["xyz"][0].numpy()[child.numpy()]
    sc = snap["scaling"][0]
    assert torch.equal(sc[kind == 2], sc[kind == 3])                       # both children of a parent: one scaling
    store[prefix + "_scaling"] = sc.numpy()[(kind == 2).numpy()]
    store[prefix + "_checksum"] = np.array([float(t.double().sum()) for n, _, _ in GROUPS for t in snap[n]])


def main():
    from oracle import densify_oracle as do
    GaussianModel = load_reference()
    store = {}
    # exact values the threshold case relies on, as this CPU evaluates them
    assert float(torch.exp(torch.zeros(1))) == 1.0 and float(torch.sigmoid(torch.zeros(1))) == 0.5
    assert float(torch.tensor([3.0]) / torch.tensor([2.0])) == 1.5 and float(torch.tensor([4.5]) / torch.tensor([3.0])) == 1.5
    assert 0.1 * 10.0 == 1.0 and float(torch.tensor(0.1) * torch.tensor(10.0)) == 1.0
    assert bool(torch.tensor([1.0]) <= 0.99999999)                        # the Python threshold is cast to fp32
    for name, c in CASES.items():
        N = c["N"]
        for attempt in range(50):
            seed = c["seed0"] + 100 * attempt
            groups, accum, denom, radii, vs_grad, vis, prune_mask = edge_state(name, seed)
            st = oracle_state(groups, accum, denom, radii)
            bad = do.near_threshold(st, c["min_opacity"], c["extent"], c["size_threshold"], c["percent_dense"]) & ~exact_rows(name)
            if not bool(bad.any()):
                break
            print(f"{name}: seed {seed} has {int(bad.sum())} rows within the margin, redrawing")
        else:
            raise RuntimeError(f"{name}: no seed satisfies the margin condition")
        store[name + "_seed"] = np.array(seed)
        params = {n: case_inputs(seed, N)[0][n] for n, _, _ in GROUPS}
        grads = case_inputs(seed, N)[1]
        before = {n: groups[n] for n in groups}
        gen = torch.Generator().manual_seed(9000 + seed)
        with _CudaToCpu(gen) as shim:
            if c["full"]:
                m = build_model(GaussianModel, params, grads); _install(m, groups)
                m.percent_dense = c["percent_dense"]
                m.xyz_gradient_accum, m.denom, m.max_radii2D = accum.clone(), denom.clone(), radii.clone()
                m.prune_points(prune_mask.clone())
                describe(snapshot(m), before, name + "_prune", store)
                store[name + "_prune_stats"] = np.concatenate([m.xyz_gradient_accum.numpy().ravel(), m.denom.numpy().ravel(),
                                                              m.max_radii2D.numpy().ravel()])
            m = build_model(GaussianModel, params, grads); _install(m, groups)
            m.percent_dense = c["percent_dense"]
            m.xyz_gradient_accum, m.denom, m.max_radii2D = accum.clone(), denom.clone(), radii.clone()
            if c["full"]:
                vsp = torch.zeros(N, 3); vsp.grad = vs_grad.clone()
                m.add_densification_stats(vsp, vis)
                store[name + "_stats_accum"] = m.xyz_gradient_accum.numpy().copy()
                store[name + "_stats_denom"] = m.denom.numpy().copy()
            shim.samples.clear()
            m.densify_and_prune(c["max_grad"], c["min_opacity"], c["extent"], c["size_threshold"])
            assert len(shim.samples) == 1
            store[name + "_samples"] = shim.samples[0].numpy()
            describe(snapshot(m), before, name + "_densify", store)
            if name == "thr_zero":
                # 0 is as false as None: the reference's result is thr_none's, bit for bit; the float vectors are stored once
                for f in ("samples", "densify_xyz", "densify_scaling"):
                    assert np.array_equal(store[f"thr_zero_{f}"], store[f"thr_none_{f}"])
                    del store[f"thr_zero_{f}"]
            n_out = m.get_xyz.shape[0]
            assert m.xyz_gradient_accum.shape == (n_out, 1) and m.denom.shape == (n_out, 1) and m.max_radii2D.shape == (n_out,)
            assert float(m.xyz_gradient_accum.abs().sum()) == 0 and float(m.denom.abs().sum()) == 0 and float(m.max_radii2D.abs().sum()) == 0
            if c["full"]:
                m = build_model(GaussianModel, params, grads); _install(m, groups)
                m.reset_opacity()
                stt = m.optimizer.state[m._opacity]
                store[name + "_reset_opacity"] = m._opacity.detach().numpy().copy()
                assert float(stt["exp_avg"].abs().sum()) == 0 and float(stt["exp_avg_sq"].abs().sum()) == 0
        k = store[name + "_densify_kind"]
        print(f"{name}: seed {seed} N {N} -> rows {len(k)} old {(k == 0).sum()} clones {(k == 1).sum()} children {(k >= 2).sum()}"
              f" S {shim.samples[0].shape[0] // 2}")
    with _CudaToCpu(torch.Generator().manual_seed(0)):
        for name, c in STATS_CASES.items():
            accum, denom, max_radii, radii, vs_grad = stats_inputs(name)
            m = GaussianModel(3)
            m.xyz_gradient_accum, m.denom, m.max_radii2D = accum.clone(), denom.clone(), max_radii.clone()
            vsp = torch.zeros(c["N"], c["width"]); vsp.grad = vs_grad.clone()
            visibility_filter = radii > 0
            m.max_radii2D[visibility_filter] = torch.max(m.max_radii2D[visibility_filter], radii[visibility_filter])    # train.py:597
            m.add_densification_stats(vsp, visibility_filter)                                                            # train.py:598
            store[name + "_accum"], store[name + "_denom"] = m.xyz_gradient_accum.numpy().copy(), m.denom.numpy().copy()
            store[name + "_max_radii2D"] = m.max_radii2D.numpy().copy()
            print(f"{name}: visible {int(visibility_filter.sum())} of {c['N']}")
    path = os.path.join(HERE, "densify_edges_golden.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
