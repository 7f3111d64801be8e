"""GPU: opengaussian_amd.densify at the sizes, populations and decision thresholds that tests/test_41_densify_gpu.py
does not reach, against vectors produced by RUNNING the reference's own GaussianModel methods
(tests/golden/make_densify_edges_golden.py -> densify_edges_golden.npz), and -- for state that only exists at run
time -- against oracle/densify_oracle.py, which tests/test_oracle_densify.py holds to the same vectors.

  sizes        255 .. 4097 rows: either side of the 256-thread block, the 2048-element scan tile (past it the scan
               takes two launches with per-workgroup partials) and the 1024-float gather chunk
  populations  nothing selected, all cloned, all split, zero rows, split parents without a surviving child, one
               surviving row, size_threshold None / 0 / 20
  thresholds   32 rows on, above and below each comparison of densify_flags_kernel
  statistics   add_densification_stats(update_filter=None, radii=...), the form training uses
  chained      densify, Adam, densify, prune_points, reset_opacity on one evolving device state

Old rows are compared bit-exact (parameters and moments), new rows carry the parent's parameters with zero moments,
the children's xyz / scaling to 1e-6; no row is exempt.  Every row that does not sit on a threshold on purpose is
decided at least 1e-5 (relative) away from one (oracle.densify_oracle.near_threshold), ten times what the device's
exp / log chains can differ by."""
import os

import numpy as np
import pytest
import torch

from oracle import densify_oracle as do
from tests.golden import make_densify_edges_golden as edges
from tests.golden.make_densify_golden import ADAM_STEPS, GROUPS, case_inputs

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "densify_edges_golden.npz")
MOMENTS = ("exp_avg", "exp_avg_sq")


def _install(groups, accum, denom, radii, dev, fused, percent_dense, step=ADAM_STEPS):
    """a CPU state ({group: (param, exp_avg, exp_avg_sq)} + statistics) as a DensifyState over a GPU optimizer"""
    from opengaussian_amd.densify import DensifyState
    from opengaussian_amd.optim import FusedAdam
    gpu = {n: torch.nn.Parameter(groups[n][0].to(dev)) for n, _, _ in GROUPS}
    Opt = FusedAdam if fused else torch.optim.Adam
    opt = Opt([{"params": [gpu[n]], "lr": lr, "name": n} for n, _, lr in GROUPS], lr=0.0, eps=1e-15)
    for n, _, _ in GROUPS:
        opt.state[gpu[n]] = {"step": torch.tensor(float(step)), "exp_avg": groups[n][1].to(dev), "exp_avg_sq": groups[n][2].to(dev)}
    return DensifyState(opt, accum.to(dev), denom.to(dev), radii.to(dev), percent_dense)


def _download(state):
    """the device state as the oracle's dict of CPU tensors"""
    P = state.params()
    st = {"params": {}, "exp_avg": {}, "exp_avg_sq": {}}
    for n, _, _ in GROUPS:
        st["params"][n] = P[n].detach().cpu().clone()
        for m in MOMENTS:
            st[m][n] = state.optimizer.state[P[n]][m].cpu().clone()
    st["accum"], st["denom"], st["max_radii2D"] = state.xyz_gradient_accum.cpu().clone(), state.denom.cpu().clone(), state.max_radii2D.cpu().clone()
    return st


def _check_state(state, want, child=None, step=None):
    """device state == `want` (an oracle-style dict): bit-exact, except xyz / scaling of the `child` rows at 1e-6"""
    got = _download(state)
    P = state.params()
    for n, _, _ in GROUPS:
        g, w = got["params"][n], want["params"][n]
        assert g.shape == w.shape and P[n].requires_grad and P[n].is_leaf and P[n].is_cuda, n
        if child is not None and n in ("xyz", "scaling"):
            assert torch.equal(g[~child], w[~child]), n
            torch.testing.assert_close(g[child], w[child], rtol=1e-6, atol=1e-6)
        else:
            assert torch.equal(g, w), n
        for m in MOMENTS:
            assert torch.equal(got[m][n], want[m][n]), (n, m)
        if step is not None:
            assert float(state.optimizer.state[P[n]]["step"]) == float(step)
    return got


def _expected_from_map(groups, src, kind, child_xyz, child_scaling):
    """the golden's compact form expanded: rows of the state before the call through the row map, moments of new rows
    zero, the children's xyz / scaling from the reference"""
    st = {"params": {n: groups[n][0] for n in groups}, "exp_avg": {n: groups[n][1] for n in groups},
          "exp_avg_sq": {n: groups[n][2] for n in groups}}
    src_t, kind_t = torch.from_numpy(src.astype(np.int64)), torch.from_numpy(kind)
    want = do._gather(st, src_t, kind_t)
    child = kind_t >= 2
    if child_xyz is not None:
        want["params"]["xyz"][child] = torch.from_numpy(child_xyz)
        want["params"]["scaling"][child] = torch.from_numpy(child_scaling)
    return want, child


def _checksum(got):
    return np.array([float(t.double().sum()) for n, _, _ in GROUPS for t in (got["params"][n], got["exp_avg"][n], got["exp_avg_sq"][n])])


def _step(state):
    """the optimizer still steps after the surgery (zero rows included)"""
    for p in state.params().values():
        p.grad = torch.ones_like(p)
    state.optimizer.step()
    torch.cuda.synchronize()
    for p in state.params().values():
        assert bool(torch.isfinite(p).all())


def _zero_stats(state, n):
    assert state.xyz_gradient_accum.shape == (n, 1) and state.denom.shape == (n, 1) and state.max_radii2D.shape == (n,)
    assert state.xyz_gradient_accum.is_cuda and state.denom.is_cuda and state.max_radii2D.is_cuda
    assert not state.xyz_gradient_accum.any() and not state.denom.any() and not state.max_radii2D.any()


def _premise(name, N, plan, n_out):
    """a population case must still BE the case it names"""
    kept, clones, children, S = plan["kept"], plan["clones"], plan["split_children"], plan["split_parents_selected"]
    if name == "none_selected":
        assert clones == 0 and S == 0 and children == 0 and 0 < kept < N
    elif name == "clone_all":
        assert clones == N and kept == N and S == 0 and children == 0
    elif name == "split_all":
        assert S == N and children == 2 * N and kept == 0 and clones == 0
    elif name == "all_faint":
        assert n_out == 0 and S > 0
    elif name == "split_no_child":
        assert S > 0 and children == 0 and clones == 0 and kept > 0
    elif name == "single_survivor":
        assert n_out == 1 and kept == 1 and S > 0
    elif name.startswith("n"):
        assert kept > 0 and clones > 0 and children > 0


@pytest.mark.parametrize("name", list(edges.CASES))
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
def test_edge_cases_match_reference_golden(gpu_device, name, fused):
    from opengaussian_amd import densify
    gold = np.load(GOLD)
    c = edges.CASES[name]
    dev, N = gpu_device, c["N"]
    groups, accum, denom, radii, vs_grad, vis, prune_mask = edges.edge_state(name, int(gold[name + "_seed"]))
    new_state = lambda: _install(groups, accum, denom, radii, dev, fused, c["percent_dense"])

    if c["full"]:
        # ---- prune_points ---------------------------------------------------------------------------------------
        state = new_state()
        params = densify.prune_points(state, prune_mask.to(dev))
        assert set(params) == {n for n, _, _ in GROUPS}
        src = gold[name + "_prune_src"]
        np.testing.assert_array_equal(src, np.nonzero(~prune_mask.numpy())[0])
        want, _ = _expected_from_map(groups, src, np.zeros(len(src), np.uint8), None, None)
        got = _check_state(state, want, step=ADAM_STEPS)
        np.testing.assert_array_equal(np.concatenate([got["accum"].numpy().ravel(), got["denom"].numpy().ravel(), got["max_radii2D"].numpy().ravel()]),
                                      gold[name + "_prune_stats"])
        np.testing.assert_allclose(_checksum(got), gold[name + "_prune_checksum"], rtol=1e-6, atol=1e-6)
        _step(state)
        # ---- reset_opacity --------------------------------------------------------------------------------------
        state = new_state()
        out = densify.reset_opacity(state)
        torch.testing.assert_close(out["opacity"].detach().cpu(), torch.from_numpy(gold[name + "_reset_opacity"]), rtol=1e-6, atol=1e-6)
        st = state.optimizer.state[out["opacity"]]
        assert st["exp_avg"].shape == (N, 1) and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
        for n, _, _ in GROUPS:
            if n != "opacity":
                p = state.params()[n]
                assert torch.equal(p.detach().cpu(), groups[n][0]) and torch.equal(state.optimizer.state[p]["exp_avg"].cpu(), groups[n][1])
        _step(state)

    # ---- (add_densification_stats +) densify_and_prune -------------------------------------------------------------
    state = new_state()
    if c["full"]:
        densify.add_densification_stats(state, vs_grad.to(dev), vis.to(dev))
        np.testing.assert_allclose(state.xyz_gradient_accum.cpu().numpy(), gold[name + "_stats_accum"], rtol=1e-6, atol=1e-7)
        np.testing.assert_array_equal(state.denom.cpu().numpy(), gold[name + "_stats_denom"])
    g_src, g_kind, g_xyz, g_scaling, g_samples = edges.golden_densify(gold, name)
    params = densify.densify_and_prune(state, c["max_grad"], c["min_opacity"], c["extent"], c["size_threshold"],
                                       samples=torch.from_numpy(g_samples).to(dev))
    plan = state.last_plan
    n_out = len(g_src)
    np.testing.assert_array_equal(plan["src_row"].cpu().numpy(), g_src)          # same rows, same order as the reference
    np.testing.assert_array_equal(plan["kind"].cpu().numpy(), g_kind)
    assert plan["split_parents_selected"] * 2 == g_samples.shape[0]
    assert plan["kept"] + plan["clones"] + plan["split_children"] == n_out
    assert (plan["kept"], plan["clones"], plan["split_children"]) == ((g_kind == 0).sum(), (g_kind == 1).sum(), (g_kind >= 2).sum())
    _premise(name, N, plan, n_out)
    want, child = _expected_from_map(groups, g_src, g_kind, g_xyz, g_scaling)
    got = _check_state(state, want, child, step=ADAM_STEPS)
    assert set(params) == {n for n, _, _ in GROUPS} and all(params[n] is state.params()[n] for n in params)
    _zero_stats(state, n_out)
    np.testing.assert_allclose(_checksum(got), gold[name + "_densify_checksum"], rtol=1e-6, atol=1e-6)
    _step(state)


def test_threshold_rows_on_the_device(gpu_device):
    """every comparison of densify_flags_kernel, row by row: the 32 rows on the threshold and the 32 rows either side of
    it each come out in the kinds the reference gives them (tests/golden/make_densify_edges_golden.THRESHOLD_GROUPS)"""
    from opengaussian_amd import densify
    gold = np.load(GOLD)
    c = edges.CASES["thresholds"]
    groups, accum, denom, radii, *_ = edges.edge_state("thresholds", int(gold["thresholds_seed"]))
    # the exact rows are exact: sizes of exactly 1, opacities of exactly 0.5, ratios of exactly 1.5, 0 / 0 and a / 0
    grp = edges.threshold_groups()
    for gi, (gk, sk, ok, _) in enumerate(edges.THRESHOLD_GROUPS):
        rows = grp == gi
        if gk == "on":
            assert bool(((accum / denom)[rows] == 1.5).all())
        if gk in ("nan", "inf"):
            assert bool((denom[rows] == 0).all()) and bool(((accum[rows] == 0) if gk == "nan" else (accum[rows] > 0)).all())
        if sk == "on":
            assert bool((groups["scaling"][0][rows].max(dim=1).values == 0).all())
        if ok == "on":
            assert bool((groups["opacity"][0][rows] == 0).all())
    state = _install(groups, accum, denom, radii, gpu_device, True, c["percent_dense"])
    S = gold["thresholds_samples"].shape[0] // 2
    densify.densify_and_prune(state, c["max_grad"], c["min_opacity"], c["extent"], c["size_threshold"],
                              samples=torch.from_numpy(gold["thresholds_samples"]).to(gpu_device))
    plan = state.last_plan
    assert plan["split_parents_selected"] == S == 32 * sum(1 for g in edges.THRESHOLD_GROUPS if g[0] != "below" and g[0] != "nan" and g[1] in ("above", "far"))
    src, kind = plan["src_row"].cpu().numpy(), plan["kind"].cpu().numpy()
    for gi, (gk, sk, ok, (n_old, n_clone, n_child)) in enumerate(edges.THRESHOLD_GROUPS):
        rows = np.nonzero(grp.numpy() == gi)[0]
        assert len(rows) == 32
        for r in rows:
            k = kind[src == r]
            assert ((k == 0).sum(), (k == 1).sum(), (k == 2).sum(), (k == 3).sum()) == (n_old, n_clone, n_child // 2, n_child // 2), \
                f"group {gi} (gradient {gk}, scale {sk}, opacity {ok}) row {r}: kinds {k.tolist()}"


@pytest.mark.parametrize("name", ["split_no_child", "split_all", "all_faint"])
def test_samples_none_on_degenerate_splits(gpu_device, name):
    """samples=None where split parents are selected and no (or every) child survives: the call succeeds and plans
    the rows of the call with explicit samples"""
    from opengaussian_amd import densify
    gold = np.load(GOLD)
    c = edges.CASES[name]
    groups, accum, denom, radii, *_ = edges.edge_state(name, int(gold[name + "_seed"]))
    state = _install(groups, accum, denom, radii, gpu_device, True, c["percent_dense"])
    gen = torch.Generator(device=gpu_device).manual_seed(5)
    densify.densify_and_prune(state, c["max_grad"], c["min_opacity"], c["extent"], c["size_threshold"], generator=gen)
    plan = state.last_plan
    g_src, g_kind, g_xyz, g_scaling, _ = edges.golden_densify(gold, name)
    np.testing.assert_array_equal(plan["src_row"].cpu().numpy(), g_src)
    np.testing.assert_array_equal(plan["kind"].cpu().numpy(), g_kind)
    _premise(name, c["N"], plan, len(g_src))
    # everything but the children's positions is the reference's result; the children lie within a few sigma of the parent
    want, child = _expected_from_map(groups, g_src, g_kind, g_xyz, g_scaling)
    got = _download(state)
    want["params"]["xyz"][child] = got["params"]["xyz"][child]
    _check_state(state, want, child, step=ADAM_STEPS)
    if child.any():
        par = torch.from_numpy(g_src.astype(np.int64))[child]
        off = (got["params"]["xyz"][child] - groups["xyz"][0][par]).norm(dim=1)
        smax = torch.exp(groups["scaling"][0][par]).max(dim=1).values
        assert float((off / smax).max()) < 8.0 and float(off.min()) > 0.0
    _zero_stats(state, len(g_src))
    _step(state)


@pytest.mark.parametrize("name", list(edges.STATS_CASES))
def test_radii_form_of_the_statistics(gpu_device, name):
    """add_densification_stats(state, grad, None, radii) -- visible = radii > 0, max_radii2D updated in the same pass --
    against the reference's two statements (train.py:597-598) with a stride of 3 and of 2"""
    from opengaussian_amd import densify
    from opengaussian_amd.densify import DensifyState
    gold = np.load(GOLD)
    dev = gpu_device
    accum, denom, max_radii, radii, vs_grad = edges.stats_inputs(name)
    assert radii.dtype == torch.int32 and (radii == 0).any() and vs_grad.shape[1] == edges.STATS_CASES[name]["width"]
    state = DensifyState(None, accum.to(dev), denom.to(dev), max_radii.to(dev))
    densify.add_densification_stats(state, vs_grad.to(dev), None, radii.to(dev))
    np.testing.assert_allclose(state.xyz_gradient_accum.cpu().numpy(), gold[name + "_accum"], rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(state.denom.cpu().numpy(), gold[name + "_denom"])
    np.testing.assert_array_equal(state.max_radii2D.cpu().numpy(), gold[name + "_max_radii2D"])
    hidden = (radii == 0).numpy()                                        # rows that are not visible are untouched, bit for bit
    np.testing.assert_array_equal(state.xyz_gradient_accum.cpu().numpy()[hidden], accum.numpy()[hidden])
    np.testing.assert_array_equal(state.max_radii2D.cpu().numpy()[hidden], max_radii.numpy()[hidden])


def test_chained_rounds_against_the_oracle(gpu_device):
    """densify, two Adam steps, densify again, prune_points, reset_opacity on ONE evolving device state.  Before every
    call the device state is downloaded and handed to the oracle with the samples used, so the optimizer's ulp drift
    cannot become a decision flip; before each densify the margin condition is checked on that state."""
    from opengaussian_amd import densify
    dev, N = gpu_device, 3000
    MAX_GRAD, MIN_OPACITY, EXTENT, THRESHOLD, PERCENT_DENSE = 1.5, 0.005, 4.0, 20, 0.01
    params, grads, accum, denom, radii, *_ = case_inputs(77, N)
    cpu = {n: torch.nn.Parameter(params[n].clone()) for n, _, _ in GROUPS}
    ref = torch.optim.Adam([{"params": [cpu[n]], "lr": lr, "name": n} for n, _, lr in GROUPS], lr=0.0, eps=1e-15)
    for gr in grads:
        for n, _, _ in GROUPS:
            cpu[n].grad = gr[n].clone()
        ref.step()
    groups = {n: (cpu[n].detach().clone(), ref.state[cpu[n]]["exp_avg"].clone(), ref.state[cpu[n]]["exp_avg_sq"].clone()) for n, _, _ in GROUPS}
    state = _install(groups, accum, denom, radii, dev, True, PERCENT_DENSE)
    g = torch.Generator().manual_seed(78)
    counts = [N]

    def observe():
        """two views' statistics in the form training uses, compared with the oracle"""
        for _ in range(2):
            n = counts[-1]
            st = _download(state)
            grad = torch.randn(n, 3, generator=g)
            rad = torch.randint(-10, 40, (n,), generator=g).clamp_min(0).to(torch.int32)
            want = do.add_densification_stats(st, grad, None, rad)
            densify.add_densification_stats(state, grad.to(dev), None, rad.to(dev))
            torch.testing.assert_close(state.xyz_gradient_accum.cpu(), want["accum"], rtol=1e-6, atol=1e-7)
            assert torch.equal(state.denom.cpu(), want["denom"]) and torch.equal(state.max_radii2D.cpu(), want["max_radii2D"])

    def densify_round():
        st = _download(state)
        for _ in range(3):                                              # a row inside the margin: moved off it, on both sides alike
            bad = do.near_threshold(st, MIN_OPACITY, EXTENT, THRESHOLD, PERCENT_DENSE)
            if not bad.any():
                break
            P = state.params()
            P["scaling"].data[bad.to(dev)] += 1e-3
            P["opacity"].data[bad.to(dev)] += 1e-3
            st = _download(state)
        assert not do.near_threshold(st, MIN_OPACITY, EXTENT, THRESHOLD, PERCENT_DENSE).any()
        _, _, _, S = do.densify_and_prune(st, MAX_GRAD, MIN_OPACITY, EXTENT, THRESHOLD, PERCENT_DENSE, None)
        samples = torch.randn(2 * S, 3, generator=g) * 0.05
        want, src, kind, _ = do.densify_and_prune(st, MAX_GRAD, MIN_OPACITY, EXTENT, THRESHOLD, PERCENT_DENSE, samples)
        step = float(state.optimizer.state[state.params()["xyz"]]["step"])
        densify.densify_and_prune(state, MAX_GRAD, MIN_OPACITY, EXTENT, THRESHOLD, samples=samples.to(dev))
        plan = state.last_plan
        assert torch.equal(plan["src_row"].cpu().long(), src) and torch.equal(plan["kind"].cpu(), kind)
        assert plan["split_parents_selected"] == S
        assert (kind == 0).any() and (kind == 1).any() and (kind >= 2).any()
        _check_state(state, want, kind >= 2, step=step)
        _zero_stats(state, len(src))
        counts.append(len(src))

    observe()
    densify_round()
    for _ in range(2):
        for p in state.params().values():
            p.grad = (torch.randn(p.shape, generator=g) * 0.1).to(dev)
        state.optimizer.step()
    observe()
    densify_round()
    # prune_points with a random quarter of the rows
    st = _download(state)
    mask = torch.rand(counts[-1], generator=g) < 0.25
    want, src, kind = do.prune_points(st, mask)
    densify.prune_points(state, mask.to(dev))
    got = _check_state(state, want)
    assert torch.equal(got["accum"], want["accum"]) and torch.equal(got["denom"], want["denom"]) and torch.equal(got["max_radii2D"], want["max_radii2D"])
    counts.append(len(src))
    # reset_opacity
    st = _download(state)
    want = do.reset_opacity(st)
    densify.reset_opacity(state)
    got = _download(state)
    torch.testing.assert_close(got["params"]["opacity"], want["params"]["opacity"], rtol=1e-6, atol=1e-6)
    want["params"]["opacity"] = got["params"]["opacity"]
    _check_state(state, want)
    assert len(counts) == 4 and all(a != b for a, b in zip(counts, counts[1:])), counts     # the point count changed three times
    _step(state)


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8], ids=["bool", "uint8"])
def test_prune_points_masks(gpu_device, dtype):
    """all-False keeps every row in place, all-True leaves zero rows, a random mask removes its rows -- whether the mask
    arrives as bool or as uint8 -- at 2049 rows (two scan tiles, an odd tail)"""
    from opengaussian_amd import densify
    dev, N = gpu_device, 2049
    gold = np.load(GOLD)
    groups, accum, denom, radii, _, _, prune_mask = edges.edge_state("n2049", int(gold["n2049_seed"]))
    st = edges.oracle_state(groups, accum, denom, radii)
    for mask in (torch.zeros(N, dtype=torch.bool), torch.ones(N, dtype=torch.bool), prune_mask):
        state = _install(groups, accum, denom, radii, dev, True, 0.01)
        want, src, kind = do.prune_points(st, mask)
        densify.prune_points(state, mask.to(dtype).to(dev))
        got = _check_state(state, want, step=ADAM_STEPS)
        n = N - int(mask.sum())
        assert got["params"]["xyz"].shape == (n, 3) and got["params"]["f_rest"].shape == (n, 15, 3)
        if n == N:
            assert torch.equal(src, torch.arange(N))
        assert torch.equal(got["accum"], want["accum"]) and torch.equal(got["denom"], want["denom"]) and torch.equal(got["max_radii2D"], want["max_radii2D"])
        assert got["accum"].shape == (n, 1) and got["max_radii2D"].shape == (n,)
        _step(state)
