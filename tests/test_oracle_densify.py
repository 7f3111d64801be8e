"""CPU: oracle/densify_oracle.py (the restated densification bookkeeping) against the vectors produced by RUNNING the
reference's own GaussianModel methods -- every case of densify_golden.npz and of densify_edges_golden.npz.  The
GPU tests then hold the HIP kernels to the goldens and, for state that only exists at run time, to this oracle.

Row map and kinds must be equal, copied rows bit-equal to the state before the call (moments of new rows zero), the
children's xyz / scaling and the float64 checksums at the tolerances of tests/test_41_densify_gpu.py."""
import os

import numpy as np
import pytest
import torch

from oracle import densify_oracle as do
from tests.golden import make_densify_edges_golden as edges
from tests.golden.make_densify_golden import ADAM_STEPS, GROUPS, PERCENT_DENSE, case_inputs

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
OLD = os.path.join(GOLDEN, "densify_golden.npz")
NEW = os.path.join(GOLDEN, "densify_edges_golden.npz")


def _old_cases():
    g = np.load(OLD)
    return [(int(r[0]), int(r[1]), float(r[2]), float(r[3]), None if r[4] < 0 else int(r[4])) for r in g["cases"]]


def _old_state(seed, P):
    """what make_densify_golden.build_model built: the seeded parameters after ADAM_STEPS steps of torch.optim.Adam"""
    params, grads, accum, denom, radii, vs_grad, vis, prune_mask = case_inputs(seed, P)
    cpu = {n: torch.nn.Parameter(params[n].clone()) for n, _, _ in GROUPS}
    opt = torch.optim.Adam([{"params": [cpu[n]], "lr": lr, "name": n} for n, _, lr in GROUPS], lr=0.0, eps=1e-15)
    for gr in grads:
        for n, _, _ in GROUPS:
            cpu[n].grad = gr[n].clone()
        opt.step()
    groups = {n: (cpu[n].detach().clone(), opt.state[cpu[n]]["exp_avg"].clone(), opt.state[cpu[n]]["exp_avg_sq"].clone())
              for n, _, _ in GROUPS}
    return groups, accum, denom, radii, vs_grad, vis, prune_mask


def _check_rows(out, groups, src, kind, exact_rows, got_rows=None, want_xyz=None, want_scaling=None):
    """out == the row map applied to `groups`; rows in `got_rows` of xyz / scaling are compared with the golden values"""
    src_t = torch.from_numpy(np.asarray(src).astype(np.int64))
    old = torch.from_numpy(np.asarray(kind) == 0)
    for n, _, _ in GROUPS:
        p = out["params"][n]
        assert p.shape[0] == len(src), n
        want = groups[n][0][src_t]
        if got_rows is not None and n in ("xyz", "scaling"):
            assert torch.equal(p[exact_rows], want[exact_rows]), n
            torch.testing.assert_close(p[got_rows], torch.from_numpy(want_xyz if n == "xyz" else want_scaling), rtol=1e-6, atol=1e-6)
        else:
            assert torch.equal(p, want), n
        w = old.reshape(-1, *([1] * (p.dim() - 1)))
        assert torch.equal(out["exp_avg"][n], groups[n][1][src_t] * w), n
        assert torch.equal(out["exp_avg_sq"][n], groups[n][2][src_t] * w), n


def _checksum(out):
    return np.array([float(t.double().sum()) for n, _, _ in GROUPS for t in (out["params"][n], out["exp_avg"][n], out["exp_avg_sq"][n])])


def _check_full(gold, k, groups, accum, denom, radii, vs_grad, vis, prune_mask):
    """prune_points, add_densification_stats (visible form) and reset_opacity of a case with all three"""
    st = edges.oracle_state(groups, accum, denom, radii)
    out, src, kind = do.prune_points(st, prune_mask)
    np.testing.assert_array_equal(src.numpy(), gold[k + "_prune_src"])
    assert not kind.any()
    _check_rows(out, groups, src.numpy(), kind.numpy(), None)
    np.testing.assert_array_equal(np.concatenate([out["accum"].numpy().ravel(), out["denom"].numpy().ravel(), out["max_radii2D"].numpy().ravel()]),
                                  gold[k + "_prune_stats"])
    np.testing.assert_allclose(_checksum(out), gold[k + "_prune_checksum"], rtol=1e-6, atol=1e-6)
    st2 = do.add_densification_stats(st, vs_grad, vis)
    np.testing.assert_allclose(st2["accum"].numpy(), gold[k + "_stats_accum"], rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(st2["denom"].numpy(), gold[k + "_stats_denom"])
    assert torch.equal(st2["max_radii2D"], radii)                       # the visible form leaves it alone
    ro = do.reset_opacity(st)
    torch.testing.assert_close(ro["params"]["opacity"], torch.from_numpy(gold[k + "_reset_opacity"]), rtol=1e-6, atol=1e-6)
    assert not ro["exp_avg"]["opacity"].any() and not ro["exp_avg_sq"]["opacity"].any()
    assert torch.equal(ro["exp_avg"]["xyz"], groups["xyz"][1])
    return st2


@pytest.mark.parametrize("seed,P,max_grad,extent,size_threshold", _old_cases())
def test_oracle_matches_reference_golden(seed, P, max_grad, extent, size_threshold):
    gold = np.load(OLD)
    k = f"s{seed}"
    groups, accum, denom, radii, vs_grad, vis, prune_mask = _old_state(seed, P)
    st2 = _check_full(gold, k, groups, accum, denom, radii, vs_grad, vis, prune_mask)
    samples = torch.from_numpy(gold[k + "_samples"])
    out, src, kind, S = do.densify_and_prune(st2, max_grad, 0.005, extent, size_threshold, PERCENT_DENSE, samples)
    is_new = gold[k + "_densify_new"]
    np.testing.assert_array_equal(src.numpy(), gold[k + "_densify_src"])
    np.testing.assert_array_equal(kind.numpy() != 0, is_new)
    assert 2 * S == samples.shape[0]
    # this fixture holds xyz / scaling of every new row, clones included
    _check_rows(out, groups, src.numpy(), kind.numpy(), torch.from_numpy(~is_new), torch.from_numpy(is_new),
                gold[k + "_densify_xyz"], gold[k + "_densify_scaling"])
    clone = kind == 1
    assert torch.equal(out["params"]["xyz"][clone], groups["xyz"][0][src[clone]])
    np.testing.assert_allclose(_checksum(out), gold[k + "_densify_checksum"], rtol=1e-6, atol=1e-6)
    n = len(src)
    assert tuple(gold[k + "_densify_n"]) == (n, n, n)
    assert out["accum"].shape == (n, 1) and out["denom"].shape == (n, 1) and out["max_radii2D"].shape == (n,)
    assert not out["accum"].any() and not out["denom"].any() and not out["max_radii2D"].any()


@pytest.mark.parametrize("name", list(edges.CASES))
def test_oracle_matches_reference_edges_golden(name):
    gold = np.load(NEW)
    c = edges.CASES[name]
    groups, accum, denom, radii, vs_grad, vis, prune_mask = edges.edge_state(name, int(gold[name + "_seed"]))
    st = edges.oracle_state(groups, accum, denom, radii)
    if c["full"]:
        st = _check_full(gold, name, groups, accum, denom, radii, vs_grad, vis, prune_mask)
    # the margin condition the fixture was generated under still holds for the state rebuilt here
    bad = do.near_threshold(st, c["min_opacity"], c["extent"], c["size_threshold"], c["percent_dense"]) & ~edges.exact_rows(name)
    assert not bad.any()
    g_src, g_kind, g_xyz, g_scaling, g_samples = edges.golden_densify(gold, name)
    samples = torch.from_numpy(g_samples)
    out, src, kind, S = do.densify_and_prune(st, c["max_grad"], c["min_opacity"], c["extent"], c["size_threshold"],
                                             c["percent_dense"], samples)
    np.testing.assert_array_equal(src.numpy(), g_src)
    np.testing.assert_array_equal(kind.numpy(), g_kind)
    assert 2 * S == samples.shape[0]
    child = torch.from_numpy(g_kind >= 2)
    _check_rows(out, groups, g_src, g_kind, ~child, child, g_xyz, g_scaling)
    np.testing.assert_allclose(_checksum(out), gold[name + "_densify_checksum"], rtol=1e-6, atol=1e-6)
    n = len(g_src)
    assert out["accum"].shape == (n, 1) and out["denom"].shape == (n, 1) and out["max_radii2D"].shape == (n,)
    assert not out["accum"].any() and not out["denom"].any() and not out["max_radii2D"].any()


def test_threshold_case_is_what_it_names():
    """every group of the threshold case has its 32 rows, and the REFERENCE made of them what THRESHOLD_GROUPS says"""
    gold = np.load(NEW)
    src, kind, *_ = edges.golden_densify(gold, "thresholds")
    grp = edges.threshold_groups().numpy()
    for gi, (_, _, _, (n_old, n_clone, n_child)) in enumerate(edges.THRESHOLD_GROUPS):
        rows = np.nonzero(grp == gi)[0]
        assert len(rows) == 32
        for r in rows:
            k = kind[src == r]
            assert ((k == 0).sum(), (k == 1).sum(), (k >= 2).sum()) == (n_old, n_clone, n_child), (gi, r)


def test_size_threshold_truthiness():
    """the fixture's three size_threshold cases are what they name: 0 prunes like None, a value prunes more"""
    gold = np.load(NEW)
    none, zero, value = (edges.golden_densify(gold, n) for n in ("thr_none", "thr_zero", "thr_value"))
    np.testing.assert_array_equal(none[0], zero[0])
    np.testing.assert_array_equal(none[1], zero[1])
    assert len(value[0]) < len(none[0]) and (value[1] >= 2).sum() < (none[1] >= 2).sum() and (value[1] == 0).sum() < (none[1] == 0).sum()


@pytest.mark.parametrize("name", list(edges.STATS_CASES))
def test_oracle_radii_statistics_match_reference(name):
    """the form training uses: update_filter None, visible = radii > 0, max_radii2D updated in the same pass"""
    gold = np.load(NEW)
    accum, denom, max_radii, radii, vs_grad = edges.stats_inputs(name)
    assert (radii == 0).any() and (radii > 0).any() and vs_grad.shape[1] == edges.STATS_CASES[name]["width"]
    st = do.add_densification_stats({"accum": accum, "denom": denom, "max_radii2D": max_radii}, vs_grad, None, radii)
    np.testing.assert_allclose(st["accum"].numpy(), gold[name + "_accum"], rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(st["denom"].numpy(), gold[name + "_denom"])
    np.testing.assert_array_equal(st["max_radii2D"].numpy(), gold[name + "_max_radii2D"])
