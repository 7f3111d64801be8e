"""GPU: the feature votes (ogs_raster_feature_votes, rasterizer.feature_votes, query.lift_features, features_from_votes,
lift_mask_features): the exact integer equalities the fixed-point table promises (with the label votes among them), its bounds,
the float64 restatement, the device's own route through the features-only backward, the pass's alpha, and the per-mask route
as an independent cross-check.

Measured on the MI355X (figures printed by the tests): the largest error against the float64 restatement on rows held to the
bar, and the largest cell difference against the backward route in units of its bar, are recorded in DESIGN.md section 6l."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import feature_votes_cases as fc
from tests import feature_votes_restatement as fr
from tests import helpers
from tests import label_votes_cases as vc
from tests.test_39_label_map_gpu import PIPE, _fresh_pass, _model_of, kept_cache  # noqa: F401  (kept_cache: a fixture)

pytestmark = pytest.mark.gpu

_RUNS: dict = {}
_PASSES: dict = {}
Q = 1 << 32
SENTINEL = -0x0123456789ABCDEF


def _hooks():
    from opengaussian_amd import _lib
    return int(_lib.lib().ogs_feature_votes_fold_columns()), int(_lib.lib().ogs_feature_votes_block_columns())


def _pass(scene, dev):
    """one kept pass per scene, in both layouts: (alpha [H, W], keep_sink dict, compacted KeptPasses entry)"""
    if scene not in _PASSES:
        from opengaussian_amd import rasterizer as R
        sc, cam = vc.scene(scene)
        (color, radii, depth, alpha), kept = _fresh_pass(sc, cam, dev)
        assert kept is not None
        kp = R.KeptPasses(budget_bytes=1 << 30)
        assert kp.admit("slot", "key", None, kept)
        _PASSES[scene] = (alpha[0], kept, kp.slots["slot"], kp)
    return _PASSES[scene][:3]


def _run(name, dev):
    """everything the tests below compare, once per case"""
    if name in _RUNS:
        return _RUNS[name]
    from opengaussian_amd import rasterizer as R
    c = fc.case(name, *_hooks())
    alpha, kept, entry = _pass(name.split("_")[0], dev)
    F = c["features"].to(dev)
    valid = None if c["valid"] is None else c["valid"].to(dev)
    P = c["sc"].means3D.shape[0]
    votes = R.feature_votes(kept, F, valid=valid)
    compact = R.feature_votes(entry, F, valid=valid)
    rows = vc.leaf_rows(P).to(dev)
    by_rows = R.feature_votes(kept, F, valid=valid, rows=rows, num_rows=vc.LEAF_ROWS)
    magnitude = R.feature_votes(kept, F.abs(), valid=valid)                  # the lift of |F|: what the sums are rounded against
    torch.cuda.synchronize()
    r = dict(case=c, D=c["D"], alpha=alpha, kept=kept, entry=entry, F=F, valid=valid, votes=votes, compact=compact, rows=rows,
             by_rows=by_rows, magnitude=magnitude, P=P)
    _RUNS[name] = r
    return r


# ---- 1. exact equalities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_exact_integer_equalities(gpu_device, name):
    from opengaussian_amd import rasterizer as R
    r = _run(name, gpu_device)
    fold, block = _hooks()
    D, P, F, valid, votes, kept = r["D"], r["P"], r["F"], r["valid"], r["votes"], r["kept"]
    assert votes.dtype == torch.int64 and votes.shape == (P, D + 1)
    assert bool((votes[:, D] >= 0).all()) and bool(votes[:, D].any()) and bool((votes[:, :D] < 0).any()) and bool((votes[:, :D] > 0).any())
    # 1. two runs into fresh tables; the pass's own layout against the compacted one of a KeptPasses entry
    assert torch.equal(votes, R.feature_votes(kept, F, valid=valid))
    assert torch.equal(votes, r["compact"])
    # 2. rows = r against index_add of rows = None (-1, >= R and 2^40 dropped), from both layouts
    rows = r["rows"]
    ok = (rows >= 0) & (rows < vc.LEAF_ROWS)
    want = torch.zeros(vc.LEAF_ROWS, D + 1, dtype=torch.int64, device=gpu_device).index_add_(0, rows[ok], votes[ok])
    assert torch.equal(r["by_rows"], want)
    assert torch.equal(R.feature_votes(r["entry"], F, valid=valid, rows=rows, num_rows=vc.LEAF_ROWS), want)
    assert bool(ok.any()) and not bool(ok.all())
    # 3. two calls into one table give twice the table
    twice = R.feature_votes(kept, F, valid=valid)
    assert R.feature_votes(kept, F, valid=valid, out=twice) is twice
    assert torch.equal(twice, 2 * votes)
    # 4. -F negates the columns < D and leaves the weight column
    neg = R.feature_votes(kept, -F, valid=valid)
    assert torch.equal(neg[:, :D], -votes[:, :D]) and torch.equal(neg[:, D], votes[:, D])
    # 5. a permutation of the channels permutes the columns
    perm = torch.randperm(D, generator=torch.Generator().manual_seed(D)).to(gpu_device)
    permuted = R.feature_votes(kept, F[perm], valid=valid)
    assert torch.equal(permuted[:, :D], votes[:, perm]) and torch.equal(permuted[:, D], votes[:, D])
    # 6. the channels split over several calls: at the fold's 16 columns, at the walk's block, and both
    for cuts in ([fold], [block], [fold, block], [1]):
        cuts = [0] + [c for c in cuts if c < D] + [D]
        if len(cuts) < 3:
            continue
        parts = [R.feature_votes(kept, F[a:b], valid=valid) for a, b in zip(cuts[:-1], cuts[1:])]
        assert torch.equal(torch.cat([p[:, :-1] for p in parts], dim=1), votes[:, :D]), cuts
        assert all(torch.equal(p[:, -1], votes[:, D]) for p in parts), cuts
    # a bool, a uint8 and an int64 mask are the same mask; fp64 copies and a strided view of the features are the same features
    if valid is not None:
        assert torch.equal(votes, R.feature_votes(kept, F, valid=valid.to(torch.uint8) * 255))
        assert torch.equal(votes, R.feature_votes(kept, F, valid=valid.to(torch.int64) * -7))
    assert torch.equal(votes, R.feature_votes(kept, F.double(), valid=valid))
    assert torch.equal(votes, R.feature_votes(kept, F.permute(1, 2, 0).contiguous().permute(2, 0, 1), valid=valid))


@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_weight_column_is_the_label_vote_of_the_mask(gpu_device, name):
    """7. column D = column 0 of label_votes over the image (valid ? 0 : -1) with one label: the fold keeps the vote kernel's chain"""
    from opengaussian_amd import rasterizer as R
    r = _run(name, gpu_device)
    valid = r["valid"] if r["valid"] is not None else torch.ones(vc.H, vc.W, dtype=torch.bool, device=gpu_device)
    lab = torch.where(valid, 0, -1).to(torch.int64)
    want = R.label_votes(r["kept"], lab, 1)
    assert torch.equal(r["votes"][:, r["D"]], want[:, 0])
    if r["valid"] is not None:
        assert bool(want[:, 1].any())                     # weight did land on invalid pixels: the mask removed something
    by_rows = R.label_votes(r["kept"], lab, 1, rows=r["rows"], num_rows=vc.LEAF_ROWS)
    assert torch.equal(r["by_rows"][:, r["D"]], by_rows[:, 0])


@pytest.mark.parametrize("scene", ["P300", "P1500", "wide"])
@pytest.mark.parametrize("kind", ["blocks8", "noise5"])
@pytest.mark.parametrize("masked", [False, True])
def test_one_hot_features_give_the_label_votes(gpu_device, scene, kind, masked):
    """8. F[c] = (lab == c): the columns < D are the label votes' columns, bit for bit"""
    from opengaussian_amd import rasterizer as R
    _, kept, entry = _pass(scene, gpu_device)
    img, L = vc.label_image("blocks8", 11) if kind == "blocks8" else vc.label_image("noise", 5)
    img = img.to(gpu_device)
    valid = fc.valid_mask().to(gpu_device) if masked else None
    F = (img[None] == torch.arange(L, device=gpu_device)[:, None, None]).to(torch.float32)
    got = R.feature_votes(kept, F, valid=valid)
    lab = img if valid is None else torch.where(valid, img, torch.full_like(img, -1))
    want = R.label_votes(entry, lab, L)
    assert bool(want[:, :L].any())
    assert torch.equal(got[:, :L], want[:, :L])
    # the weight column is the valid weight whatever the labels are
    counted = torch.ones_like(img, dtype=torch.bool) if valid is None else valid
    assert torch.equal(got[:, L], R.label_votes(kept, torch.where(counted, 0, -1).to(torch.int64), 1)[:, 0])


# ---- 2. bounds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P1500_2b+1_masked", "wide_b+1", "P1500_b", "P300_3_masked"])
def test_nothing_is_written_outside_the_table(gpu_device, name):
    from opengaussian_amd import rasterizer as R
    r = _run(name, gpu_device)
    D, F, valid = r["D"], r["F"], r["valid"]
    for rows, Rn, want in ((None, r["P"], r["votes"]), (r["rows"], vc.LEAF_ROWS, r["by_rows"])):
        pad = 3
        big = torch.full((Rn + 2 * pad, D + 1), SENTINEL, dtype=torch.int64, device=gpu_device)
        table = big[pad:pad + Rn]
        table.zero_()
        R.feature_votes(r["kept"], F, valid=valid, rows=rows, num_rows=None if rows is None else Rn, out=table)
        assert torch.equal(table, want)
        assert bool((big[:pad] == SENTINEL).all()) and bool((big[pad + Rn:] == SENTINEL).all())
    # fewer rows than Gaussians with rows = None: the ids beyond the table are dropped on the device, the rest is unchanged
    few = 100
    big = torch.full((few + 6, D + 1), SENTINEL, dtype=torch.int64, device=gpu_device)
    big[3:3 + few].zero_()
    rows = torch.arange(r["P"], device=gpu_device, dtype=torch.int32)                  # int32: handed to the kernel as it is
    R.feature_votes(r["kept"], F, valid=valid, rows=rows, num_rows=few, out=big[3:3 + few])
    assert torch.equal(big[3:3 + few], r["votes"][:few]) and bool((big[:3] == SENTINEL).all()) and bool((big[3 + few:] == SENTINEL).all())


def _raw_args(r, dev):
    from opengaussian_amd import _lib
    kept = r["kept"]
    a = _lib.OgsRasterFwdArgs()
    a.P, a.W, a.H, a.C = r["P"], vc.W, vc.H, int(kept["Cn"])
    a.image_buffer, a.sorted_rec, a.quad_list = (_lib.ptr(kept[k]) for k in ("image", "sorted_rec", "quad_list"))
    return a


def test_raw_c_abi_with_rows_and_mask_bytes_at_the_edges_of_their_ranges(gpu_device):
    """int32 rows at 0, R - 1, R, -1, INT32_MAX and INT32_MIN and mask bytes 1, 2, 128 and 255 reach the kernel as they are"""
    from opengaussian_amd import _lib
    r = _run("P1500_b+1_masked", gpu_device)
    D, P, Rn = r["D"], r["P"], vc.LEAF_ROWS
    edge = torch.tensor([0, Rn - 1, Rn, -1, 2 ** 31 - 1, -2 ** 31, Rn + 1, 3], dtype=torch.int32)
    rows = edge[torch.arange(P) % len(edge)].to(gpu_device).contiguous()
    g = torch.Generator().manual_seed(5)
    nonzero = torch.tensor([1, 2, 128, 255], dtype=torch.uint8)[torch.randint(0, 4, (vc.H, vc.W), generator=g)].to(gpu_device)
    mask = torch.where(r["valid"], nonzero, torch.zeros_like(nonzero)).contiguous()
    pad = 2
    big = torch.full((Rn + 2 * pad, D + 1), SENTINEL, dtype=torch.int64, device=gpu_device)
    big[pad:pad + Rn].zero_()
    fv = _lib.OgsFeatureVotesArgs()
    fv.features, fv.num_channels, fv.valid = _lib.ptr(r["F"]), D, _lib.ptr(mask)
    fv.rows, fv.num_rows, fv.votes = _lib.ptr(rows), Rn, big[pad:].data_ptr()
    a = _raw_args(r, gpu_device)
    assert _lib.lib().ogs_raster_feature_votes(C.byref(a), C.byref(fv), torch.cuda.current_stream().cuda_stream) == 0
    ok = (rows >= 0) & (rows < Rn)
    want = torch.zeros(Rn, D + 1, dtype=torch.int64, device=gpu_device).index_add_(0, rows[ok].to(torch.int64), r["votes"][ok])
    assert torch.equal(big[pad:pad + Rn], want) and bool(want[0].any()) and bool(want[Rn - 1].any())
    assert bool((big[:pad] == SENTINEL).all()) and bool((big[pad + Rn:] == SENTINEL).all())


def test_bad_arguments_raise_on_the_host(gpu_device):
    from opengaussian_amd import _lib
    from opengaussian_amd import rasterizer as R
    r = _run("P300_3_masked", gpu_device)
    D, F, valid, kept, P = r["D"], r["F"], r["valid"], r["kept"], r["P"]
    with pytest.raises(RuntimeError, match="24 x 40"):
        R.feature_votes(kept, F[:, :, :-1])
    with pytest.raises(RuntimeError, match="24 x 40"):
        R.feature_votes(kept, F.permute(0, 2, 1).contiguous())
    with pytest.raises(RuntimeError, match="24 x 40"):
        R.feature_votes(kept, F, valid=valid[:-1])
    with pytest.raises(RuntimeError, match="floating"):
        R.feature_votes(kept, F.to(torch.int64))
    with pytest.raises(RuntimeError, match="num_rows"):
        R.feature_votes(kept, F, rows=r["rows"], num_rows=0)
    with pytest.raises(RuntimeError, match="Gaussians"):
        R.feature_votes(kept, F, rows=r["rows"][:-1], num_rows=vc.LEAF_ROWS)
    with pytest.raises(RuntimeError, match="out must be"):
        R.feature_votes(kept, F, out=torch.zeros(P, D, dtype=torch.int64, device=gpu_device))
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.feature_votes(kept, F.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.feature_votes(kept, F, valid=valid.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.feature_votes(kept, F, rows=r["rows"].cpu(), num_rows=vc.LEAF_ROWS)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.feature_votes(kept, F, out=torch.zeros(P, D + 1, dtype=torch.int64))
    # the C ABI: NULL pointers, R < 1, D < 1 and a grouped pass are codes from the host side, with a real pass behind them
    lib = _lib.lib()
    a = _raw_args(r, gpu_device)
    table = torch.zeros(P, D + 1, dtype=torch.int64, device=gpu_device)
    mask = valid.to(torch.uint8).contiguous()
    fv = _lib.OgsFeatureVotesArgs()
    fv.features, fv.num_channels, fv.valid, fv.rows, fv.num_rows, fv.votes = _lib.ptr(F), D, _lib.ptr(mask), None, P, _lib.ptr(table)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: lib.ogs_raster_feature_votes(C.byref(a), C.byref(fv), stream)
    for obj, field, bad in ((fv, "num_rows", 0), (fv, "num_channels", 0), (fv, "num_channels", -3), (fv, "features", None),
                            (fv, "votes", None), (a, "image_buffer", None), (a, "sorted_rec", None), (a, "quad_list", None),
                            (a, "num_groups", 2), (a, "P", 0), (a, "C", 5)):
        saved = getattr(obj, field)
        setattr(obj, field, bad)
        assert call() < 0, field
        setattr(obj, field, saved)
    assert not bool(table.any())
    assert call() == 0 and torch.equal(table, r["votes"])


# ---- 3. against the float64 restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_votes_against_the_float64_restatement(gpu_device, name):
    from opengaussian_amd import query
    r = _run(name, gpu_device)
    hooks = _hooks()
    got = query.votes_as_float(r["votes"]).cpu().numpy()
    want = fc.oracle(name, *hooks)
    worst = helpers.assert_grads_close_modulo_threshold_flips(got, want, fc.GRAD_BAR, want_fp32=lambda: fc.oracle_fp32(name, *hooks),
                                                              what=name)
    print(name, "D", r["D"], "table max", float(np.abs(want).max()), "largest error of the rows held to the bar / table max", worst)
    if name.startswith("wide"):
        # the small Gaussians against their own maximum: the wide ones own the table's
        small = slice(0, 300)
        worst = helpers.assert_grads_close_modulo_threshold_flips(got[small], want[small], fc.GRAD_BAR, what=name + " small rows",
                                                                  want_fp32=lambda: fc.oracle_fp32(name, *hooks)[small])
        print(name, "small rows: max", float(np.abs(want[small]).max()), "largest error / that max", worst)


def test_features_from_votes_against_the_restatement(gpu_device):
    from opengaussian_amd import query
    name = "P1500_f+1_masked"
    r = _run(name, gpu_device)
    feat, weight = query.features_from_votes(r["votes"], min_weight=0.05)
    # the same table through the restatement's row loop: the same float64 operations
    want_feat, want_weight = fr.features_from_table(r["votes"].cpu().numpy().astype(np.float64) / Q, min_weight=0.05)
    np.testing.assert_array_equal(feat.cpu().numpy(), want_feat)
    np.testing.assert_array_equal(weight.cpu().numpy(), want_weight)
    assert 0 < int((want_weight > 0.05).sum()) < r["P"] and bool((feat[weight <= 0.05] == 0).all())
    # against the float64 table of the restatement on the rows with at least a quarter pixel of weight that it holds to the
    # bar: d(s / w) <= (ds + |s / w| dw) / w with ds, dw <= GRAD_BAR of the table maximum
    o = fc.oracle(name, *_hooks())
    o_feat, o_weight = fr.features_from_table(o, min_weight=0.05)
    bar = fc.GRAD_BAR * np.abs(o).max()
    held = (np.abs(query.votes_as_float(r["votes"]).cpu().numpy() - o).max(axis=1) <= bar) & (o_weight >= 0.25) & (want_weight > 0.05)
    assert held.sum() >= 30                                # 36 rows of the masked P1500 scene carry a whole pixel of weight
    tol = bar * (1 + np.abs(o_feat).max(axis=1)) / o_weight.clip(1e-30)
    err = np.abs(feat.cpu().numpy() - o_feat).max(axis=1)
    print("features_from_votes: rows", int(held.sum()), "largest error / its tolerance", float((err[held] / tol[held]).max()))
    assert (err[held] <= tol[held]).all()


# ---- 4. against the device's existing route ------------------------------------------------------------------------------------------
def _backward_route(sc, cam, F, valid, dev):
    """the table through the drop-in rasterizer: colours [P, 9] the only input that requires grad, upstream planes v * F[c] and
    v, ceil((D + 1) / 9) features-only backward calls"""
    from opengaussian_amd.rasterizer import GaussianRasterizer
    s = sc.to(dev)
    P, D = s.means3D.shape[0], F.shape[0]
    v = torch.ones(vc.H, vc.W, device=dev) if valid is None else valid.to(torch.float32)
    planes = torch.cat([F * v[None], v[None], torch.zeros(8, vc.H, vc.W, device=dev)])
    rast = GaussianRasterizer(helpers.settings_for(cam, (0.0,) * 9, 0, dev))
    cols = torch.zeros(P, 9, device=dev, requires_grad=True)
    color = rast(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities, colors_precomp=cols,
                 scales=s.scales, rotations=s.rotations)[0]
    table = torch.zeros(P, D + 1, dtype=torch.float32, device=dev)
    for c0 in range(0, D + 1, 9):
        (g,) = torch.autograd.grad(color, cols, planes[c0:c0 + 9].contiguous(), retain_graph=True)
        n = min(9, D + 1 - c0)
        table[:, c0:c0 + n] = g[:, :n]
    return table


@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_votes_against_the_backward_route(gpu_device, name):
    from opengaussian_amd import query
    r = _run(name, gpu_device)
    c = r["case"]
    route = _backward_route(c["sc"], c["cam"], r["F"], r["valid"], gpu_device).to(torch.float64)
    got = query.votes_as_float(r["votes"])
    # the weights are the same bits on both sides; the sums differ: two fp32 sums over at most 64 terms, 2 * 63 * 2^-24 = 7.5e-6
    # of the summed magnitudes, which the lift of |F| gives per row
    bar = 1e-5 * query.votes_as_float(r["magnitude"]).sum(dim=1, keepdim=True) + 2.0 ** -30
    ratio = ((got - route).abs() / bar).max()
    print(name, "D", r["D"], "largest |votes - backward route| in units of the bar (1e-5 of the row's total of |F| + 2^-30):", float(ratio),
          "absolute:", float((got - route).abs().max()))
    assert float(ratio) <= 1.0


# ---- 5. sums -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_sum_of_the_weight_column_is_the_valid_alpha(gpu_device, name):
    from opengaussian_amd import query
    r = _run(name, gpu_device)
    valid = r["valid"] if r["valid"] is not None else torch.ones(vc.H, vc.W, dtype=torch.bool, device=gpu_device)
    total = float(query.votes_as_float(r["votes"][:, r["D"]]).sum())
    alpha = float(r["alpha"].to(torch.float64)[valid].sum())
    print(name, "sum of the weight column", total, "sum of alpha over the valid pixels", alpha)
    assert alpha > 10 and abs(total - alpha) <= 1e-4 * int(valid.sum())


@pytest.mark.parametrize("scene", ["P300", "P1500", "wide"])
@pytest.mark.parametrize("masked", [False, True])
def test_constant_planes_give_the_constant_times_the_weight(gpu_device, scene, masked):
    from opengaussian_amd import query
    from opengaussian_amd import rasterizer as R
    _, kept, _ = _pass(scene, gpu_device)
    k = torch.tensor([0.3, -1.7, 3.25], device=gpu_device)
    F = k[:, None, None].expand(3, vc.H, vc.W)
    t = query.votes_as_float(R.feature_votes(kept, F, valid=fc.valid_mask().to(gpu_device) if masked else None))
    bar = fc.GRAD_BAR * float(t.abs().max())
    err = float((t[:, :3] - t[:, 3:] * k.double()[None]).abs().max())
    print(scene, masked, "largest |column - constant * weight| / the bar", err / bar)
    assert float(t[:, 3].max()) > 0.5 and err <= bar


# ---- 6. the per-mask route as the cross-check, lift_features -----------------------------------------------------------------------
def _second_camera():
    Rm, t = helpers.POSES["roll_180"]
    return helpers.general_camera(vc.W, vc.H, vc.F, vc.F, Rm, t)


@pytest.mark.parametrize("L", [5, 70])
@pytest.mark.parametrize("by_leaf", [False, True])
def test_lift_features_agrees_with_lift_mask_features(gpu_device, L, by_leaf):
    """F(p) = M[lab(p)] on the masked pixels: the dense kernel against one label_votes launch per view and a matmul"""
    from opengaussian_amd import query
    fold, _ = _hooks()
    D = fold + 1
    sc, cam = vc.scene("P1500")
    model = _model_of(sc, gpu_device)
    cams = [cam.to(gpu_device), _second_camera().to(gpu_device)]
    g = torch.Generator().manual_seed(100 + L)
    M = [torch.randn(L, D, generator=g).to(gpu_device), torch.randn(L, D, generator=g).to(gpu_device)]
    labs = [vc.label_image("noise", L)[0].to(gpu_device), (vc.label_image("blocks4", 23)[0] % L).to(gpu_device)]
    masks = [(lab >= 0) & (lab < L) for lab in labs]
    feats = [torch.where(ok[None], m[lab.clamp(0, L - 1)].permute(2, 0, 1), torch.full((), 9.0, device=gpu_device)).contiguous()
             for lab, ok, m in zip(labs, masks, M)]
    kw = dict(rows=vc.leaf_rows(1500).to(gpu_device), num_rows=vc.LEAF_ROWS) if by_leaf else {}
    bg = torch.zeros(3, device=gpu_device)
    with torch.no_grad():
        dense = query.votes_as_float(query.lift_features(cams, model, PIPE, bg, 0, feats, valid_images=masks, **kw))
        feat_sum, weight = query.lift_mask_features(cams, model, PIPE, bg, 0, labs, M, **kw)
    assert feat_sum.dtype == torch.float64 and feat_sum.shape == (dense.shape[0], D) and weight.shape == (dense.shape[0],)
    bar = fc.GRAD_BAR * float(dense.abs().max())
    err_f, err_w = float((dense[:, :D] - feat_sum).abs().max()), float((dense[:, D] - weight).abs().max())
    print("L", L, "by leaf", by_leaf, "table max", float(dense.abs().max()), "errors / bar", err_f / bar, err_w / bar)
    assert float(weight.max()) > 0.5 and err_f <= bar and err_w <= bar
    # the means of the two routes where there is a pixel's worth of weight: sums and weights within `bar` of each other give
    # |s_a / w_a - s_b / w_b| <= bar * (1 + |mean|) / w to first order; twice that covers the second order
    mean_a, w_a = query.features_from_votes(query.lift_features(cams, model, PIPE, bg, 0, feats, valid_images=masks, **kw), min_weight=1.0)
    seen = w_a > 1.0
    mean_b = feat_sum[seen] / weight[seen][:, None]
    assert bool(seen.any()) and float((mean_a[seen] - mean_b).abs().max()) <= 2 * bar * (1 + float(mean_b.abs().max()))


def test_lift_features_over_two_cameras(gpu_device, kept_cache):
    from opengaussian_amd import query
    from opengaussian_amd.renderer import render
    from tests.test_3a_label_votes_gpu import _pass_of_model
    R = kept_cache
    _, block = _hooks()
    D = block + 1
    sc, cam = vc.scene("P1500")
    model = _model_of(sc, gpu_device)
    cams = [cam.to(gpu_device), _second_camera().to(gpu_device)]
    feats = [fc.features(D).to(gpu_device), fc.features(D, seed=1).to(gpu_device)]
    masks = [None, fc.valid_mask().to(gpu_device)]
    bg = torch.zeros(3, device=gpu_device)
    rows = vc.leaf_rows(1500).to(gpu_device)
    singles = [R.feature_votes(_pass_of_model(model, c, gpu_device), f, valid=m) for c, f, m in zip([cam, _second_camera()], feats, masks)]
    assert bool(singles[1].any()) and not torch.equal(singles[0], singles[1]), "the second camera sees the scene too"
    fresh = query.lift_features(cams, model, PIPE, bg, 0, feats, valid_images=masks)
    assert fresh.dtype == torch.int64 and torch.equal(fresh, singles[0] + singles[1])
    assert not R.KEPT_PASSES.slots and R.KEPT_PASSES.stats["admitted"] == 0, "the call admits nothing"
    by_rows = query.lift_features(cams, model, PIPE, bg, 0, feats, valid_images=masks, rows=rows, num_rows=vc.LEAF_ROWS)
    ok = (rows >= 0) & (rows < vc.LEAF_ROWS)
    assert torch.equal(by_rows, torch.zeros_like(by_rows).index_add_(0, rows[ok], fresh[ok]))
    # a frozen model: the passes render() kept are the source, and give the same table
    with torch.no_grad():
        for c in cams:
            render(c, model, PIPE, bg, 0, rescale=False)
        assert R.KEPT_PASSES.stats["admitted"] == 2
        stats = dict(R.KEPT_PASSES.stats)
        passes = dict(R.PASS_STATS)
        kept = query.lift_features(cams, model, PIPE, bg, 0, feats, valid_images=masks)
        mask_route = query.lift_mask_features(cams, model, PIPE, bg, 0, [vc.label_image("noise", 5)[0].to(gpu_device)] * 2,
                                              [torch.randn(5, 3, device=gpu_device)] * 2)
        assert R.KEPT_PASSES.stats == stats and len(R.KEPT_PASSES.slots) == 2
        assert R.PASS_STATS == passes, "no pass was run: the kept ones were walked"
    assert torch.equal(kept, fresh) and mask_route[0].shape == (1500, 3)
    # argument errors and forward only
    with pytest.raises(ValueError):
        query.lift_features(cams, model, PIPE, bg, 0, feats[:1])
    with pytest.raises(ValueError):
        query.lift_features(cams, model, PIPE, bg, 0, [feats[0], feats[1][:-1]])
    with pytest.raises(ValueError):
        query.lift_features(cams, model, PIPE, bg, 0, [feats[0], feats[1][:, :-1]])
    with pytest.raises(ValueError):
        query.lift_features(cams, model, PIPE, bg, 0, feats, valid_images=masks[:1])
    with pytest.raises(ValueError):
        query.lift_features(cams, model, PIPE, bg, 0, feats, rows=rows)
    with pytest.raises(ValueError):
        query.lift_mask_features(cams, model, PIPE, bg, 0, [masks[1].long()] * 2, [torch.randn(5, 3, device=gpu_device)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        query.lift_features(cams, model, PIPE, bg, 0, [f.cpu() for f in feats])
    model._xyz.requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward only"):
        query.lift_features(cams, model, PIPE, bg, 0, feats, valid_images=masks)
    with pytest.raises(RuntimeError, match="forward only"):
        query.lift_mask_features(cams, model, PIPE, bg, 0, [masks[1].long()] * 2, [torch.randn(2, 3, device=gpu_device)] * 2)
    with torch.no_grad():
        assert torch.equal(query.lift_features(cams, model, PIPE, bg, 0, feats, valid_images=masks), fresh)
