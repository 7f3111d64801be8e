"""GPU: the feature map (ogs_raster_feature_map, rasterizer.feature_map, query.render_feature_map): the exact equalities a map
without atomics promises, the device's own route through ceil(D / 12) re-blends of a 12-channel kept pass (bit for bit), the
float64 restatement, the pass's alpha, the adjoint identity with the feature votes, the autograd route built on it, and its bounds.

Measured on the MI355X (figures printed by the tests): the largest error against the float64 restatement in units of the bar and
the two sides of the adjoint identity are recorded in DESIGN.md section 6m."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import feature_map_cases as mc
from tests import feature_map_restatement as mr
from tests import feature_votes_restatement as fr
from tests import helpers
from tests import label_votes_cases as vc
from tests import label_votes_restatement as vr
from tests.test_39_label_map_gpu import PIPE, _fresh_pass, _model_of, kept_cache  # noqa: F401  (kept_cache: a fixture)

pytestmark = pytest.mark.gpu

_RUNS: dict = {}
_PASSES: dict = {}
SENTINEL = -1.2345678e9


def _hooks():
    from opengaussian_amd import _lib
    return int(_lib.lib().ogs_feature_map_fold_columns()), int(_lib.lib().ogs_feature_map_block_columns())


def _pass(scene, dev):
    """per scene, once: the 3-channel kept pass in both layouts, its alpha, and a compacted 12-channel kept pass with a zero
    background for the re-blend route"""
    if scene not in _PASSES:
        from opengaussian_amd import rasterizer as R
        sc, cam = mc.scene(scene)
        (color, radii, depth, alpha), kept = _fresh_pass(sc, cam, dev)
        assert kept is not None
        kp = R.KeptPasses(budget_bytes=1 << 30)
        assert kp.admit("slot", "key", None, kept)
        s = sc.to(dev)
        P = s.means3D.shape[0]
        rs12 = helpers.settings_for(cam, (0.0,) * 12, 0, dev)
        sink: list = []
        R._RasterizeGaussians.apply(s.means3D, torch.zeros_like(s.means3D), None, torch.zeros(P, 12, device=dev), s.opacities,
                                    s.scales, s.rotations, None, rs12, 0, None, None, 1, sink, True)
        kp12 = R.KeptPasses(budget_bytes=1 << 30)
        assert sink and kp12.admit("slot", "key", None, sink[0])
        _PASSES[scene] = dict(alpha=alpha[0], kept=kept, entry=kp.slots["slot"], entry12=kp12.slots["slot"], rs12=rs12,
                              keep=(kp, kp12), sc=sc, cam=cam, P=P)
    return _PASSES[scene]


def _reblend_route(p, Xp):
    """[D, H, W]: ceil(D / 12) re-blends of the 12-channel kept pass over [P, 12] slices of the per-Gaussian features"""
    from opengaussian_amd import rasterizer as R
    P, D = Xp.shape
    planes = []
    with torch.no_grad():
        for c0 in range(0, D, 12):
            n = min(12, D - c0)
            cols = torch.zeros(P, 12, device=Xp.device)
            cols[:, :n] = Xp[:, c0:c0 + n]
            planes.append(R._ReblendKept.apply(cols, p["entry12"], p["rs12"])[0][:n].clone())
    return torch.cat(planes)


def _per_gaussian(X, rows, P):
    """X[rows] with a zero row where the row lies outside [0, R); X itself without rows"""
    if rows is None:
        return X
    ok = (rows >= 0) & (rows < X.shape[0])
    return torch.where(ok[:, None], X[rows.clamp(0, X.shape[0] - 1)], torch.zeros((), device=X.device))


def _run(name, dev):
    """everything the tests below compare, once per case"""
    if name in _RUNS:
        return _RUNS[name]
    from opengaussian_amd import rasterizer as R
    c = mc.case(name, *_hooks())
    p = _pass(c["scene"], dev)
    X = c["features"].to(dev)
    rows = None if c["rows"] is None else c["rows"].to(dev)
    fmap, alpha = R.feature_map(p["kept"], X, rows=rows, with_alpha=True)
    compact = R.feature_map(p["entry"], X, rows=rows)
    torch.cuda.synchronize()
    r = dict(case=c, D=c["D"], P=c["P"], H=c["H"], W=c["W"], p=p, X=X, rows=rows, map=fmap, alpha=alpha, compact=compact,
             Xp=_per_gaussian(X, rows, c["P"]))
    _RUNS[name] = r
    return r


# ---- 1. exact equalities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_exact_equalities(gpu_device, name):
    from opengaussian_amd import rasterizer as R
    r = _run(name, gpu_device)
    fold, block = _hooks()
    D, P, X, rows, fmap, kept = r["D"], r["P"], r["X"], r["rows"], r["map"], r["p"]["kept"]
    assert fmap.dtype == torch.float32 and fmap.shape == (D, r["H"], r["W"]) and bool(torch.isfinite(fmap).all())
    assert bool((fmap < 0).any()) and bool((fmap > 0).any())
    # 1. two runs; the pass's own layout against the compacted one of a KeptPasses entry
    assert torch.equal(fmap, R.feature_map(kept, X, rows=rows))
    assert torch.equal(fmap, r["compact"])
    # 2. channels_last is the planar map permuted, from both layouts, and brings the same alpha
    last, alpha_last = R.feature_map(kept, X, rows=rows, channels_last=True, with_alpha=True)
    assert last.shape == (r["H"], r["W"], D) and last.is_contiguous() and torch.equal(last.permute(2, 0, 1), fmap)
    assert torch.equal(R.feature_map(r["p"]["entry"], X, rows=rows, channels_last=True), last) and torch.equal(alpha_last, r["alpha"])
    # 3. a permutation of the channels permutes the planes
    perm = torch.randperm(D, generator=torch.Generator().manual_seed(D)).to(gpu_device)
    assert torch.equal(R.feature_map(kept, X[:, perm], rows=rows), fmap[perm])
    # 4. the channels split over several calls: at one column, at the fold's 16, at the walk's block, and both
    for cuts in ([1], [fold], [block], [fold, block]):
        cuts = [0] + [c for c in cuts if c < D] + [D]
        if len(cuts) < 3:
            continue
        parts = [R.feature_map(kept, X[:, a:b], rows=rows) for a, b in zip(cuts[:-1], cuts[1:])]
        assert torch.equal(torch.cat(parts), fmap), cuts
    # 5. rows = r with a table against rows = None with X[r]; a row outside [0, R) against a zero feature row
    assert torch.equal(R.feature_map(kept, r["Xp"]), fmap)
    if rows is None:
        assert torch.equal(R.feature_map(kept, X, rows=torch.arange(P, device=gpu_device)), fmap)
    else:
        ok = (rows >= 0) & (rows < X.shape[0])
        assert bool(ok.any()) and not bool(ok.all())
        padded = torch.cat([X, torch.zeros(1, D, device=gpu_device)])
        assert torch.equal(R.feature_map(kept, padded, rows=torch.where(ok, rows, torch.full_like(rows, X.shape[0]))), fmap)
        assert torch.equal(R.feature_map(kept, X, rows=torch.where(ok, rows, torch.full_like(rows, -1)).to(torch.int32)), fmap)
    # 6. -X negates the map; fp64 copies and a strided view of the features are the same features
    assert torch.equal(R.feature_map(kept, -X, rows=rows), -fmap)
    assert torch.equal(R.feature_map(kept, X.double(), rows=rows), fmap)
    assert torch.equal(R.feature_map(kept, X.t().contiguous().t(), rows=rows), fmap)


@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_alpha_is_the_pass_alpha_bit_for_bit(gpu_device, name):
    from opengaussian_amd import rasterizer as R
    r = _run(name, gpu_device)
    assert r["alpha"].shape == (r["H"], r["W"]) and torch.equal(r["alpha"], r["p"]["alpha"])
    labels = torch.zeros(r["P"], dtype=torch.int64, device=gpu_device)
    assert torch.equal(r["alpha"], R.label_map(r["p"]["kept"], labels, 1)[3])
    # rows that count nobody: a zero map and still the whole alpha
    nobody = torch.full((r["P"],), -1, dtype=torch.int64, device=gpu_device)
    zero, alpha = R.feature_map(r["p"]["entry"], r["X"][:1], rows=nobody, with_alpha=True)
    assert not bool(zero.any()) and torch.equal(alpha, r["alpha"])


# ---- 2. against the device's existing route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_map_equals_the_reblend_route_bit_for_bit(gpu_device, name):
    """the chain acc = fmaf(w, x, acc) in depth order from +0 is the forward blend's own; v_mfma_f32_16x16x4_f32 is that chain"""
    r = _run(name, gpu_device)
    route = _reblend_route(r["p"], r["Xp"])
    diff = (route - r["map"]).abs()
    print(name, "D", r["D"], "pixels that differ from the re-blend route:", int((diff > 0).any(dim=0).sum()), "largest difference",
          float(diff.max()), "map max", float(r["map"].abs().max()))
    assert torch.equal(route, r["map"])


# ---- 3. against the float64 restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_map_against_the_float64_restatement(gpu_device, name):
    """rows of the comparison = pixels: a pixel may miss the bar only where the fp32 restatement leaves the float64 one too (a
    1/255 or stop-rule flip), and then agrees with the fp32 one; the share of such pixels is capped as for the feature votes"""
    r = _run(name, gpu_device)
    hooks = _hooks()
    pix = lambda m: np.ascontiguousarray(np.asarray(m).reshape(r["D"], -1).T)
    want, want_alpha = mc.oracle(name, *hooks)
    worst = helpers.assert_grads_close_modulo_threshold_flips(pix(r["map"].cpu().numpy()), pix(want), mc.MAP_BAR, what=name,
                                                              want_fp32=lambda: pix(mc.oracle_fp32(name, *hooks)[0]))
    err_alpha = float(np.abs(r["alpha"].cpu().numpy() - want_alpha).max())
    print(name, "D", r["D"], "map max", float(np.abs(want).max()), "largest error of the pixels held to the bar / map max", worst,
          "= bar x", worst / mc.MAP_BAR, "alpha error", err_alpha)


@pytest.mark.parametrize("scene", mc.SCENES)
def test_constant_features_give_the_constant_times_alpha(gpu_device, scene):
    from opengaussian_amd import rasterizer as R
    p = _pass(scene, gpu_device)
    k = torch.tensor([0.3, -1.7, 3.25], device=gpu_device)
    for X, rows in ((k[None].expand(p["P"], 3), None), (k[None].expand(vc.LEAF_ROWS, 3), torch.zeros(p["P"], dtype=torch.int64, device=gpu_device))):
        fmap, alpha = R.feature_map(p["kept"], X, rows=rows, with_alpha=True)
        bar = mc.MAP_BAR * float(fmap.abs().max())
        err = float((fmap.double() - k.double()[:, None, None] * alpha.double()[None]).abs().max())
        print(scene, "largest |plane - constant * alpha| / the bar", err / bar)
        assert float(alpha.max()) > 0.9 and err <= bar


@pytest.mark.parametrize("P", [300, 1500])
def test_one_hot_features_give_the_label_map(gpu_device, P):
    """X = onehot(labels): the planes are the per-label weights, their argmax is label_map's label where the winner's margin
    over the runner-up exceeds the bar, and the winner's plane is label_map's weight at the bar"""
    from opengaussian_amd import rasterizer as R
    from tests import label_map_cases as lmc
    c = lmc.scene_case(P, 5)
    p = _pass(f"P{P}", gpu_device)
    labels, L = c["labels"].to(gpu_device), c["L"]
    ok = (labels >= 0) & (labels < L)
    onehot = (ok[:, None] & (labels.clamp(0, L - 1)[:, None] == torch.arange(L, device=gpu_device)[None])).to(torch.float32)
    planes = R.feature_map(p["kept"], onehot)
    by_rows = R.feature_map(p["kept"], torch.eye(L, device=gpu_device), rows=labels)       # the same through a [L, L] table
    assert torch.equal(planes, by_rows)
    label, weight, second, _ = R.label_map(p["kept"], labels, L)
    bar = mc.MAP_BAR * float(planes.max())
    decided = (weight - second) > bar
    assert int(decided.sum()) > 200
    assert torch.equal(planes.argmax(dim=0)[decided].to(torch.int32), label[decided])
    assert float((planes.max(dim=0).values - weight).abs().max()) <= bar
    assert not bool(planes[:, label < 0].any())


# ---- 4. the adjoint identity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P1500_3", "P1500_3_rows", "P1500_b+1", "P1500_b+1_rows", "odd_b+1_rows"])
def test_adjoint_identity_with_the_feature_votes(gpu_device, name):
    """sum(feature_map(X) * F) = sum(X * feature_votes(F)[:, :D]), both sides summed in float64 on the host"""
    from opengaussian_amd import query
    from opengaussian_amd import rasterizer as R
    r = _run(name, gpu_device)
    D, X, rows, kept = r["D"], r["X"], r["rows"], r["p"]["kept"]
    F = mc.upstream(D, H=r["H"], W=r["W"]).to(gpu_device)
    votes = R.feature_votes(kept, F, rows=rows, num_rows=None if rows is None else X.shape[0])
    lhs = float((r["map"].double().cpu() * F.double().cpu()).sum())
    rhs = float((X.double().cpu() * query.votes_as_float(votes)[:, :D].cpu()).sum())
    scale = float((R.feature_map(kept, X.abs(), rows=rows).double().cpu() * F.abs().double().cpu()).sum())
    print(name, "D", D, "sum(map * F)", lhs, "sum(X * votes)", rhs, "|difference| / (bar = 2e-4 of sum(map(|X|) * |F|))",
          abs(lhs - rhs) / (mc.GRAD_BAR * scale))
    assert scale > 100 and abs(lhs - rhs) <= mc.GRAD_BAR * scale


# ---- 5. autograd -----------------------------------------------------------------------------------------------------------------------
def _want_grad(sc, cam, G, rows, Rn, dtype=torch.float64):
    """the transpose applied to an upstream gradient G [D, H, W] by the float64 restatement of the feature votes"""
    t = fr.feature_table(sc, cam, np.asarray(G, np.float64), dtype=dtype)[:, :G.shape[0]]
    return t if rows is None else vr.rows_table(t, rows, Rn)


@pytest.mark.parametrize("by_rows", [False, True])
def test_render_feature_map_backward(gpu_device, kept_cache, by_rows):
    from opengaussian_amd import query
    sc, cam = mc.scene("P300")
    model, view = _model_of(sc, gpu_device), cam.to(gpu_device)
    bg = torch.zeros(3, device=gpu_device)
    P, D = 300, 3
    Rn = vc.LEAF_ROWS if by_rows else P
    rows = vc.leaf_rows(P) if by_rows else None
    rows_dev = None if rows is None else rows.to(gpu_device)
    G = mc.upstream(D)
    X = mc.features(Rn, D).to(gpu_device).requires_grad_(True)

    def grad_of(upstream, **kw):
        X.grad = None
        out = query.render_feature_map(view, model, PIPE, bg, 0, X, rows=rows_dev, **kw)
        assert isinstance(out, query.FeatureMap) and out.features.requires_grad and not out.alpha.requires_grad
        out.features.backward(upstream.to(gpu_device))
        return X.grad.clone(), out

    rows_np = None if rows is None else rows.numpy()
    check = lambda got, up, what: print(what, "largest error of the rows held to the bar / table max", helpers.assert_grads_close_modulo_threshold_flips(
        got.cpu().numpy(), _want_grad(sc, cam, up.numpy(), rows_np, Rn), mc.GRAD_BAR, what=what,
        want_fp32=lambda: _want_grad(sc, cam, up.numpy(), rows_np, Rn, dtype=torch.float32)))
    g1, out = grad_of(G)
    assert g1.dtype == torch.float32 and g1.shape == (Rn, D)
    check(g1, G, "upstream of magnitude 1")
    # a mean loss: the same RELATIVE bar, which the fixed-point table alone (quantum 2^-32) would not hold
    tiny = G * 1e-7
    g2, _ = grad_of(tiny)
    check(g2, tiny, "upstream of magnitude 1e-7")
    assert float((g2 / 1e-7 - g1).abs().max()) <= mc.GRAD_BAR * float(g1.abs().max())
    # two backward calls give the same bytes; a zero upstream gives zeros; a huge one stays finite
    assert torch.equal(grad_of(G)[0], g1)
    assert not bool(grad_of(torch.zeros_like(G))[0].any())
    g3, _ = grad_of(G * 1e12)
    assert bool(torch.isfinite(g3).all()) and float((g3 / 1e12 - g1).abs().max()) <= mc.GRAD_BAR * float(g1.abs().max())
    # channels_last: the same map permuted, the same gradient from the permuted upstream
    g4, last = grad_of(G.permute(1, 2, 0).contiguous(), channels_last=True)
    assert torch.equal(last.features.permute(2, 0, 1), out.features) and torch.equal(g4, g1)
    # normalize: map / clamp(alpha, 1e-8) outside the Function, so the upstream that reaches it is G / clamp(alpha)
    g5, norm = grad_of(G, normalize=True)
    alpha = out.alpha.detach()
    assert torch.equal(norm.features.detach(), out.features.detach() / alpha.clamp_min(1e-8)[None])
    seen = (alpha > 0.05).cpu()                                        # where alpha is tiny the quotient amplifies its rounding
    g6, _ = grad_of(torch.where(seen[None], G, torch.zeros(())), normalize=True)
    check(g6, torch.where(seen[None], G / alpha.cpu().clamp_min(1e-8)[None], torch.zeros(())), "normalize=True")
    assert bool(torch.isfinite(g5).all())
    g7, _ = grad_of(torch.where(seen[None], G, torch.zeros(())).permute(1, 2, 0).contiguous(), normalize=True, channels_last=True)
    assert torch.equal(g7, g6)


def test_render_feature_map_over_a_kept_pass_equals_a_fresh_one(gpu_device, kept_cache):
    from opengaussian_amd import query
    from opengaussian_amd.renderer import render
    R = kept_cache
    sc, cam = mc.scene("P1500")
    model, view = _model_of(sc, gpu_device), cam.to(gpu_device)
    bg = torch.zeros(3, device=gpu_device)
    _, block = _hooks()
    X = mc.features(vc.LEAF_ROWS, block + 1).to(gpu_device)
    rows = vc.leaf_rows(1500).to(gpu_device)
    with torch.no_grad():
        fresh = query.render_feature_map(view, model, PIPE, bg, 0, X, rows=rows)
        assert not R.KEPT_PASSES.slots and R.KEPT_PASSES.stats["admitted"] == 0, "the call admits nothing"
        out = render(view, model, PIPE, bg, 0, rescale=False)
        assert R.KEPT_PASSES.stats["admitted"] == 1
        stats, passes = dict(R.KEPT_PASSES.stats), dict(R.PASS_STATS)
        entry = next(iter(R.KEPT_PASSES.slots.values()))
        kept = query.render_feature_map(view, model, PIPE, bg, 0, X, rows=rows)
        assert R.KEPT_PASSES.stats == stats and len(R.KEPT_PASSES.slots) == 1
        assert R.PASS_STATS == passes, "no pass was run: the kept one was walked"
    assert torch.equal(fresh.features, kept.features) and torch.equal(fresh.alpha, kept.alpha)
    assert torch.equal(kept.alpha, out["alpha"][0]) and torch.equal(kept.features, R.feature_map(entry, X, rows=rows))
    # relevancy on top of it, both layouts
    text = mc.features(4, block + 1, seed=3).to(gpu_device)
    canon = mc.features(3, block + 1, seed=4).to(gpu_device)
    with torch.no_grad():
        last = query.render_feature_map(view, model, PIPE, bg, 0, X, rows=rows, channels_last=True)
    rel = query.relevancy_maps(kept.features, text, canon)
    assert rel.shape == (4, mc.H, mc.W) and float(rel.min()) >= 0 and float(rel.max()) <= 1
    assert float((rel - query.relevancy_maps(last.features, text, canon, channels_last=True, chunk=77)).abs().max()) <= 1e-5
    # argument errors and the geometry's rule
    with pytest.raises(ValueError):
        query.render_feature_map(view, model, PIPE, bg, 0, X)                          # R != P without rows
    with pytest.raises(ValueError):
        query.render_feature_map(view, model, PIPE, bg, 0, X, rows=rows[:-1])
    with pytest.raises(ValueError):
        query.render_feature_map(view, model, PIPE, bg, 0, X.long(), rows=rows)
    with pytest.raises(RuntimeError, match="no CPU path"):
        query.render_feature_map(view, model, PIPE, bg, 0, X.cpu(), rows=rows)
    model._xyz.requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward only"):
        query.render_feature_map(view, model, PIPE, bg, 0, X, rows=rows)
    with torch.no_grad():
        assert torch.equal(query.render_feature_map(view, model, PIPE, bg, 0, X, rows=rows).features, fresh.features)


# ---- 6. bounds -------------------------------------------------------------------------------------------------------------------------
def _raw_args(r):
    from opengaussian_amd import _lib
    kept = r["p"]["kept"]
    a = _lib.OgsRasterFwdArgs()
    a.P, a.W, a.H, a.C = r["P"], r["W"], r["H"], int(kept["Cn"])
    a.image_buffer, a.sorted_rec, a.quad_list = (_lib.ptr(kept[k]) for k in ("image", "sorted_rec", "quad_list"))
    return a


@pytest.mark.parametrize("name", ["P1500_2b+1_rows", "odd_b+1_rows", "odd_3", "wide_b+1"])
@pytest.mark.parametrize("channels_last", [False, True])
def test_nothing_is_written_outside_the_outputs(gpu_device, name, channels_last):
    """the raw C ABI with sentinel planes / pixels around out_map and out_alpha, int32 rows at the edges of their range; with the
    odd image the pixels beyond W and H of the cut quadrants would land in the next row, the next plane or the guard"""
    from opengaussian_amd import _lib
    r = _run(name, gpu_device)
    D, P, H, W = r["D"], r["P"], r["H"], r["W"]
    Rn = vc.LEAF_ROWS
    X = mc.features(Rn, D, seed=9).to(gpu_device)
    edge = torch.tensor([0, Rn - 1, Rn, -1, 2 ** 31 - 1, -2 ** 31, Rn + 1, 3], dtype=torch.int32)
    rows = edge[torch.arange(P) % len(edge)].to(gpu_device).contiguous()
    guard = 2 * H * W + 64                                             # floats in front of and behind the map: a multiple of four
    big = torch.full((guard + D * H * W + guard,), SENTINEL, dtype=torch.float32, device=gpu_device)
    big_alpha = torch.full((3, H, W), SENTINEL, dtype=torch.float32, device=gpu_device)
    fm = _lib.OgsFeatureMapArgs()
    fm.features, fm.num_channels, fm.rows, fm.num_rows = _lib.ptr(X), D, _lib.ptr(rows), Rn
    fm.channels_last, fm.out_map, fm.out_alpha = int(channels_last), big[guard:].data_ptr(), big_alpha[1].data_ptr()
    a = _raw_args(r)
    assert _lib.lib().ogs_raster_feature_map(C.byref(a), C.byref(fm), torch.cuda.current_stream().cuda_stream) == 0
    got = big[guard:guard + D * H * W].reshape((H, W, D) if channels_last else (D, H, W))
    from opengaussian_amd import rasterizer as R
    ok = (rows >= 0) & (rows < Rn)
    want = R.feature_map(r["p"]["kept"], _per_gaussian(X, rows.to(torch.int64), P), channels_last=channels_last)
    assert bool(ok.any()) and torch.equal(got, want) and bool(want.any())
    assert bool((big[:guard] == SENTINEL).all()) and bool((big[guard + D * H * W:] == SENTINEL).all())
    assert torch.equal(big_alpha[1], r["alpha"]) and bool((big_alpha[0] == SENTINEL).all()) and bool((big_alpha[2] == SENTINEL).all())
    # out_alpha == NULL: the map alone; a map at an address that is no multiple of 16 bytes (the 4-byte planar stores)
    big.fill_(SENTINEL)
    fm.out_map, fm.out_alpha = big[guard + 1:].data_ptr(), None
    assert _lib.lib().ogs_raster_feature_map(C.byref(a), C.byref(fm), torch.cuda.current_stream().cuda_stream) == 0
    assert torch.equal(big[guard + 1:guard + 1 + D * H * W].reshape(got.shape), want)
    assert bool((big[:guard + 1] == SENTINEL).all()) and bool((big[guard + 1 + D * H * W:] == SENTINEL).all())


def test_bad_arguments_raise_on_the_host(gpu_device):
    from opengaussian_amd import _lib
    from opengaussian_amd import rasterizer as R
    r = _run("P300_3_rows", gpu_device)
    D, X, rows, kept, P = r["D"], r["X"], r["rows"], r["p"]["kept"], r["P"]
    with pytest.raises(RuntimeError, match="300 Gaussians"):
        R.feature_map(kept, X)                                         # [7, 3] without rows
    with pytest.raises(RuntimeError, match="300 Gaussians"):
        R.feature_map(kept, X, rows=rows[:-1])
    with pytest.raises(RuntimeError, match="floating"):
        R.feature_map(kept, X.to(torch.int64), rows=rows)
    with pytest.raises(RuntimeError, match="D >= 1"):
        R.feature_map(kept, X[:, :0], rows=rows)
    with pytest.raises(RuntimeError, match="integer"):
        R.feature_map(kept, X, rows=rows.float())
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.feature_map(kept, X.cpu(), rows=rows)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.feature_map(kept, X, rows=rows.cpu())
    with pytest.raises(RuntimeError, match="ungrouped streaming pass"):
        R.feature_map(None, X, rows=rows)
    # the C ABI: NULL pointers, R < 1, D < 1, a grouped pass and C outside {3, 6, 9, 12} are codes from the host side, with a real
    # pass behind them; nothing was written
    lib = _lib.lib()
    a = _raw_args(r)
    out = torch.full((D, r["H"], r["W"]), SENTINEL, dtype=torch.float32, device=gpu_device)
    row32 = torch.where((rows >= 0) & (rows < X.shape[0]), rows, torch.full_like(rows, -1)).to(torch.int32).contiguous()
    fm = _lib.OgsFeatureMapArgs()
    fm.features, fm.num_channels, fm.rows, fm.num_rows, fm.out_map = _lib.ptr(X), D, _lib.ptr(row32), X.shape[0], _lib.ptr(out)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: lib.ogs_raster_feature_map(C.byref(a), C.byref(fm), stream)
    for obj, field, bad in ((fm, "num_rows", 0), (fm, "num_channels", 0), (fm, "num_channels", -3), (fm, "features", None),
                            (fm, "out_map", None), (a, "image_buffer", None), (a, "sorted_rec", None), (a, "quad_list", None),
                            (a, "num_groups", 2), (a, "P", 0), (a, "C", 5)):
        saved = getattr(obj, field)
        setattr(obj, field, bad)
        assert call() < 0, field
        setattr(obj, field, saved)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call() == 0 and torch.equal(out, r["map"])
