"""GPU: the label votes (ogs_raster_label_votes, rasterizer.label_votes, query.lift_labels and the table helpers): the exact
integer equalities the fixed-point table promises, its bounds, the float64 restatement, the device's own one-hot route through
the features-only backward, the pass's alpha, and the mask-prompt route end to end.

Measured on the MI355X (figures printed by the tests): the largest error against the float64 restatement on rows held to the
bar, and the largest cell difference against the one-hot route in units of its bar, are recorded in DESIGN.md section 6k."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers
from tests import label_votes_cases as vc
from tests import label_votes_restatement as vr
from tests.test_39_label_map_gpu import PIPE, _fresh_pass, _model_of, kept_cache  # noqa: F401  (kept_cache: a fixture)

pytestmark = pytest.mark.gpu

_RUNS: dict = {}
Q = 1 << 32


def _hooks():
    from opengaussian_amd import _lib
    return int(_lib.lib().ogs_label_votes_fold_columns()), int(_lib.lib().ogs_label_votes_quadrant_capacity())


def _case(name):
    return vc.case(name, *_hooks())


def _run(name, dev):
    """everything the tests below compare, once per case"""
    if name in _RUNS:
        return _RUNS[name]
    from opengaussian_amd import rasterizer as R
    c = _case(name)
    (color, radii, depth, alpha), kept = _fresh_pass(c["sc"], c["cam"], dev)
    assert kept is not None
    img = c["image"].to(dev)
    P = c["sc"].means3D.shape[0]
    votes = R.label_votes(kept, img, c["L"])
    kp = R.KeptPasses(budget_bytes=1 << 30)
    assert kp.admit("slot", "key", None, kept)
    entry = kp.slots["slot"]
    compact = R.label_votes(entry, img, c["L"])
    rows = vc.leaf_rows(P).to(dev)
    by_rows = R.label_votes(kept, img, c["L"], rows=rows, num_rows=vc.LEAF_ROWS)
    torch.cuda.synchronize()
    r = dict(case=c, alpha=alpha[0], kept=kept, entry=entry, img=img, votes=votes, compact=compact, rows=rows, by_rows=by_rows, P=P)
    _RUNS[name] = r
    return r


# ---- 1. exact equalities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_exact_integer_equalities(gpu_device, name):
    from opengaussian_amd import rasterizer as R
    r = _run(name, gpu_device)
    c, L, P, img, votes = r["case"], r["case"]["L"], r["P"], r["img"], r["votes"]
    assert votes.dtype == torch.int64 and votes.shape == (P, L + 1) and bool((votes >= 0).all()) and bool(votes.any())
    # two runs into fresh tables
    assert torch.equal(votes, R.label_votes(r["kept"], img, L))
    # the pass's own layout against the compacted one of a KeptPasses entry
    assert torch.equal(votes, r["compact"])
    # rows = r against index_add of rows = None (-1 and >= R dropped), from both layouts
    rows = r["rows"]
    ok = (rows >= 0) & (rows < vc.LEAF_ROWS)
    want = torch.zeros(vc.LEAF_ROWS, L + 1, dtype=torch.int64, device=gpu_device).index_add_(0, rows[ok], votes[ok])
    assert torch.equal(r["by_rows"], want)
    assert torch.equal(R.label_votes(r["entry"], img, L, rows=rows, num_rows=vc.LEAF_ROWS), want)
    assert bool(ok.any()) and not bool(ok.all())
    # an int32 image whose outside values are already -1 is the same image
    as32 = torch.where((img >= 0) & (img < L), img, torch.full_like(img, -1)).to(torch.int32)
    assert torch.equal(votes, R.label_votes(r["kept"], as32, L))
    # ... and so is the int32 image with its raw outside values (L, L + 3, -2, -7), which reach the kernel as they are
    assert torch.equal(votes, R.label_votes(r["kept"], img.to(torch.int32), L))
    # relabelling l -> 7 l + 3 permutes the columns; every other column of the wider table stays zero
    L2 = 7 * L + 4
    inside = (img >= 0) & (img < L)
    wider = R.label_votes(r["kept"], torch.where(inside, 7 * img + 3, torch.full_like(img, -1)), L2)
    want = torch.zeros(P, L2 + 1, dtype=torch.int64, device=gpu_device)
    want[:, 3:7 * L:7] = votes[:, :L]
    want[:, L2] = votes[:, L]
    assert torch.equal(wider, want)
    # two calls into one table give twice the table
    twice = R.label_votes(r["kept"], img, L)
    assert R.label_votes(r["kept"], img, L, out=twice) is twice
    assert torch.equal(twice, 2 * votes)
    if name.endswith("_null") or name.endswith("_L0"):
        assert not bool(votes[:, :L].any()) and bool(votes[:, L].any())


def test_wide_int64_values_stay_outside(gpu_device):
    """64-bit labels and rows outside the int32 range are outside, not wrapped into range"""
    from opengaussian_amd import rasterizer as R
    r = _run("P300_noise5", gpu_device)
    L, img = r["case"]["L"], r["img"]
    far = torch.where(img < 0, torch.full_like(img, (1 << 32) + 2), img)              # would wrap to label 2
    assert torch.equal(R.label_votes(r["kept"], far, L), r["votes"])
    rows = torch.arange(r["P"], device=gpu_device, dtype=torch.int64)
    rows[::2] += 1 << 32                                                              # would wrap to the row itself
    got = R.label_votes(r["kept"], img, L, rows=rows, num_rows=r["P"])
    want = r["votes"].clone()
    want[::2] = 0
    assert torch.equal(got, want)


# ---- 2. bounds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P1500_noise70", "wide_blocks8", "P1500_many4"])
def test_nothing_is_written_outside_the_table(gpu_device, name):
    from opengaussian_amd import rasterizer as R
    r = _run(name, gpu_device)
    L, img = r["case"]["L"], r["img"]
    sentinel = -0x0123456789ABCDEF
    for rows, Rn, want in ((None, r["P"], r["votes"]), (r["rows"], vc.LEAF_ROWS, r["by_rows"])):
        pad = 3
        big = torch.full((Rn + 2 * pad, L + 1), sentinel, dtype=torch.int64, device=gpu_device)
        table = big[pad:pad + Rn]
        table.zero_()
        R.label_votes(r["kept"], img, L, rows=rows, num_rows=None if rows is None else Rn, out=table)
        assert torch.equal(table, want)
        assert bool((big[:pad] == sentinel).all()) and bool((big[pad + Rn:] == sentinel).all())
    # fewer rows than Gaussians with rows = None: the ids beyond the table are dropped on the device, the rest is unchanged
    few = 100
    big = torch.full((few + 6, L + 1), sentinel, dtype=torch.int64, device=gpu_device)
    big[3:3 + few].zero_()
    rows = torch.arange(r["P"], device=gpu_device, dtype=torch.int32)                  # int32: handed to the kernel as it is
    R.label_votes(r["kept"], img, L, rows=rows, num_rows=few, out=big[3:3 + few])
    assert torch.equal(big[3:3 + few], r["votes"][:few]) and bool((big[:3] == sentinel).all()) and bool((big[3 + few:] == sentinel).all())


def test_bad_arguments_raise_on_the_host(gpu_device):
    from opengaussian_amd import _lib
    from opengaussian_amd import rasterizer as R
    r = _run("P300_noise5", gpu_device)
    L, img, kept, P = r["case"]["L"], r["img"], r["kept"], r["P"]
    with pytest.raises(RuntimeError, match="24 x 40"):
        R.label_votes(kept, img[:, :-1], L)
    with pytest.raises(RuntimeError, match="24 x 40"):
        R.label_votes(kept, img.t().contiguous(), L)
    with pytest.raises(RuntimeError, match="num_rows"):
        R.label_votes(kept, img, L, rows=r["rows"], num_rows=0)
    with pytest.raises(RuntimeError, match="num_labels"):
        R.label_votes(kept, img, -1)
    with pytest.raises(RuntimeError, match="Gaussians"):
        R.label_votes(kept, img, L, rows=r["rows"][:-1], num_rows=vc.LEAF_ROWS)
    with pytest.raises(RuntimeError, match="out must be"):
        R.label_votes(kept, img, L, out=torch.zeros(P, L, dtype=torch.int64, device=gpu_device))
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.label_votes(kept, img.cpu(), L)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.label_votes(kept, img, L, rows=r["rows"].cpu(), num_rows=vc.LEAF_ROWS)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.label_votes(kept, img, L, out=torch.zeros(P, L + 1, dtype=torch.int64))
    # the C ABI: NULL pointers, R < 1, L < 0 and a grouped pass are codes from the host side, with a real pass behind them
    lib = _lib.lib()
    a = _lib.OgsRasterFwdArgs()
    a.P, a.W, a.H, a.C = P, vc.W, vc.H, int(kept["Cn"])
    a.image_buffer, a.sorted_rec, a.quad_list = (_lib.ptr(kept[k]) for k in ("image", "sorted_rec", "quad_list"))
    lab = img.to(torch.int32).contiguous()
    table = torch.zeros(P, L + 1, dtype=torch.int64, device=gpu_device)
    lv = _lib.OgsLabelVotesArgs()
    lv.pixel_labels, lv.num_labels, lv.rows, lv.num_rows, lv.votes = _lib.ptr(lab), L, None, P, _lib.ptr(table)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: lib.ogs_raster_label_votes(C.byref(a), C.byref(lv), stream)
    for obj, field, bad in ((lv, "num_rows", 0), (lv, "num_labels", -1), (lv, "pixel_labels", None), (lv, "votes", None),
                            (a, "image_buffer", None), (a, "sorted_rec", None), (a, "quad_list", None), (a, "num_groups", 2),
                            (a, "P", 0), (a, "C", 5)):
        saved = getattr(obj, field)
        setattr(obj, field, bad)
        assert call() < 0, field
        setattr(obj, field, saved)
    assert not bool(table.any())
    assert call() == 0 and torch.equal(table, r["votes"])


# ---- 3. against the float64 restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_votes_against_the_float64_restatement(gpu_device, name):
    from opengaussian_amd import query
    r = _run(name, gpu_device)
    hooks = _hooks()
    got = query.votes_as_float(r["votes"]).cpu().numpy()
    want = vc.oracle(name, *hooks)
    worst = helpers.assert_grads_close_modulo_threshold_flips(got, want, vc.GRAD_BAR, want_fp32=lambda: vc.oracle_fp32(name, *hooks),
                                                              what=name)
    print(name, "table max", float(want.max()), "largest error of the rows held to the bar / table max", worst)
    if name.startswith("wide"):
        # the small Gaussians against their own maximum: the wide ones own the table's
        small = slice(0, 300)
        worst = helpers.assert_grads_close_modulo_threshold_flips(got[small], want[small], vc.GRAD_BAR, what=name + " small rows",
                                                                  want_fp32=lambda: vc.oracle_fp32(name, *hooks)[small])
        print(name, "small rows: max", float(want[small].max()), "largest error / that max", worst)


# ---- 4. against the device's own one-hot route -----------------------------------------------------------------------------------------
def _one_hot_route(sc, cam, image, L, dev):
    """the table through the drop-in rasterizer: colours [P, 9] the only input that requires grad, one-hot upstream planes,
    ceil((L + 1) / 9) features-only backward calls"""
    from opengaussian_amd.rasterizer import GaussianRasterizer
    s = sc.to(dev)
    P = s.means3D.shape[0]
    lab = torch.where((image >= 0) & (image < L), image, torch.full_like(image, L))
    rast = GaussianRasterizer(helpers.settings_for(cam, (0.0,) * 9, 0, dev))
    cols = torch.zeros(P, 9, device=dev, requires_grad=True)
    color = rast(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities, colors_precomp=cols,
                 scales=s.scales, rotations=s.rotations)[0]
    table = torch.zeros(P, L + 1, dtype=torch.float32, device=dev)
    ids = torch.arange(9, device=dev)[:, None, None]
    for c0 in range(0, L + 1, 9):
        planes = (lab[None] == ids + c0).to(torch.float32)
        (g,) = torch.autograd.grad(color, cols, planes, retain_graph=True)
        n = min(9, L + 1 - c0)
        table[:, c0:c0 + n] = g[:, :n]
    return table


@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_votes_against_the_one_hot_route(gpu_device, name):
    from opengaussian_amd import query
    r = _run(name, gpu_device)
    c = r["case"]
    route = _one_hot_route(c["sc"], c["cam"], r["img"], c["L"], gpu_device).to(torch.float64)
    got = query.votes_as_float(r["votes"])
    # the weights are the same bits on both sides; the sums differ: two fp32 sums over at most 64 pixels, 2 * 63 * 2^-24 = 7.5e-6
    bar = 1e-5 * route.sum(dim=1, keepdim=True) + 2.0 ** -30
    ratio = ((got - route).abs() / bar).max()
    print(name, "largest |votes - one-hot route| in units of the bar (1e-5 of the row's total + 2^-30):", float(ratio),
          "absolute:", float((got - route).abs().max()))
    assert float(ratio) <= 1.0


# ---- 5. against the pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_sum_of_the_table_is_the_sum_of_alpha(gpu_device, name):
    from opengaussian_amd import query
    r = _run(name, gpu_device)
    total = float(query.votes_as_float(r["votes"]).sum())
    alpha = float(r["alpha"].to(torch.float64).sum())
    print(name, "sum of the table", total, "sum of alpha", alpha)
    assert abs(total - alpha) <= 1e-4 * vc.W * vc.H
    # every column against the alpha over the pixels of its label
    lab = torch.where((r["img"] >= 0) & (r["img"] < r["case"]["L"]), r["img"], torch.full_like(r["img"], r["case"]["L"]))
    per_label = torch.zeros(r["case"]["L"] + 1, dtype=torch.float64, device=gpu_device).index_add_(
        0, lab.reshape(-1), r["alpha"].to(torch.float64).reshape(-1))
    cols = query.votes_as_float(r["votes"]).sum(dim=0)
    count = torch.bincount(lab.reshape(-1), minlength=r["case"]["L"] + 1)
    assert bool(((cols - per_label).abs() <= 1e-4 * count).all())


# ---- 6. labels_from_votes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.LABEL_CHECK)
def test_labels_from_votes_on_decided_rows(gpu_device, name):
    from opengaussian_amd import query
    r = _run(name, gpu_device)
    want = vc.oracle(name, *_hooks())
    o_label, o_weight, o_second, o_total = vr.labels_from_votes(want)
    decided = (o_label >= 0) & (o_weight - o_second > vc.DECIDED * want.max())
    label, weight, second, total = (t.cpu().numpy() for t in query.labels_from_votes(r["votes"]))
    print(name, "decided", int(decided.sum()), "of", int((o_label >= 0).sum()), "mismatches on decided rows",
          int((label[decided] != o_label[decided]).sum()))
    assert decided.sum() >= 0.9 * (o_label >= 0).sum()
    np.testing.assert_array_equal(label[decided], o_label[decided])
    # what the outputs say about themselves
    assert ((label >= 0) == (weight > 0)).all() and (second <= weight).all() and (weight <= total + 1e-12).all()


# ---- 7. a quadrant with many labels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in vc.CASE_NAMES if "many" in n])
def test_every_label_of_a_many_label_quadrant_is_folded(gpu_device, name):
    r = _run(name, gpu_device)
    c = r["case"]
    fold, cap = _hooks()
    lab = vc.clamp_labels(c["image"].numpy(), c["L"])
    quad = np.unique(lab[vc.QUAD_Y0:vc.QUAD_Y0 + 8, vc.QUAD_X0:vc.QUAD_X0 + 8])
    assert len(quad) == c["many"]
    cols = r["votes"].sum(dim=0).cpu().numpy()
    # every label of the quadrant, whichever column block of the fold it fell into, has a non-zero cell
    assert (cols[quad] > 0).all(), (c["many"], fold, quad[cols[quad] == 0])


# ---- 8. lift_labels and the mask prompts ---------------------------------------------------------------------------------------------------
def _second_camera():
    Rm, t = helpers.POSES["roll_180"]
    return helpers.general_camera(vc.W, vc.H, vc.F, vc.F, Rm, t)


def _pass_of_model(model, cam, dev):
    import types
    s = types.SimpleNamespace(means3D=model.get_xyz, opacities=model.get_opacity, scales=model.get_scaling, rotations=model.get_rotation)
    s.to = lambda dev: s
    return _fresh_pass(s, cam, dev)[1]


def test_lift_labels_over_two_cameras(gpu_device, kept_cache):
    from opengaussian_amd import query
    from opengaussian_amd.renderer import render
    R = kept_cache
    c = _case("P1500_noise70")
    model = _model_of(c["sc"], gpu_device)
    cams = [c["cam"].to(gpu_device), _second_camera().to(gpu_device)]
    images = [c["image"].to(gpu_device), vc.label_image("blocks4", 23)[0].to(gpu_device) * 3]
    L = 70
    bg = torch.zeros(3, device=gpu_device)
    rows = vc.leaf_rows(1500).to(gpu_device)
    singles = [R.label_votes(_pass_of_model(model, cam, gpu_device), img, L) for cam, img in zip([c["cam"], _second_camera()], images)]
    assert bool(singles[1].any()) and not torch.equal(singles[0], singles[1]), "the second camera sees the scene too"
    fresh = query.lift_labels(cams, model, PIPE, bg, 0, images, L)
    assert fresh.dtype == torch.int64 and torch.equal(fresh, singles[0] + singles[1])
    assert not R.KEPT_PASSES.slots and R.KEPT_PASSES.stats["admitted"] == 0, "the call admits nothing"
    by_rows = query.lift_labels(cams, model, PIPE, bg, 0, images, L, rows=rows, num_rows=vc.LEAF_ROWS)
    ok = (rows >= 0) & (rows < vc.LEAF_ROWS)
    assert torch.equal(by_rows, torch.zeros_like(by_rows).index_add_(0, rows[ok], fresh[ok]))
    # a frozen model: the passes render() kept are the source, and give the same table
    with torch.no_grad():
        for cam in cams:
            render(cam, model, PIPE, bg, 0, rescale=False)
        assert R.KEPT_PASSES.stats["admitted"] == 2
        stats = dict(R.KEPT_PASSES.stats)
        passes = dict(R.PASS_STATS)
        kept = query.lift_labels(cams, model, PIPE, bg, 0, images, L)
        assert R.KEPT_PASSES.stats == stats and len(R.KEPT_PASSES.slots) == 2
        assert R.PASS_STATS == passes, "no pass was run: the kept ones were walked"
    assert torch.equal(kept, fresh)
    # forward only
    with pytest.raises(ValueError):
        query.lift_labels(cams, model, PIPE, bg, 0, images[:1], L)
    with pytest.raises(ValueError):
        query.lift_labels(cams, model, PIPE, bg, 0, [images[0], images[1][:-1]], L)
    model._xyz.requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward only"):
        query.lift_labels(cams, model, PIPE, bg, 0, images, L)
    with torch.no_grad():
        assert torch.equal(query.lift_labels(cams, model, PIPE, bg, 0, images, L), fresh)


def test_select_leaves_by_masks_end_to_end(gpu_device):
    """leaves that follow the image (a 4 x 2 grid of 10 x 12 pixel cells): a block prompt over a cell returns that cell's leaf,
    and the selection goes through render_queries"""
    from opengaussian_amd import query
    c = _case("P1500_noise5")
    sc, cam = c["sc"], c["cam"].to(gpu_device)
    model = _model_of(sc, gpu_device)
    z = sc.means3D[:, 2].clamp_min(0.2)
    px = sc.means3D[:, 0] * vc.F / z + vc.W / 2 - 0.5
    py = sc.means3D[:, 1] * vc.F / z + vc.H / 2 - 0.5
    leaf = ((py / 12).floor().clamp(0, 1) * 4 + (px / 10).floor().clamp(0, 3)).to(torch.int64).to(gpu_device)
    prompts = torch.full((vc.H, vc.W), -1, dtype=torch.int64)
    prompts[0:12, 30:40] = 0                       # the cell of leaf 3
    prompts[12:24, 0:20] = 1                       # the cells of leaves 4 and 5
    bg = torch.zeros(3, device=gpu_device)
    with torch.no_grad():
        sel = query.select_leaves_by_masks([cam], model, PIPE, bg, 0, [prompts.to(gpu_device)], 2, leaf, 9)
        assert [s.tolist() for s in sel] == [[3], [4, 5]]
        out = query.render_queries(cam, model, PIPE, bg, 0, leaf, sel, root_num=4, leaf_num=2, post_process=False, better_vis=False)
        ref = query.render_queries(cam, model, PIPE, bg, 0, leaf, [torch.tensor([3], device=gpu_device), torch.tensor([4, 5], device=gpu_device)],
                                   root_num=4, leaf_num=2, post_process=False, better_vis=False)
    assert out.kept == [True, True] and out.counts == ref.counts
    assert torch.equal(out.images[0], ref.images[0]) and torch.equal(out.silhouettes[1], ref.silhouettes[1])
    # the silhouette of prompt 0's object lies under the prompt
    sil = out.silhouettes[0][0]
    assert float(sil[0:12, 30:40].sum()) > 0.8 * float(sil.sum())
