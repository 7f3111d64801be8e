"""The table of the stream contract tests (tests/stream_harness.py): one Case per public entry point that launches HIP work, and
one per C entry point that issues a memset, a copy or more than one launch, called through _lib.lib() with caller-owned buffers.

Every case draws its inputs twice from a seed (the real draw and the decoy), same shapes and ranges.  Shapes are the smallest
that still take the path the case is about.  Importing this module needs no GPU (tests/test_stream_table_host.py reads the
table); building a case does.

A float gradient that arrives through float atomics is compared with the bar its family's own GPU test holds two runs, or the
oracle, to (`bar_from` names it); everything else is compared bit for bit."""
from __future__ import annotations

import ctypes as C
import types

import torch

from tests.stream_harness import Case, Prepared, on

W, H, F = 96, 64, 80.0                  # at most 128 x 80
BG = (0.1, 0.2, 0.3)
BITS = "bits"
# tests/test_90_fullsize_properties_gpu.py::test_s1m_backward_linearity_and_repeatability: two runs agree to 1e-6 of the
# family's largest gradient (the fp64 record is rounded to fp32 once)
RASTER_GRAD = (0.0, 0.0, 1e-6)
RASTER_BAR = "tests/test_90_fullsize_properties_gpu.py::test_s1m_backward_linearity_and_repeatability"
# tests/test_35_mask_edges_gpu.py (near / grad_near): values rtol 2e-5 / atol 1e-6, gradients 1e-4 of the largest entry
MASK_VALUE = (2e-5, 1e-6, None)
MASK_GRAD = (0.0, 0.0, 1e-4)
MASK_BAR = "tests/test_35_mask_edges_gpu.py::test_pixel_counts"

ASYNC_TINY = "include/ogs_raster.h, ogs_raster_forward_tiny: 'Asynchronous, no read-back.'"
ASYNC_GEOM_NULL = "include/ogs_raster.h, ogs_raster_forward_geometry: 'num_rendered_host == NULL: no read-back, no synchronisation'"
ASYNC_DEFERRED = ("include/ogs_raster.h: 'Sync-free variant of the two calls above' (geometry with NULL, "
                  "ogs_raster_read_num_rendered_async, ogs_raster_forward_render_deferred)")
ASYNC_BACKWARD = "include/ogs_raster.h, ogs_raster_backward: 'Asynchronous on `stream`.'"
ASYNC_REBLEND = "include/ogs_raster.h, ogs_raster_forward_reblend: 'Asynchronous.'"
ASYNC_QUERY_WALK = "include/ogs_query.h, the four kept-pass walks: 'Forward only.  Asynchronous.'"
ASYNC_KNN = "include/ogs_knn.h: 'the entry point does no read-back' / 'No read-back, no float atomics'"
ASYNC_KNN_PY = "opengaussian_amd/knn.py docstrings: 'Nothing is read back from the device.' / 'nothing is read back'"
ASYNC_WIDE = "include/ogs_kmeans.h, wide k-means: 'Nothing is read back; everything runs on `stream`.'"
ASYNC_SEED = "include/ogs_kmeans.h, wide seeding: 'nothing is read back, so all k rounds are launched'"
ASYNC_ADAM = "include/ogs_optim.h, ogs_adam_step: 'Asynchronous on `stream`.'"
ASYNC_SELECT = "opengaussian_amd/query.py, select_leaves_by_text: 'No read-back'"
ASYNC_GROUP_STATS = "include/ogs_raster.h, ogs_raster_forward_group_stats: 'Asynchronous.'"
BLOCK_GEOMETRY = ("include/ogs_raster.h, ogs_raster_forward_geometry: 'writes num_rendered to *num_rendered_host (host memory) and "
                  "returns after the stream has finished it'")
BLOCK_DEFERRED_PY = ("opengaussian_amd/rasterizer.py, _streaming_render: 'the true count arrives through an async pinned copy and is "
                     "only WAITED for after everything is queued'")
BLOCK_EMITTED = "include/ogs_raster.h, ogs_raster_read_num_emitted: 'read back with a BLOCKING 4-byte copy into *host'"
BLOCK_TINY_BWD = "opengaussian_amd/rasterizer.py, tiny pass: 'backward() re-renders through the streaming path'"
BLOCK_GROUPED = "opengaussian_amd/rasterizer.py, rasterize_group_stats: 'Uses the blocking num_rendered read-back, as every grouped pass.'"
BLOCK_PLAN = "include/ogs_optim.h, ogs_densify_plan: 'Synchronises the stream (one 16-byte read-back'"
BLOCK_CODEBOOK = "opengaussian_amd/query.py, build_codebook: the k-means++ seeding's one read-back of the seeded count"
BLOCK_CONFUSION = "opengaussian_amd/query.py, confusion_table: 'one min / max read-back'"
BLOCK_SPLIT = "opengaussian_amd/query.py, multi_split: 'One read-back of the counts per split (the size of ``rows``).'"
BLOCK_REFINE = "opengaussian_amd/sam_refine.py, refine_sam_masks: 'stage 1 on the host: label classes, not pixels'"
BLOCK_RADIX = "include/ogs_raster.h, ogs_selftest_radix_sort: '*result_buffer (host) receives 0 or 1'"
ASYNC_SCAN = "include/ogs_raster.h, ogs_selftest_scan_u32: 'Asynchronous, no read-back.'"
BLOCK_KEPT_ADMIT = "opengaussian_amd/rasterizer.py, KeptPasses.admit: 'one 8-byte read-back per admitted view'"

# Launchers no case names.  Only profiling and debug hooks may stand here.
EXEMPT = {
    "ogs_selftest_wave_fold16": "test hook of one wave reduction: one launch, no memset, no state; tests/test_30_mask_gpu.py",
    "ogs_selftest_mfma_rank1": "test hook of one matrix instruction chain: one launch, not used by the kernels",
    "ogs_selftest_tile_order": "test hook of the workgroup order: one launch over a caller's ranges",
}


def _gen(seed, salt=0):
    return torch.Generator().manual_seed(seed * 1000 + salt)


def _camera():
    from opengaussian_amd.synthetic import make_camera
    return make_camera(W, H, F, F)


def _settings(dev, bg=BG, sh_degree=3, debug=False):
    from tests import helpers
    return helpers.settings_for(_camera(), bg, sh_degree, dev, debug)


SCENE_KEYS = ("means3D", "scales", "rotations", "opacities", "shs", "ins_feat")


def _scene(P, seed):
    from tests import helpers
    sc, _ = helpers.tiny_scene(P, W, H, F, seed=seed)
    return {k: getattr(sc, k).contiguous() for k in SCENE_KEYS}


def _leaves(b, keys):
    return {k: b[k].detach().clone().requires_grad_(True) for k in keys}


def _grads(leaves):
    return [v.grad for v in leaves.values()]


# ---- rasterizer ------------------------------------------------------------------------------------------------------------------
def _raster(P, kind="sh", backward=True, blocking=False, emitted=False):
    """GaussianRasterizer / rasterize_fused / rasterize_groups over a seeded scene, with the backward called from default-stream
    context on upstream gradients produced on the side stream"""
    def build(dev):
        from opengaussian_amd import rasterizer as R
        Cn = {"sh": 3, "fused": 9, "groups": 3}[kind]
        G = 3 if kind == "groups" else 1
        rs = _settings(dev)
        lead = (G,) if G > 1 else ()

        def inputs(seed):
            g = _gen(seed, 1)
            d = _scene(P, seed)
            d["g_color"] = torch.randn(*lead, Cn, H, W, generator=g)
            d["g_alpha"] = torch.randn(*lead, 1, H, W, generator=g)
            d["group"] = torch.randint(0, G + 1, (P,), generator=g).to(torch.int32)      # id G: in no group
            return d

        keys = ("means3D", "scales", "rotations", "opacities", "shs") + (("ins_feat",) if kind == "fused" else ())

        def run(b, s):
            if blocking:
                R._LAST_NUM_RENDERED.clear()
            saved = R._DEBUG_EMITTED
            R._DEBUG_EMITTED = [] if emitted else saved
            try:
                with on(s), torch.set_grad_enabled(backward):
                    lv = _leaves(b, keys) if backward else {k: b[k] for k in keys}
                    m2 = torch.zeros(P, 3, device=dev, requires_grad=backward)
                    geo = dict(scales=lv["scales"], rotations=lv["rotations"])
                    if kind == "sh":
                        out = R.GaussianRasterizer(rs)(means3D=lv["means3D"], means2D=m2, opacities=lv["opacities"],
                                                       shs=lv["shs"], **geo)
                    elif kind == "fused":
                        out = R.rasterize_fused(lv["means3D"], m2, lv["opacities"], lv["shs"], lv["ins_feat"], rs, **geo)
                    else:
                        out = R.rasterize_groups(lv["means3D"], m2, lv["opacities"], b["group"], G, rs, shs=lv["shs"], **geo)
                    color, radii, depth, alpha = out
                    gc, ga = b["g_color"] * 1.0, b["g_alpha"] * 1.0
            finally:
                R._DEBUG_EMITTED = saved
            outs = [color.detach(), radii, depth.detach(), alpha.detach()]
            if backward:
                torch.autograd.backward([color, alpha], [gc, ga])
                outs += _grads(lv) + [m2.grad]
            return outs
        return Prepared(inputs, run)
    return build


def _raster_compare(backward, n_leaves):
    return [BITS] * 4 + ([RASTER_GRAD] * (n_leaves + 1) if backward else [])


def _raster_model(P, backward):
    def build(dev):
        from opengaussian_amd import rasterizer as R
        rs = _settings(dev)
        keys = ("means3D", "features_dc", "features_rest", "opacity", "scaling", "rotation")

        def inputs(seed):
            g = _gen(seed, 2)
            sc = _scene(P, seed)
            op = sc["opacities"].clamp(1e-4, 1 - 1e-4)
            return {"means3D": sc["means3D"], "features_dc": 0.5 * torch.randn(P, 1, 3, generator=g),
                    "features_rest": 0.1 * torch.randn(P, 15, 3, generator=g), "opacity": torch.log(op / (1 - op)),
                    "scaling": torch.log(sc["scales"]), "rotation": sc["rotations"] * 1.5,
                    "g_color": torch.randn(3, H, W, generator=g)}

        def run(b, s):
            with on(s), torch.set_grad_enabled(backward):
                lv = _leaves(b, keys) if backward else {k: b[k] for k in keys}
                m2 = torch.zeros(P, 3, device=dev, requires_grad=backward)
                color, radii, depth, alpha = R.rasterize_model(lv["means3D"], m2, lv["features_dc"], lv["features_rest"],
                                                               lv["opacity"], lv["scaling"], lv["rotation"], rs)
                scales, rots, opac, shs = R.activate_model(b["features_dc"], b["features_rest"], b["opacity"], b["scaling"],
                                                           b["rotation"])
                gc = b["g_color"] * 1.0
            outs = [color.detach(), radii, depth.detach(), alpha.detach(), scales, rots, opac, shs]
            if backward:
                torch.autograd.backward([color], [gc])
                outs += _grads(lv)
            return outs
        return Prepared(inputs, run)
    return build


def _visible(dev):
    from opengaussian_amd import rasterizer as R
    P = 700
    rs = _settings(dev)

    def run(b, s):
        with on(s), torch.no_grad():
            radii = R.visible_radii(b["means3D"], b["opacities"], rs, b["ins_feat"][:, :3].contiguous(), b["scales"], b["rotations"])
            vis = R.GaussianRasterizer(rs).markVisible(b["means3D"])
        return [radii, vis]
    return Prepared(lambda seed: _scene(P, seed), run)


def _group_stats(dev):
    from opengaussian_amd import rasterizer as R
    P, G, L = 600, 3, 5
    rs = _settings(dev)

    def inputs(seed):
        g = _gen(seed, 3)
        d = _scene(P, seed)
        d["group"] = torch.randint(0, G + 1, (P,), generator=g).to(torch.int32)
        d["labels"] = torch.randint(-1, L, (H, W), generator=g).to(torch.int32)
        return d

    def run(b, s):
        with on(s), torch.no_grad():
            return list(R.rasterize_group_stats(b["means3D"], b["opacities"], b["group"], G, b["labels"], L, rs,
                                                b["ins_feat"][:, :3].contiguous(), b["scales"], b["rotations"]))
    return Prepared(inputs, run)


def _kept_state(dev, P=900, seed=77):
    """the state an ungrouped streaming 3-channel pass leaves behind, made once on the default stream (not part of a draw)"""
    from opengaussian_amd import rasterizer as R
    sc = {k: v.to(dev) for k, v in _scene(P, seed).items()}
    sink: list = []
    with torch.no_grad():
        R._RasterizeGaussians.apply(sc["means3D"], torch.zeros_like(sc["means3D"]), None, sc["means3D"], sc["opacities"],
                                    sc["scales"], sc["rotations"], None, _settings(dev, (0, 0, 0), 0), 0, None, None, 1, sink,
                                    True)
    torch.cuda.synchronize()
    assert sink, "the pass kept nothing"
    return sink[0]


def _kept_walks(dev):
    """label_map, label_votes, feature_votes and feature_map over one kept pass; the draws are the labels and features"""
    from opengaussian_amd import rasterizer as R
    P, L, D = 900, 7, 65
    kept = _kept_state(dev, P)

    def inputs(seed):
        g = _gen(seed, 4)
        return {"labels": torch.randint(-1, L, (P,), generator=g), "pixel_labels": torch.randint(-1, L, (H, W), generator=g),
                "rows": torch.randint(-1, 40, (P,), generator=g), "image": torch.randn(D, H, W, generator=g),
                "table": torch.randn(40, D, generator=g)}

    def run(b, s):
        with on(s), torch.no_grad():
            lm = R.label_map(kept, b["labels"], L)
            lv = R.label_votes(kept, b["pixel_labels"], L, rows=b["rows"], num_rows=40)
            fv = R.feature_votes(kept, b["image"], rows=b["rows"], num_rows=40)
            fm, alpha = R.feature_map(kept, b["table"], rows=b["rows"], with_alpha=True)
        return list(lm) + [lv, fv, fm, alpha]
    return Prepared(inputs, run)


def _tiny_model(dev, P=700, seed=9):
    from tests.golden import render_cases as rc
    g = _gen(seed, 5)
    sc = _scene(P, seed)
    op = sc["opacities"].clamp(1e-4, 1 - 1e-4)
    params = {"_xyz": sc["means3D"].clone(), "_features_dc": 0.5 * torch.randn(P, 1, 3, generator=g),
              "_features_rest": 0.1 * torch.randn(P, 15, 3, generator=g), "_scaling": torch.log(sc["scales"]),
              "_rotation": sc["rotations"].clone(), "_opacity": torch.log(op / (1 - op)), "_ins_feat": torch.randn(P, 6, generator=g)}
    return rc.TinyModel(params, dev, requires_grad=False)


PIPE = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


def _render(keep):
    """renderer.render over a frozen model whose instance features are the draw.  keep: the first call admits the pass to a
    kept-pass cache of the case's own, every later call is ONE re-blend launch of it; otherwise every call is a full pass."""
    def build(dev):
        from opengaussian_amd import rasterizer as R
        from opengaussian_amd.renderer import render
        P = 700
        model, cam = _tiny_model(dev, P), _camera().to(dev)
        bg = torch.tensor(BG, device=dev)
        cache = R.KeptPasses(budget_bytes=(1 << 30) if keep else 0)
        torch.cuda.synchronize()

        def inputs(seed):
            g = _gen(seed, 6)
            return {"ins_feat": torch.randn(P, 6, generator=g), "g_feat": torch.randn(6, H, W, generator=g)}

        def run(b, s):
            saved = R.KEPT_PASSES
            R.KEPT_PASSES = cache
            try:
                with on(s):
                    model._ins_feat = b["ins_feat"].detach().clone().requires_grad_(True)
                    out = render(cam, model, PIPE, bg, 0, rescale=False)
                    gf = b["g_feat"] * 1.0
            finally:
                R.KEPT_PASSES = saved
            torch.autograd.backward([out["ins_feat"]], [gf])
            return [out["render"].detach(), out["ins_feat"].detach(), out["alpha"].detach(), out["radii"], model._ins_feat.grad]
        return Prepared(inputs, run)
    return build


def _kept_admit(dev):
    """rasterize_fused with a frozen key over a cache of the call's own: a full pass that is admitted (ogs_raster_compact_kept,
    one read-back), then the same call again, which re-blends what the first one kept"""
    from opengaussian_amd import rasterizer as R
    P = 700
    rs = _settings(dev)

    def inputs(seed):
        g = _gen(seed, 34)
        d = _scene(P, seed)
        d["g_color"] = torch.randn(9, H, W, generator=g)
        return d

    def run(b, s):
        saved = R.KEPT_PASSES
        R.KEPT_PASSES = R.KeptPasses(budget_bytes=1 << 30)
        try:
            with on(s):
                feats = b["ins_feat"].detach().clone().requires_grad_(True)
                m2 = torch.zeros(P, 3, device=dev)
                call = lambda: R.rasterize_fused(b["means3D"], m2, b["opacities"], b["shs"], feats, rs, scales=b["scales"],
                                                 rotations=b["rotations"], frozen_key=("slot", "key", None))
                first = call()
                second = call()
                admitted, hits = R.KEPT_PASSES.stats["admitted"], R.KEPT_PASSES.stats["hits"]
                gc = b["g_color"] * 1.0
        finally:
            R.KEPT_PASSES = saved
        assert (admitted, hits) == (1, 1), (admitted, hits)
        torch.autograd.backward([second[0]], [gc])
        return [t.detach() for t in first] + [t.detach() for t in second] + [feats.grad]
    return Prepared(inputs, run)


def _feature_map_backward(dev):
    from opengaussian_amd import query, rasterizer as R
    P, Rn, D = 700, 30, 20
    model, cam = _tiny_model(dev, P), _camera().to(dev)
    bg = torch.zeros(3, device=dev)
    cache = R.KeptPasses(budget_bytes=0)
    torch.cuda.synchronize()

    def inputs(seed):
        g = _gen(seed, 7)
        return {"X": torch.randn(Rn, D, generator=g), "rows": torch.randint(-1, Rn, (P,), generator=g),
                "g_map": torch.randn(D, H, W, generator=g)}

    def run(b, s):
        saved = R.KEPT_PASSES
        R.KEPT_PASSES = cache
        try:
            with on(s):
                X = b["X"].detach().clone().requires_grad_(True)
                out = query.render_feature_map(cam, model, PIPE, bg, 0, X, rows=b["rows"])
                gm = b["g_map"] * 1.0
        finally:
            R.KEPT_PASSES = saved
        out.features.backward(gm)
        return [out.features.detach(), out.alpha.detach(), X.grad]
    return Prepared(inputs, run)


# ---- masks and losses ----------------------------------------------------------------------------------------------------------
def _masks(form):
    def build(dev):
        from opengaussian_amd import mask_ops as mk
        N, Cc, h, w = 11, 6, 40, 52

        def inputs(seed):
            g = _gen(seed, 8)
            return {"feat": torch.rand(Cc, h, w, generator=g), "labels": torch.randint(0, N + 1, (h, w), generator=g).to(torch.int32),
                    "sil": torch.rand(1, h, w, generator=g), "means": torch.rand(N, Cc, generator=g)}

        def run(b, s):
            with on(s):
                fm = b["feat"].detach().clone().requires_grad_(True)
                sw = b["sil"].detach().clone().requires_grad_(True)
                mu = b["means"].detach().clone().requires_grad_(True)
                masks = mk.LabelMasks(b["labels"], N)
                if form == "mask":
                    masks = masks.dense()
                mean = mk.mask_feature_mean(fm, masks, image_mask=sw)
                coh = mk.cohesion_loss(fm, masks, mean)
                # the separation loss ranks pairwise distances: it gets a table of the draw, not the atomically summed means
                sep = mk.separation_loss(mu, 40_000)
                with torch.no_grad():
                    _, var, cnt = mk.mask_feature_mean(b["feat"], masks, return_var=True)
                loss = mean.square().sum() + coh + sep
                up = torch.ones_like(loss)
            loss.backward(up)
            return [mean.detach(), coh.detach(), var, cnt, sep.detach(), mu.grad, fm.grad, sw.grad]
        return Prepared(inputs, run)
    return build


# variance: tests/test_35_mask_edges_gpu.py near(var, var_ref, rtol=2e-4, atol=1e-7); unweighted counts are integers; the separation
# loss is deterministic (tests/test_34_separation_edges_gpu.py holds two runs to the same bits)
MASK_COMPARE = [MASK_VALUE, MASK_VALUE, (2e-4, 1e-7, None), BITS, BITS, BITS, MASK_GRAD, MASK_GRAD]


def _losses(dev):
    from opengaussian_amd import losses

    def inputs(seed):
        g = _gen(seed, 9)
        return {"img": torch.rand(3, 50, 70, generator=g), "gt": torch.rand(3, 50, 70, generator=g),
                "x6": torch.rand(6, 50, 70, generator=g), "t6": torch.rand(6, 50, 70, generator=g),
                "mask": (torch.rand(50, 70, generator=g) < 0.6), "weight": torch.rand(50, 70, generator=g)}

    def run(b, s):
        with on(s):
            img = b["img"].detach().clone().requires_grad_(True)
            x6 = b["x6"].detach().clone().requires_grad_(True)
            loss, l1 = losses.photometric_loss(img, b["gt"], 0.2)
            m1 = losses.l1_loss(x6, b["t6"], b["mask"], b["weight"])
            m2 = losses.l2_loss(x6, b["t6"], b["mask"], b["weight"])
            total = loss + 2.0 * m1 + 3.0 * m2
            up = torch.ones_like(total)
        total.backward(up)
        return [loss.detach(), l1.detach(), m1.detach(), m2.detach(), img.grad, x6.grad]
    return Prepared(inputs, run)


# ---- optimiser and densification ------------------------------------------------------------------------------------------------
GROUPS = (("xyz", (3,), 1.6e-4), ("f_dc", (1, 3), 2.5e-3), ("f_rest", (15, 3), 1.25e-4), ("opacity", (1,), 0.05),
          ("scaling", (3,), 5e-3), ("rotation", (4,), 1e-3), ("ins_feat", (6,), 1e-3))


def _model_inputs(P, seed):
    g = _gen(seed, 10)
    d = {}
    for n, shape, _ in GROUPS:
        d[n] = torch.randn(P, *shape, generator=g) * 0.3
        d["grad_" + n] = torch.randn(P, *shape, generator=g)
        d["m_" + n] = torch.randn(P, *shape, generator=g) * 0.01
        d["v_" + n] = torch.rand(P, *shape, generator=g) * 0.01
    d["scaling"] = d["scaling"] - 3.0
    d["accum"] = torch.rand(P, 1, generator=g) * 4e-4
    d["denom"] = torch.randint(0, 3, (P, 1), generator=g).to(torch.float32)
    d["radii2D"] = torch.rand(P, generator=g) * 30
    d["vs_grad"] = torch.randn(P, 3, generator=g) * 1e-3
    d["radii"] = torch.randint(0, 40, (P,), generator=g).to(torch.int32)
    d["prune"] = torch.rand(P, generator=g) < 0.3
    return d


def _optimizer(b, dev):
    from opengaussian_amd.optim import FusedAdam
    p = {n: torch.nn.Parameter(b[n].detach().clone()) for n, _, _ in GROUPS}
    opt = FusedAdam([{"params": [p[n]], "lr": lr, "name": n} for n, _, lr in GROUPS], lr=0.0, eps=1e-15)
    for n, _, _ in GROUPS:
        opt.state[p[n]] = {"step": torch.tensor(3.0), "exp_avg": b["m_" + n].clone(), "exp_avg_sq": b["v_" + n].clone()}
    return opt, p


def _opt_outputs(opt):
    outs = []
    for group in opt.param_groups:
        p = group["params"][0]
        outs += [p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]]
    return outs


def _adam(dev):
    P = 1200

    def run(b, s):
        with on(s):
            opt, p = _optimizer(b, dev)
            for n, _, _ in GROUPS:
                p[n].grad = b["grad_" + n].clone()
            opt.step()
        return _opt_outputs(opt)
    return Prepared(lambda seed: _model_inputs(P, seed), run)


def _densify(what):
    def build(dev):
        from opengaussian_amd import densify as dn
        P = 1200

        def run(b, s):
            with on(s):
                opt, _ = _optimizer(b, dev)
                state = dn.DensifyState(opt, b["accum"].clone(), b["denom"].clone(), b["radii2D"].clone(), 0.01)
                if what == "stats":
                    dn.add_densification_stats(state, b["vs_grad"], radii=b["radii"])
                    return [state.xyz_gradient_accum, state.denom, state.max_radii2D]
                if what == "prune":
                    dn.prune_points(state, b["prune"])
                    return _opt_outputs(opt) + [state.xyz_gradient_accum, state.denom, state.max_radii2D]
                torch.cuda.manual_seed(7)                               # the split children's draw
                dn.densify_and_prune(state, 2e-4, 0.005, 4.0, 20)
                return _opt_outputs(opt) + [state.last_plan["src_row"], state.last_plan["kind"]]
        return Prepared(lambda seed: _model_inputs(P, seed), run)
    return build


# ---- k-means ---------------------------------------------------------------------------------------------------------------------
def _quantize(dev):
    from opengaussian_amd import kmeans
    N = 3000

    def inputs(seed):
        g = _gen(seed, 11)
        return {"xyz": torch.rand(N, 3, generator=g), "ins_feat": torch.rand(N, 6, generator=g)}

    def run(b, s):
        with on(s):
            qk = kmeans.Quantize_kMeans(num_clusters=64, num_leaf_clusters=4, num_iters=3)
            feat = torch.cat((b["ins_feat"], b["xyz"]), dim=1)
            qk.centers = feat[:64].clone()
            gaussian = types.SimpleNamespace(_xyz=b["xyz"], _ins_feat=b["ins_feat"].detach().clone().requires_grad_(True))
            qk.forward(gaussian, 0, assign=True, mode="root")
            out = gaussian._ins_feat_q
            cent = qk.centers.clone()
            sharded = cent.clone()
            ids2 = kmeans.lloyd_sharded(feat, sharded, 2, 1)
        return [out.detach(), qk.nn_index, cent, sharded, ids2]
    return Prepared(inputs, run)


def _wide(dev):
    from opengaussian_amd import kmeans
    N, D, k = 2500, 65, 24

    def inputs(seed):
        g = _gen(seed, 12)
        X = torch.randn(N, D, generator=g)
        return {"X": X, "w": torch.rand(N, generator=g) + 0.1, "C": X[torch.randperm(N, generator=g)[:k]].clone()}

    def run(b, s):
        with on(s):
            ids, dist = kmeans.wide_assign(b["X"], b["C"])
            cu = b["C"].clone()
            counts = kmeans.wide_update(b["X"], ids, cu, weights=b["w"])
            cl = b["C"].clone()
            lloyd = kmeans.wide_lloyd(b["X"], cl, 3, weights=b["w"])
            seeded = kmeans.wide_seed(b["X"], k, "l2", b["w"], 3)
        return [ids, dist, cu, counts, cl] + list(lloyd) + list(seeded)
    return Prepared(inputs, run)


def _codebook(dev):
    from opengaussian_amd import query
    N, D, k = 1500, 32, 8

    def inputs(seed):
        return {"X": torch.randn(N, D, generator=_gen(seed, 13))}

    def run(b, s):
        with on(s):
            book = query.build_codebook(b["X"], k, iters=2, init="k-means++", seed=5)
        return [book.leaf_ind]
    return Prepared(inputs, run)


# ---- kNN -------------------------------------------------------------------------------------------------------------------------
def _points(n, seed, salt):
    g = _gen(seed, salt)
    centres = torch.rand(6, 3, generator=g)
    return (centres[torch.randint(0, 6, (n,), generator=g)] + 0.08 * torch.randn(n, 3, generator=g)).contiguous()


def _knn_lists(dev):
    """neighbors, Index build / query / radius_count, the one-shot forms, dbscan, components, reverse_edges"""
    from opengaussian_amd import knn
    n, m, K = 3000, 700, 8

    def inputs(seed):
        g = _gen(seed, 14)
        return {"pts": _points(n, seed, 15), "q": _points(m, seed, 16) * 1.3 - 0.1,
                "labels": torch.randint(-1, 3, (n,), generator=g).to(torch.int32)}

    def run(b, s):
        with on(s):
            idx, d2 = knn.neighbors(b["pts"], K)
            index = knn.Index(b["pts"])
            qi, qd = index.query(b["q"], K)
            rc = index.radius_count(b["q"], 0.07)
            rc2 = knn.radius_count(b["pts"], 0.05, labels=b["labels"])
            q2 = knn.query(b["pts"], b["q"], 3)
            db = knn.dbscan(b["pts"], 0.03, 5, labels=b["labels"])
            comp = knn.components(idx, d2, 0.03 * 0.03, labels=b["labels"])
            begin, slots = knn.reverse_edges(idx)
            live = torch.arange(slots.numel(), device=dev) < begin[-1]
            slots = torch.where(live, slots, torch.full_like(slots, -1))             # past begin[-1]: unspecified
        return [idx, d2, qi, qd, rc, rc2, *q2, *db, *comp, begin, slots]
    return Prepared(inputs, run)


def _knn_filters(dev):
    """outlier_mask (grouped), distCUDA2 on both routes: ogs_knn_group_ksum and the box search"""
    from opengaussian_amd import knn
    n = 2500

    def inputs(seed):
        g = _gen(seed, 17)
        return {"pts": _points(n, seed, 18), "group": torch.randint(-1, 4, (n,), generator=g)}

    def run(b, s):
        with on(s):
            keep = knn.outlier_mask(b["pts"], b["group"], 4)
            one = knn.outlier_mask(b["pts"])
            brute = knn.distCUDA2(b["pts"], route="brute")
            boxes = knn.distCUDA2(b["pts"], route="boxes")
        return [keep, one, brute, boxes]
    return Prepared(inputs, run)


# the group totals of the outlier filter are fp64 atomic adds "whose order moves the last bits only" (knn.outlier_mask): the
# keep masks are decisions on them, compared as bits like every other run-to-run check of the family
# (tests/test_37_knn_gpu.py::test_many_groups_through_knn_py_in_callers_order_and_deterministic)


def _knn_graph(dev):
    """aggregate, gather_sum with backward (both gradients), smoothness_energy, query.neighbor_smoothness with backward"""
    from opengaussian_amd import knn, query
    n, K, D = 2000, 8, 65
    pts = _points(n, 3, 19).to(dev)
    idx, d2 = knn.neighbors(pts, K)
    rev = knn.reverse_edges(idx)
    torch.cuda.synchronize()

    def inputs(seed):
        g = _gen(seed, 20)
        return {"X": torch.randn(n, D, generator=g), "w": torch.rand(n, K, generator=g), "G": torch.randn(n, D, generator=g)}

    def run(b, s):
        with on(s):
            agg = knn.aggregate(b["X"], idx, b["w"])
            X = b["X"].detach().clone().requires_grad_(True)
            w = b["w"].detach().clone().requires_grad_(True)
            out = knn.gather_sum(X, idx, w)                              # the reverse lists are built in the backward
            energy, total = knn.smoothness_energy(b["X"], idx, b["w"])
            X2 = b["X"].detach().clone().requires_grad_(True)
            w2 = b["w"].detach().clone().requires_grad_(True)
            loss = query.neighbor_smoothness(X2, idx, w2, rev, reduction="sum")
            G = b["G"] * 1.0
            up = torch.ones_like(loss)
        out.backward(G)
        loss.backward(up)
        return [agg, out.detach(), energy, total, loss.detach(), X.grad, w.grad, X2.grad, w2.grad]
    return Prepared(inputs, run)


# ---- query -----------------------------------------------------------------------------------------------------------------------
def _query_text(dev):
    from opengaussian_amd import query
    Q, K, D, N = 5, 300, 64, 4000

    def inputs(seed):
        g = _gen(seed, 21)
        return {"text": torch.randn(Q, D, generator=g), "leaf": torch.randn(K, D, generator=g),
                "occu": torch.randint(0, 12, (K,), generator=g), "centers": torch.rand(K + 1, 6, generator=g),
                "leaf_ind": torch.randint(0, K, (N,), generator=g)}

    def run(b, s):
        with on(s):
            sim, sel, cnt = query.select_leaves_by_text(b["text"], b["leaf"], b["occu"], b["centers"], 10.0)
            live = torch.arange(sel.shape[1], device=dev)[None, :] < cnt[:, None]
            pred = query.classify_points(b["text"], b["leaf"], b["occu"], b["leaf_ind"])
            listed = torch.where(live, sel, torch.full_like(sel, -1))
        return [sim, listed, cnt, pred]
    return Prepared(inputs, run)


def _query_tables(dev):
    from opengaussian_amd import query
    N, Cc, K, Q = 4000, 9, 37, 70

    def inputs(seed):
        g = _gen(seed, 22)
        return {"gt": torch.randint(0, Cc, (N,), generator=g), "pred": torch.randint(0, Cc, (N,), generator=g),
                "ignore": torch.rand(N, generator=g) < 0.1, "leaf_ind": torch.randint(-1, K + 1, (N,), generator=g),
                "words": torch.randint(-2 ** 62, 2 ** 62, (K, 2), generator=g), "row_ok": torch.rand(N, generator=g) < 0.8,
                "keep": torch.rand(Q, generator=g) < 0.7}

    def run(b, s):
        with on(s):
            conf = query.confusion_table(b["gt"], b["pred"], Cc, b["ignore"])
            begin, rows, counts = query.multi_split(b["leaf_ind"], b["words"], Q, b["row_ok"], b["keep"])
        return [conf, begin, rows, counts]
    return Prepared(inputs, run)


# ---- other -----------------------------------------------------------------------------------------------------------------------
def _refine(dev):
    from opengaussian_amd.sam_refine import MultiViewSAMMaskRefiner
    from tests.golden import sam_refine_cases as sc
    # 96 x 64: the whole-image footprint of the model's first Gaussian (6144 pixels) is more than one wave walks, so its label
    # sums take the workgroup kernel (ogs_refine_footprint_labels_block)
    n, width, height = 300, 96, 64
    cams = [c.to(dev) for c in sc.cameras(width, height, sc.FOCAL * width / sc.W, full=False)]
    names = ("xyz", "opacity", "scaling", "rotation", "features")

    def inputs(seed):
        m = sc.model(n, seed)
        d = dict(zip(names, (m.get_xyz, m.get_opacity, m.get_scaling, m.get_rotation, m.get_features)))
        for c, t in enumerate(sc.masks(width, height, seed=seed, block=(16, 24), void=(2, 2))):
            d[f"mask{c}"] = t.to(torch.int32)
        return d

    def run(b, s):
        with on(s):
            model = sc.Model(*(b[k] for k in names))
            refiner = MultiViewSAMMaskRefiner()
            out = refiner.refine_sam_masks(cams, [b[f"mask{c}"] for c in range(3)], model, sam_level=sc.SAM_LEVEL, stage1_stride=7)
        return [t for t in out if torch.is_tensor(t)]
    return Prepared(inputs, run)


def _sh_exchange(dev):
    from opengaussian_amd import dp
    P, M = 900, 16
    ex = dp.ShGradExchange(P, M, dev)
    campos = torch.tensor([[0.3, -0.2, -4.0]], device=dev)
    torch.cuda.synchronize()

    def inputs(seed):
        g = _gen(seed, 23)
        return {"means3D": torch.randn(P, 3, generator=g), "rgb": torch.randn(P, 3, generator=g)}

    def run(b, s):
        with on(s):
            ex.gather_async(b["rgb"])
            return [ex.rebuild(b["means3D"], campos, 3)]
    return Prepared(inputs, run)


# ---- the C ABI with caller-owned buffers ------------------------------------------------------------------------------------------
def _u8(n, dev):
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device=dev)


def _st(s):
    return torch.cuda.current_stream().cuda_stream if s is None else s.cuda_stream


def _call(name, *args):
    from opengaussian_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args), name)


def _p(t):
    return None if t is None else t.data_ptr()


def _c_knn_radius(dev):
    """ogs_knn_index_build, ogs_knn_radius_count (memsets its counts), ogs_knn_dbscan (memsets its cluster count)"""
    from opengaussian_amd import _lib
    L = _lib.lib()
    n, m = 3000, 700
    e = lambda *sh, dt=torch.int32: torch.empty(*sh, dtype=dt, device=dev)
    index_bytes = int(L.ogs_knn_index_bytes(n))
    index, build_tmp = _u8(index_bytes, dev), _u8(L.ogs_knn_index_build_tmp_bytes(n), dev)
    count, rc_tmp = e(m), _u8(L.ogs_knn_radius_count_tmp_bytes(n, m), dev)
    cluster, core, degree, sizes, first, ncl = e(n), e(n, dt=torch.uint8), e(n), e(n), e(n), e(1)
    db_tmp = _u8(L.ogs_knn_dbscan_tmp_bytes(n), dev)
    K = 8
    nidx, nd2, nb_tmp = e(n, K), e(n, K, dt=torch.float32), _u8(L.ogs_knn_neighbors_tmp_bytes(n), dev)
    qidx, qd2, q_tmp = e(m, K), e(m, K, dt=torch.float32), _u8(L.ogs_knn_query_tmp_bytes(n, m), dev)

    def inputs(seed):
        g = _gen(seed, 24)
        return {"pts": _points(n, seed, 25), "q": _points(m, seed, 26), "labels": torch.randint(-1, 3, (n,), generator=g).to(torch.int32),
                "qlabels": torch.randint(-1, 3, (m,), generator=g).to(torch.int32), "r2": torch.rand(1, generator=g) * 0.004 + 0.002}

    def run(b, s):
        st = _st(s)
        _call("ogs_knn_index_build", n, _p(b["pts"]), _p(index), index_bytes, _p(build_tmp), build_tmp.numel(), st)
        _call("ogs_knn_radius_count", n, _p(index), m, _p(b["q"]), _p(b["r2"]), _p(b["labels"]), _p(b["qlabels"]), _p(count),
              _p(rc_tmp), rc_tmp.numel(), st)
        _call("ogs_knn_dbscan", n, _p(b["pts"]), _p(b["r2"]), 5, _p(b["labels"]), _p(cluster), _p(core), _p(degree), _p(sizes),
              _p(first), _p(ncl), _p(db_tmp), db_tmp.numel(), st)
        _call("ogs_knn_neighbors", n, _p(b["pts"]), K, 1, _p(nidx), _p(nd2), _p(nb_tmp), nb_tmp.numel(), st)
        _call("ogs_knn_query", n, _p(index), m, _p(b["q"]), K, _p(qidx), _p(qd2), _p(q_tmp), q_tmp.numel(), st)
        return [count, cluster, core, degree, sizes, first, ncl, nidx, nd2, qidx, qd2]
    return Prepared(inputs, run, out=[index, count, cluster, core, degree, sizes, first, ncl, nidx, nd2, qidx, qd2],
                    tmp=[build_tmp, rc_tmp, db_tmp, nb_tmp, q_tmp])


def _c_knn_graph(dev):
    """ogs_knn_transpose (memsets begin), ogs_knn_smoothness_fwd (memsets total) and _bwd, ogs_knn_components (memsets count),
    ogs_knn_aggregate_t"""
    from opengaussian_amd import _lib
    L = _lib.lib()
    n, K, D = 2000, 8, 20
    e = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device=dev)
    i32 = torch.int32
    begin, slots = e(n + 1, dt=i32), e(n * K, dt=i32)
    tr_tmp = _u8(L.ogs_knn_transpose_tmp_bytes(n, K, n), dev)
    energy, total = e(n), e(2, dt=torch.float64)
    sf_tmp = _u8(L.ogs_knn_smoothness_fwd_tmp_bytes(n), dev)
    gF, gw = e(n, D), e(n, K)
    sb_tmp = _u8(L.ogs_knn_smoothness_bwd_tmp_bytes(n, K, D), dev)
    comp, sizes, first, count = e(n, dt=i32), e(n, dt=i32), e(n, dt=i32), e(1, dt=i32)
    cc_tmp = _u8(L.ogs_knn_components_tmp_bytes(n), dev)
    gX = e(n, D)
    at_tmp = _u8(L.ogs_knn_aggregate_t_tmp_bytes(n, K, n, D), dev)

    def inputs(seed):
        g = _gen(seed, 27)
        idx = torch.randint(0, n, (n, K), generator=g).to(i32)
        idx[torch.rand(n, K, generator=g) < 0.1] = -1
        return {"idx": idx, "w": torch.rand(n, K, generator=g), "F": torch.randn(n, D, generator=g),
                "d2": torch.rand(n, K, generator=g), "max_d2": torch.rand(1, generator=g) * 0.2 + 0.1,
                "scale": torch.rand(1, generator=g) + 0.5, "labels": torch.randint(-1, 3, (n,), generator=g).to(i32)}

    def run(b, s):
        st = _st(s)
        _call("ogs_knn_transpose", n, K, n, _p(b["idx"]), _p(begin), _p(slots), _p(tr_tmp), tr_tmp.numel(), st)
        _call("ogs_knn_smoothness_fwd", n, K, D, _p(b["idx"]), _p(b["w"]), _p(b["F"]), _p(energy), _p(total), _p(sf_tmp),
              sf_tmp.numel(), st)
        _call("ogs_knn_smoothness_bwd", n, K, D, _p(b["idx"]), _p(b["w"]), _p(b["F"]), _p(begin), _p(slots), _p(b["scale"]), _p(gF),
              _p(gw), _p(sb_tmp), sb_tmp.numel(), st)
        _call("ogs_knn_components", n, K, _p(b["idx"]), _p(b["d2"]), _p(b["max_d2"]), _p(b["labels"]), _p(comp), _p(sizes),
              _p(first), _p(count), _p(cc_tmp), cc_tmp.numel(), st)
        _call("ogs_knn_aggregate_t", n, K, n, D, _p(begin), _p(slots), _p(b["w"]), _p(b["F"]), _p(gX), _p(at_tmp), at_tmp.numel(), st)
        with on(s):
            live = torch.arange(n * K, device=dev) < begin[-1]
            listed = torch.where(live, slots, torch.full_like(slots, -1))
        return [begin, listed, energy, total, gF, gw, comp, sizes, first, count, gX]
    return Prepared(inputs, run, out=[begin, slots, energy, total, gF, gw, comp, sizes, first, count, gX],
                    tmp=[tr_tmp, sf_tmp, sb_tmp, cc_tmp, at_tmp])


def _c_wide(dev):
    """ogs_kmeans_wide_assign / _update (memsets counts) / _inertia / _lloyd / _seed (memsets the head of its scratch)"""
    from opengaussian_amd import _lib
    L = _lib.lib()
    N, D, k, iters = 2500, 65, 24, 3
    e = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device=dev)
    nbytes = int(L.ogs_kmeans_wide_tmp_bytes(N, D, k))
    tmp = _u8(nbytes, dev)
    ids, dist, counts, total = e(N, dt=torch.int32), e(N), e(k), e(1, dt=torch.float64)
    ids_l, dist_l, counts_l, inertia = e(N, dt=torch.int32), e(N), e(k), e(iters + 1, dt=torch.float64)
    cu, cl = e(k, D), e(k, D)
    seed_bytes = int(L.ogs_kmeans_wide_seed_tmp_bytes(N, D, k))
    seed_tmp = _u8(seed_bytes, dev)
    centers, rows, ids_s, d2, stats = e(k, D), e(k, dt=torch.int32), e(N, dt=torch.int32), e(N), e(4, dt=torch.int64)

    def inputs(seed):
        g = _gen(seed, 28)
        X = torch.randn(N, D, generator=g)
        return {"X": X, "w": torch.rand(N, generator=g) + 0.1, "C": X[torch.randperm(N, generator=g)[:k]].clone()}

    def run(b, s):
        st = _st(s)
        with on(s):
            cu.copy_(b["C"])
            cl.copy_(b["C"])
        _call("ogs_kmeans_wide_assign", _p(b["X"]), N, D, _p(b["C"]), k, 0, _p(ids), _p(dist), _p(tmp), nbytes, st)
        _call("ogs_kmeans_wide_update", _p(b["X"]), _p(b["w"]), N, D, _p(ids), k, 0, _p(cu), _p(counts), _p(tmp), nbytes, st)
        _call("ogs_kmeans_wide_inertia", _p(dist), _p(b["w"]), N, _p(total), _p(tmp), nbytes, st)
        _call("ogs_kmeans_wide_lloyd", _p(b["X"]), _p(b["w"]), N, D, _p(cl), k, 0, iters, _p(ids_l), _p(dist_l), _p(counts_l),
              _p(inertia), _p(tmp), nbytes, st)
        _call("ogs_kmeans_wide_seed", _p(b["X"]), _p(b["w"]), None, N, D, k, 3, 1, _p(centers), _p(rows), _p(ids_s), _p(d2),
              _p(stats), _p(seed_tmp), seed_bytes, st)
        return [ids, dist, cu, counts, total, cl, ids_l, dist_l, counts_l, inertia, centers, rows, ids_s, d2, stats[:1]]
    # what the Python wrapper hands over zeroed or preset (kmeans.wide_lloyd, kmeans.wide_seed) is cleared the same way here
    return Prepared(inputs, run, out=[ids, dist, counts, total, ids_l, dist_l, inertia], tmp=[tmp, seed_tmp],
                    clear=[counts_l, centers, ids_s, d2, stats, rows])


def _c_query(dev):
    """ogs_query_confusion (memsets conf) and the split trio count / scan (memsets begin and counts) / scatter"""
    from opengaussian_amd import _lib
    L = _lib.lib()
    N, Cc, K, Q = 4000, 9, 37, 40
    i64 = torch.int64
    conf = torch.empty(Cc, Cc, dtype=i64, device=dev)
    tmp = _u8(L.ogs_query_split_tmp_bytes(N, Q), dev)
    begin = torch.empty(Q + 1, dtype=torch.int32, device=dev)
    counts = torch.empty(Q, dtype=torch.int32, device=dev)
    rows = torch.empty(N * Q, dtype=i64, device=dev)

    def inputs(seed):
        g = _gen(seed, 29)
        return {"gt": torch.randint(0, Cc, (N,), generator=g), "pred": torch.randint(0, Cc, (N,), generator=g),
                "ignore": (torch.rand(N, generator=g) < 0.1).to(torch.uint8), "leaf_ind": torch.randint(-1, K + 1, (N,), generator=g),
                "words": torch.randint(-2 ** 62, 2 ** 62, (K,), generator=g), "row_ok": (torch.rand(N, generator=g) < 0.8).to(torch.uint8)}

    def run(b, s):
        st = _st(s)
        _call("ogs_query_confusion", N, _p(b["gt"]), _p(b["pred"]), _p(b["ignore"]), Cc, _p(conf), st)
        _call("ogs_query_split_count", N, _p(b["leaf_ind"]), K, _p(b["words"]), _p(b["row_ok"]), Q, _p(tmp), st)
        _call("ogs_query_split_scan", N, Q, None, _p(tmp), _p(begin), _p(counts), st)
        # capacity N * Q instead of the read-back total: "the scatter writes nothing at or past it"
        _call("ogs_query_split_scatter", N, _p(b["leaf_ind"]), K, _p(b["words"]), _p(b["row_ok"]), Q, None, _p(tmp), _p(rows),
              N * Q, st)
        with on(s):
            live = torch.arange(N * Q, device=dev) < begin[-1]
            listed = torch.where(live, rows, torch.full_like(rows, -1))
        return [conf, begin, counts, listed]
    return Prepared(inputs, run, out=[conf, begin, counts, rows], tmp=[tmp])


def _c_masks(form):
    def build(dev):
        """ogs_{mask,label}_feature_sums (memsets the table), _sums_backward (memsets dfeat and dweight), _cohesion and
        _cohesion_backward (memset their tables)"""
        N, Cc, h, w = 11, 6, 40, 52
        HW = h * w
        e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
        table, coh, dfeat, dweight, dfeat2, dmean = e(N, 16), e(N, 16), e(Cc, HW), e(HW), e(Cc, HW), e(N, 16)
        sq = e(N, 16)

        def inputs(seed):
            g = _gen(seed, 30)
            return {"feat": torch.rand(Cc, HW, generator=g), "labels": torch.randint(0, N + 1, (HW,), generator=g).to(torch.int32),
                    "weight": torch.rand(HW, generator=g), "coef": torch.randn(N, Cc, generator=g), "coef_cnt": torch.randn(N, generator=g),
                    "mean": torch.rand(N, Cc, generator=g), "gl": torch.rand(N, generator=g)}

        def run(b, s):
            st = _st(s)
            with on(s):
                member = b["labels"]
                if form == "mask":
                    member = (b["labels"][None] == torch.arange(1, N + 1, dtype=torch.int32, device=dev)[:, None]).to(torch.uint8)
                    member = member.contiguous()
            _call(f"ogs_{form}_feature_sums", _p(b["feat"]), _p(member), _p(b["weight"]), Cc, N, HW, 0, _p(table), st)
            _call(f"ogs_{form}_feature_sums_backward", _p(member), _p(b["weight"]), _p(b["coef"]), _p(b["feat"]), _p(b["coef_cnt"]),
                  Cc, N, HW, _p(dfeat), _p(dweight), st)
            _call(f"ogs_{form}_cohesion", _p(b["feat"]), _p(member), _p(b["mean"]), Cc, N, HW, _p(coh), st)
            _call(f"ogs_{form}_cohesion_backward", _p(b["feat"]), _p(member), _p(b["mean"]), _p(b["gl"]), Cc, N, HW, _p(dfeat2),
                  _p(dmean), st)
            _call(f"ogs_{form}_feature_sqdev", _p(b["feat"]), _p(member), _p(b["weight"]), _p(b["mean"]), Cc, N, HW, _p(sq), st)
            return [table[:, :Cc + 1], dfeat, dweight, coh[:, :2], dfeat2, dmean[:, :Cc], sq[:, :Cc]]
        return Prepared(inputs, run, out=[table, coh, dfeat, dweight, dfeat2, dmean, sq])
    return build


C_MASK_COMPARE = [MASK_VALUE, MASK_GRAD, MASK_GRAD, MASK_VALUE, MASK_GRAD, MASK_GRAD, (2e-4, 1e-7, None)]


def _c_losses(dev):
    """the image losses (a partial-sum launch and a one-workgroup reduction each, no atomics) and the separation loss (two
    launches), every scratch dirtied"""
    from opengaussian_amd import _lib
    L = _lib.lib()
    Cc, h, w, N = 3, 50, 70, 40
    e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
    out5, dimg, out3, dx = e(5), e(Cc, h, w), e(3), e(6, h * w)
    ph_tmp, mk_tmp = _u8(L.ogs_loss_photometric_tmp_bytes(Cc, h, w), dev), _u8(L.ogs_loss_masked_tmp_bytes(), dev)
    loss, grad, sep_tmp = e(1), e(N, 6), e(N * N + N)

    def inputs(seed):
        g = _gen(seed, 35)
        return {"img": torch.rand(Cc, h, w, generator=g), "gt": torch.rand(Cc, h, w, generator=g), "g": torch.rand(3, generator=g) + 0.5,
                "x6": torch.rand(6, h * w, generator=g), "t6": torch.rand(6, h * w, generator=g),
                "mask": (torch.rand(h * w, generator=g) < 0.6).to(torch.uint8), "weight": torch.rand(h * w, generator=g),
                "means": torch.rand(N, 6, generator=g)}

    def run(b, s):
        st = _st(s)
        g = b["g"]
        _call("ogs_loss_photometric_forward", _p(b["img"]), _p(b["gt"]), Cc, h, w, 0.2, _p(out5), _p(ph_tmp), st)
        _call("ogs_loss_photometric_backward", _p(b["img"]), _p(b["gt"]), g[0:1].data_ptr(), g[1:2].data_ptr(), g[2:3].data_ptr(),
              0.2, Cc, h, w, _p(dimg), st)
        _call("ogs_loss_masked_forward", _p(b["x6"]), _p(b["t6"]), _p(b["mask"]), _p(b["weight"]), 1, 2, 6, h * w, _p(out3),
              _p(mk_tmp), st)
        _call("ogs_loss_masked_backward", _p(b["x6"]), _p(b["t6"]), _p(b["mask"]), _p(b["weight"]), 1, 2, 6, h * w, _p(out3),
              g[0:1].data_ptr(), _p(dx), st)
        _call("ogs_separation_loss", _p(b["means"]), N, 6, 1, _p(loss), _p(grad), _p(sep_tmp), st)
        return [out5, dimg, out3, dx, loss, grad]
    return Prepared(inputs, run, out=[out5, dimg, out3, dx, loss, grad], tmp=[ph_tmp, mk_tmp, sep_tmp])


def _c_raster(deferred):
    """The forward through the C ABI on caller-owned buffers, every scratch and output dirtied on the stream first, then the
    backward with a dirty gradient record (bwd_tmp_is_clear = 0: it clears the record itself).
    deferred: geometry without a read-back, the async count copy, the deferred render phase with a capacity of twice what either
    draw renders -- no call of the sequence waits for the stream.  Otherwise the blocking geometry phase and the exact render
    phase, then the backward."""
    def build(dev):
        from opengaussian_amd import _lib
        from opengaussian_amd import rasterizer as R
        L = _lib.lib()
        P, Cn = 800, 3
        rs = _settings(dev)
        # no pair list is longer than every Gaussian on every tile
        cap = P * ((W + 15) // 16) * ((H + 15) // 16)
        gb, gtb, ib = R._geom_sizes(P, W, H, Cn, 1)
        btb, srb, qlb = R._render_sizes(cap, W, H, Cn)
        e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
        color, depth, alpha, radii = e(Cn, H, W), e(1, H, W), e(1, H, W), torch.empty(P, dtype=torch.int32, device=dev)
        geom, geom_tmp, image = _u8(gb, dev), _u8(gtb, dev), _u8(ib, dev)
        point_list = torch.empty(cap, dtype=torch.int32, device=dev)
        bin_tmp, sorted_rec, quad_list = _u8(btb, dev), _u8(srb, dev), _u8(qlb, dev)
        bwd_tmp = _u8(L.ogs_raster_backward_tmp_bytes(P), dev)
        g_m3, g_m2, g_op, g_scl, g_rot, g_sh = e(P, 3), e(P, 3), e(P, 1), e(P, 3), e(P, 4), e(P, 16, 3)
        pinned = torch.zeros(1, dtype=torch.int32).pin_memory()
        bg = torch.tensor(BG, device=dev)
        view, proj, campos = (t.to(dev).contiguous() for t in (rs.viewmatrix, rs.projmatrix, rs.campos))
        torch.cuda.synchronize()

        def inputs(seed):
            d = _scene(P, seed)
            d.pop("ins_feat")
            g = _gen(seed, 31)
            d["g_color"], d["g_alpha"] = torch.randn(Cn, H, W, generator=g), torch.randn(1, H, W, generator=g)
            return d

        def run(b, s):
            st = _st(s)
            a = R._fwd_args(rs, P, Cn, b["means3D"], b["shs"], None, b["opacities"], b["scales"], b["rotations"], None, bg, view,
                            proj, campos, color, depth, alpha, radii, None, 1)
            a.geom_buffer, a.geom_tmp, a.image_buffer = _p(geom), _p(geom_tmp), _p(image)
            a.point_list, a.binning_tmp, a.sorted_rec, a.quad_list = _p(point_list), _p(bin_tmp), _p(sorted_rec), _p(quad_list)
            if deferred:
                _call("ogs_raster_forward_geometry", C.byref(a), st, None)
                _call("ogs_raster_read_num_rendered_async", C.byref(a), st, pinned.data_ptr())
                _call("ogs_raster_forward_render_deferred", C.byref(a), cap, st)
                return [color, depth, alpha, radii]
            n = C.c_int64(0)
            _call("ogs_raster_forward_geometry", C.byref(a), st, C.byref(n))
            _call("ogs_raster_forward_render", C.byref(a), int(n.value), st)
            bw = _lib.OgsRasterBwdArgs()
            bw.P, bw.W, bw.H, bw.C = P, W, H, Cn
            bw.sh_degree, bw.sh_coeffs = 3, 16
            bw.tanfovx, bw.tanfovy, bw.scale_modifier = float(rs.tanfovx), float(rs.tanfovy), 1.0
            bw.num_rendered, bw.num_groups, bw.bwd_tmp_is_clear = int(n.value), 1, 0
            bw.bg, bw.means3D, bw.shs, bw.opacities = _p(bg), _p(b["means3D"]), _p(b["shs"]), _p(b["opacities"])
            bw.scales, bw.rotations = _p(b["scales"]), _p(b["rotations"])
            bw.viewmatrix, bw.projmatrix, bw.campos = _p(view), _p(proj), _p(campos)
            bw.radii, bw.out_alpha, bw.dL_dcolor, bw.dL_dalpha = _p(radii), _p(alpha), _p(b["g_color"]), _p(b["g_alpha"])
            bw.geom_buffer, bw.image_buffer, bw.point_list, bw.bwd_tmp = _p(geom), _p(image), _p(point_list), _p(bwd_tmp)
            bw.sorted_rec, bw.quad_list = _p(sorted_rec), _p(quad_list)
            bw.dL_dmeans2D, bw.dL_dopacity, bw.dL_dmeans3D = _p(g_m2), _p(g_op), _p(g_m3)
            bw.dL_dsh, bw.dL_dscales, bw.dL_drotations = _p(g_sh), _p(g_scl), _p(g_rot)
            _call("ogs_raster_backward", C.byref(bw), st)
            return [color, depth, alpha, radii, g_m3, g_m2, g_op, g_scl, g_rot, g_sh]
        outs = [color, depth, alpha, radii] + ([] if deferred else [g_m3, g_m2, g_op, g_scl, g_rot, g_sh])
        return Prepared(inputs, run, out=outs, tmp=[geom, geom_tmp, image, point_list, bin_tmp, sorted_rec, quad_list, bwd_tmp])
    return build


def _c_group_stats(dev):
    """ogs_raster_forward_group_stats clears max_alpha, count and its fixed-point table itself; all three are dirtied first"""
    from opengaussian_amd import _lib
    from opengaussian_amd import rasterizer as R
    L = _lib.lib()
    P, G, Ln, Cn = 600, 3, 5, 3
    rs = _settings(dev)
    cap = P * ((W + 15) // 16) * ((H + 15) // 16)
    gb, gtb, _ = R._geom_sizes(P, W, H, Cn, 1)
    btb, _, _ = R._render_sizes(cap, W, H, Cn)
    geom, geom_tmp = _u8(gb, dev), _u8(gtb, dev)
    image, tmp = _u8(L.ogs_raster_stats_image_bytes(W, H, G), dev), _u8(L.ogs_raster_stats_tmp_bytes(G, Ln, Cn), dev)
    point_list, bin_tmp = torch.empty(cap, dtype=torch.int32, device=dev), _u8(btb, dev)
    max_alpha = torch.empty(G, dtype=torch.float32, device=dev)
    count = torch.empty(G, Ln + 1, dtype=torch.int64, device=dev)
    feat_sum = torch.empty(G, Ln + 1, Cn, dtype=torch.float32, device=dev)
    radii = torch.empty(P, dtype=torch.int32, device=dev)
    bg = torch.tensor(BG, device=dev)
    view, proj, campos = (t.to(dev).contiguous() for t in (rs.viewmatrix, rs.projmatrix, rs.campos))
    torch.cuda.synchronize()

    def inputs(seed):
        g = _gen(seed, 32)
        d = _scene(P, seed)
        d["cols"] = d.pop("ins_feat")[:, :3].contiguous()
        d.pop("shs")
        d["group"] = torch.randint(0, G + 1, (P,), generator=g).to(torch.int32)
        d["labels"] = torch.randint(-1, Ln, (H * W,), generator=g).to(torch.int32)
        return d

    def run(b, s):
        st = _st(s)
        a = R._fwd_args(rs, P, Cn, b["means3D"], None, b["cols"], b["opacities"], b["scales"], b["rotations"], None, bg, view, proj,
                        campos, None, None, None, radii, b["group"], G)
        a.geom_buffer, a.geom_tmp, a.image_buffer = _p(geom), _p(geom_tmp), _p(image)
        a.point_list, a.binning_tmp = _p(point_list), _p(bin_tmp)
        n = C.c_int64(0)
        _call("ogs_raster_forward_geometry", C.byref(a), st, C.byref(n))
        sa = _lib.OgsGroupStatsArgs()
        sa.labels, sa.num_labels, sa.alpha_threshold = _p(b["labels"]), Ln, 0.5
        sa.max_alpha, sa.count, sa.feat_sum, sa.stats_tmp = _p(max_alpha), _p(count), _p(feat_sum), _p(tmp)
        _call("ogs_raster_forward_group_stats", C.byref(a), C.byref(sa), int(n.value), st)
        return [max_alpha, count, feat_sum, radii]
    return Prepared(inputs, run, out=[max_alpha, count, feat_sum, radii], tmp=[geom, geom_tmp, image, tmp, point_list, bin_tmp])


def _c_tiny(raw):
    """ogs_raster_forward_tiny / _tiny_raw: two launches over geom_buffer and geom_tmp, both dirtied"""
    def build(dev):
        from opengaussian_amd import _lib
        from opengaussian_amd import rasterizer as R
        L = _lib.lib()
        P, Cn = 200, 3
        rs = _settings(dev)
        nmax = int(L.ogs_raster_tiny_max_points())
        geom, geom_tmp = _u8(L.ogs_raster_geom_bytes(nmax, 12), dev), _u8(L.ogs_raster_geom_tmp_bytes(nmax), dev)
        e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
        color, depth, alpha, radii = e(Cn, H, W), e(1, H, W), e(1, H, W), torch.empty(P, dtype=torch.int32, device=dev)
        bg = torch.tensor(BG, device=dev)
        view, proj, campos = (t.to(dev).contiguous() for t in (rs.viewmatrix, rs.projmatrix, rs.campos))
        torch.cuda.synchronize()

        def inputs(seed):
            d = _scene(P, seed)
            d.pop("ins_feat")
            d["rest"] = d["shs"][:, 1:].contiguous()
            d["dc"] = d["shs"][:, :1].contiguous()
            d["op_raw"] = torch.log(d["opacities"].clamp(1e-4, 1 - 1e-4) / (1 - d["opacities"].clamp(1e-4, 1 - 1e-4)))
            d["scl_raw"] = torch.log(d["scales"])
            return d

        def run(b, s):
            if raw:
                a = R._fwd_args(rs, P, Cn, b["means3D"], None, None, None, None, None, None, bg, view, proj, campos, color, depth,
                                alpha, radii, None, 1)
                a.sh_coeffs = 16
                rm = R._raw_model_struct(b["dc"], b["rest"], b["op_raw"], b["scl_raw"], b["rotations"])
            else:
                a = R._fwd_args(rs, P, Cn, b["means3D"], b["shs"], None, b["opacities"], b["scales"], b["rotations"], None, bg,
                                view, proj, campos, color, depth, alpha, radii, None, 1)
            a.geom_buffer, a.geom_tmp = _p(geom), _p(geom_tmp)
            if raw:
                _call("ogs_raster_forward_tiny_raw", C.byref(a), C.byref(rm), _st(s))
            else:
                _call("ogs_raster_forward_tiny", C.byref(a), _st(s))
            return [color, depth, alpha, radii]
        return Prepared(inputs, run, out=[color, depth, alpha, radii], tmp=[geom, geom_tmp])
    return build


def _c_raster_raw(dev):
    """ogs_raster_forward_geometry_raw (blocking count), the render phase, ogs_raster_backward_raw with a dirty gradient record"""
    from opengaussian_amd import _lib
    from opengaussian_amd import rasterizer as R
    L = _lib.lib()
    P, Cn, M = 800, 3, 16
    rs = _settings(dev)
    cap = P * ((W + 15) // 16) * ((H + 15) // 16)
    gb, gtb, ib = R._geom_sizes(P, W, H, Cn, 1)
    btb, srb, qlb = R._render_sizes(cap, W, H, Cn)
    e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
    color, depth, alpha, radii = e(Cn, H, W), e(1, H, W), e(1, H, W), torch.empty(P, dtype=torch.int32, device=dev)
    geom, geom_tmp, image = _u8(gb, dev), _u8(gtb, dev), _u8(ib, dev)
    point_list = torch.empty(cap, dtype=torch.int32, device=dev)
    bin_tmp, sorted_rec, quad_list = _u8(btb, dev), _u8(srb, dev), _u8(qlb, dev)
    bwd_tmp = _u8(L.ogs_raster_backward_tmp_bytes(P), dev)
    g_m3, g_m2, g_dc, g_rest, g_op, g_scl, g_rot = e(P, 3), e(P, 3), e(P, 1, 3), e(P, M - 1, 3), e(P, 1), e(P, 3), e(P, 4)
    bg = torch.tensor(BG, device=dev)
    view, proj, campos = (t.to(dev).contiguous() for t in (rs.viewmatrix, rs.projmatrix, rs.campos))
    torch.cuda.synchronize()

    def inputs(seed):
        sc = _scene(P, seed)
        g = _gen(seed, 36)
        op = sc["opacities"].clamp(1e-4, 1 - 1e-4)
        return {"means3D": sc["means3D"], "dc": sc["shs"][:, :1].contiguous(), "rest": sc["shs"][:, 1:].contiguous(),
                "op_raw": torch.log(op / (1 - op)), "scl_raw": torch.log(sc["scales"]), "rot_raw": sc["rotations"] * 1.5,
                "g_color": torch.randn(Cn, H, W, generator=g), "g_alpha": torch.randn(1, H, W, generator=g)}

    def run(b, s):
        st = _st(s)
        a = R._fwd_args(rs, P, Cn, b["means3D"], None, None, None, None, None, None, bg, view, proj, campos, color, depth, alpha,
                        radii, None, 1)
        a.sh_coeffs = M
        a.geom_buffer, a.geom_tmp, a.image_buffer = _p(geom), _p(geom_tmp), _p(image)
        a.point_list, a.binning_tmp, a.sorted_rec, a.quad_list = _p(point_list), _p(bin_tmp), _p(sorted_rec), _p(quad_list)
        rm = R._raw_model_struct(b["dc"], b["rest"], b["op_raw"], b["scl_raw"], b["rot_raw"])
        n = C.c_int64(0)
        _call("ogs_raster_forward_geometry_raw", C.byref(a), C.byref(rm), st, C.byref(n))
        # what the render phase's argument check wants to see (include/ogs_model.h): it reads none of them
        a.shs, a.opacities, a.scales, a.rotations = rm.features_dc, rm.opacity, rm.scaling, rm.rotation
        _call("ogs_raster_forward_render", C.byref(a), int(n.value), st)
        bw = _lib.OgsRasterBwdArgs()
        bw.P, bw.W, bw.H, bw.C = P, W, H, Cn
        bw.sh_degree, bw.sh_coeffs = 3, M
        bw.tanfovx, bw.tanfovy, bw.scale_modifier = float(rs.tanfovx), float(rs.tanfovy), 1.0
        bw.num_rendered, bw.num_groups, bw.bwd_tmp_is_clear = int(n.value), 1, 0
        bw.bg, bw.means3D = _p(bg), _p(b["means3D"])
        bw.viewmatrix, bw.projmatrix, bw.campos = _p(view), _p(proj), _p(campos)
        bw.radii, bw.out_alpha, bw.dL_dcolor, bw.dL_dalpha = _p(radii), _p(alpha), _p(b["g_color"]), _p(b["g_alpha"])
        bw.geom_buffer, bw.image_buffer, bw.point_list, bw.bwd_tmp = _p(geom), _p(image), _p(point_list), _p(bwd_tmp)
        bw.sorted_rec, bw.quad_list = _p(sorted_rec), _p(quad_list)
        bw.dL_dmeans2D, bw.dL_dmeans3D = _p(g_m2), _p(g_m3)
        gr = _lib.OgsRawModelGrads()
        gr.features_dc, gr.features_rest, gr.scaling, gr.rotation, gr.opacity = _p(g_dc), _p(g_rest), _p(g_scl), _p(g_rot), _p(g_op)
        _call("ogs_raster_backward_raw", C.byref(bw), C.byref(rm), C.byref(gr), st)
        return [color, depth, alpha, radii, g_m3, g_m2, g_dc, g_rest, g_op, g_scl, g_rot]
    return Prepared(inputs, run, out=[color, depth, alpha, radii, g_m3, g_m2, g_dc, g_rest, g_op, g_scl, g_rot],
                    tmp=[geom, geom_tmp, image, point_list, bin_tmp, sorted_rec, quad_list, bwd_tmp])


def _c_raster_kept(dev):
    """A 3-channel colour pass through the C ABI, then what reads the state it leaves: ogs_raster_read_num_emitted (a copy),
    ogs_raster_export_binning (a launch, a copy and a memset), ogs_raster_compact_kept into dirtied buffers, and
    ogs_raster_forward_reblend over the compacted state, which must give the pass's own images"""
    from opengaussian_amd import _lib
    from opengaussian_amd import rasterizer as R
    P, Cn = 1300, 3
    rs = _settings(dev)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    cap = P * tiles
    gb, gtb, ib = R._geom_sizes(P, W, H, Cn, 1)
    btb, srb, qlb = R._render_sizes(cap, W, H, Cn)
    e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
    color, depth, alpha, radii = e(Cn, H, W), e(1, H, W), e(1, H, W), torch.empty(P, dtype=torch.int32, device=dev)
    color2, depth2, alpha2 = e(Cn, H, W), e(1, H, W), e(1, H, W)
    geom, geom_tmp, image = _u8(gb, dev), _u8(gtb, dev), _u8(ib, dev)
    point_list = torch.empty(cap, dtype=torch.int32, device=dev)
    bin_tmp, sorted_rec, quad_list = _u8(btb, dev), _u8(srb, dev), _u8(qlb, dev)
    new_image, new_sorted, new_quad = _u8(ib, dev), _u8(srb, dev), _u8(qlb, dev)
    keys = torch.empty(cap, dtype=torch.int64, device=dev)
    ranges = torch.empty(tiles, 2, dtype=torch.int32, device=dev)
    ncontrib = torch.empty(H, W, dtype=torch.int32, device=dev)
    bg = torch.tensor(BG, device=dev)
    view, proj, campos = (t.to(dev).contiguous() for t in (rs.viewmatrix, rs.projmatrix, rs.campos))
    up = lambda n: (n + 255) // 256 * 256
    o_cnt = up(tiles * 8) + up(W * H * 4)                      # image_buffer layout: include/ogs_raster.h, ogs_raster_compact_kept
    torch.cuda.synchronize()

    def inputs(seed):
        d = _scene(P, seed)
        d["cols"] = d.pop("ins_feat")[:, :3].contiguous()
        d.pop("shs")
        return d

    def run(b, s):
        st = _st(s)
        a = R._fwd_args(rs, P, Cn, b["means3D"], None, b["cols"], b["opacities"], b["scales"], b["rotations"], None, bg, view, proj,
                        campos, color, depth, alpha, radii, None, 1)
        a.geom_buffer, a.geom_tmp, a.image_buffer = _p(geom), _p(geom_tmp), _p(image)
        a.point_list, a.binning_tmp, a.sorted_rec, a.quad_list = _p(point_list), _p(bin_tmp), _p(sorted_rec), _p(quad_list)
        n, emitted = C.c_int64(0), C.c_uint32(0)
        _call("ogs_raster_forward_geometry", C.byref(a), st, C.byref(n))
        _call("ogs_raster_forward_render", C.byref(a), int(n.value), st)
        _call("ogs_raster_read_num_emitted", C.byref(a), st, C.byref(emitted))
        _call("ogs_raster_export_binning", C.byref(a), int(n.value), _p(keys), _p(ranges), _p(ncontrib), st)
        with on(s):
            # as KeptPasses.admit: the records each tile packed, re-laid out by their exclusive scan
            packed = image[o_cnt:o_cnt + tiles * 20].view(torch.int32).view(tiles, 5)[:, 4].to(torch.int64)
            ends = torch.cumsum(packed, 0)
            new_image.copy_(image)
            new_image[: tiles * 8] = torch.stack((ends - packed, ends), 1).to(torch.int32).contiguous().view(-1).view(torch.uint8)
            listed = torch.where(torch.arange(cap, device=dev) < ranges[:, 1].max(), keys, torch.zeros_like(keys))
        _call("ogs_raster_compact_kept", W, H, Cn, _p(image), _p(sorted_rec), _p(quad_list), _p(new_image), _p(new_sorted),
              _p(new_quad), st)
        r = _lib.OgsRasterFwdArgs()
        r.P, r.W, r.H, r.C = P, W, H, Cn
        r.bg, r.colors_precomp = _p(bg), _p(b["cols"])
        r.out_color, r.out_depth, r.out_alpha = _p(color2), _p(depth2), _p(alpha2)
        r.image_buffer, r.sorted_rec, r.quad_list = _p(new_image), _p(new_sorted), _p(new_quad)
        _call("ogs_raster_forward_reblend", C.byref(r), st)
        with on(s):
            counts = torch.tensor([int(n.value), int(emitted.value)], dtype=torch.int64).to(dev)
        return [color, depth, alpha, radii, color2, depth2, alpha2, listed, ranges, ncontrib, counts]

    def check(o):
        for i, what in enumerate(("colour", "depth", "alpha")):
            if not torch.equal(o[i], o[4 + i]):
                return f"the re-blend of the compacted state gives another {what} image than the pass"
        return None
    return Prepared(inputs, run, out=[color, depth, alpha, radii, color2, depth2, alpha2, keys, ranges, ncontrib, new_sorted, new_quad],
                    tmp=[geom, geom_tmp, image, point_list, bin_tmp, sorted_rec, quad_list, new_image], check=check)


def _c_kmeans(dev):
    """ogs_kmeans_lloyd (a fill of counts and the ticket inside tmp, then 2 * iters + 1 launches), ogs_kmeans_accumulate (three
    launches over tmp), ogs_kmeans_update, ogs_kmeans_assign, ogs_kmeans_gather at k = 64, d = 9 (fixed summation order)"""
    from opengaussian_amd import _lib
    L = _lib.lib()
    N, d, k, iters = 3000, 9, 64, 3
    tmp = _u8(L.ogs_kmeans_tmp_bytes(N, d, k), dev)
    tmp2 = _u8(L.ogs_kmeans_tmp_bytes(N, d, k), dev)
    e = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device=dev)
    cent, ids, table, counts, cent2, ids2, out = e(k, d), e(N, dt=torch.int64), e(k, d + 1), e(k), e(k, d), e(N, dt=torch.int64), e(N, 6)

    def inputs(seed):
        return {"feat": torch.rand(N, d, generator=_gen(seed, 37))}

    def run(b, s):
        st = _st(s)
        with on(s):
            cent.copy_(b["feat"][:k])
            cent2.copy_(b["feat"][:k])
            counts.fill_(1e-6)
        _call("ogs_kmeans_lloyd", _p(b["feat"]), N, d, _p(cent), k, k, iters, 1, _p(ids), 0, _p(tmp), st)
        _call("ogs_kmeans_accumulate", _p(b["feat"]), N, d, _p(cent2), k, k, _p(table), _p(tmp2), st)
        _call("ogs_kmeans_update", _p(table), k, d, 1, _p(counts), _p(cent2), st)
        _call("ogs_kmeans_assign", _p(b["feat"]), N, d, _p(cent2), k, _p(ids2), 5, st)
        _call("ogs_kmeans_gather", _p(cent), _p(ids), N, d, 6, _p(out), st)
        return [cent, ids, table, counts, cent2, ids2, out]
    return Prepared(inputs, run, out=[ids, table, ids2, out], tmp=[tmp, tmp2])


def _c_densify(dev):
    """ogs_densify_plan (a flags launch, four scans over tmp, a copy, a synchronisation) and ogs_densify_map over the same tmp"""
    from opengaussian_amd import _lib
    L = _lib.lib()
    N = 1200
    tmp = _u8(L.ogs_densify_tmp_bytes(N), dev)
    src_row = torch.empty(4 * N, dtype=torch.int32, device=dev)       # n_out <= N old + N clones + 2 N children
    kind = torch.empty(4 * N, dtype=torch.uint8, device=dev)
    sample_row = torch.empty(4 * N, dtype=torch.int32, device=dev)

    def inputs(seed):
        g = _gen(seed, 38)
        return {"accum": torch.rand(N, generator=g) * 4e-4, "denom": torch.randint(1, 3, (N,), generator=g).to(torch.float32),
                "scaling": torch.randn(N, 3, generator=g) * 0.3 - 3.0, "opacity": torch.randn(N, generator=g)}

    def run(b, s):
        st = _st(s)
        a = _lib.OgsDensifyArgs()
        a.N = N
        a.grad_accum, a.denom, a.scaling, a.opacity = _p(b["accum"]), _p(b["denom"]), _p(b["scaling"]), _p(b["opacity"])
        a.max_grad, a.min_opacity, a.extent, a.percent_dense, a.prune_world_size = 2e-4, 0.005, 4.0, 0.01, 1
        totals = (C.c_uint32 * 4)()
        _call("ogs_densify_plan", C.byref(a), _p(tmp), totals, st)
        nA, nB, nC, S = (int(v) for v in totals)
        n_out = nA + nB + 2 * nC
        if n_out:
            _call("ogs_densify_map", N, _p(tmp), _p(src_row), _p(kind), _p(sample_row), st)
        with on(s):
            counts = torch.tensor([nA, nB, nC, S], dtype=torch.int64).to(dev)
        return [src_row[:n_out], kind[:n_out], sample_row[:n_out], counts]
    return Prepared(inputs, run, out=[src_row, kind, sample_row], tmp=[tmp])


def _c_query_text(dev):
    """ogs_query_select with and without the ranking, ogs_query_classify (two launches)"""
    Q, K, D, N = 5, 300, 64, 4000
    e = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device=dev)
    sim, selected, count = e(Q, K), e(Q, 10, dt=torch.int32), e(Q, dt=torch.int32)
    cls, pred = e(K, dt=torch.int32), e(N, dt=torch.int64)

    def inputs(seed):
        g = _gen(seed, 39)
        return {"text": torch.randn(Q, D, generator=g), "leaf": torch.randn(K, D, generator=g),
                "valid": (torch.rand(K, generator=g) < 0.6).to(torch.uint8), "centers": torch.rand(K + 1, 6, generator=g),
                "leaf_ind": torch.randint(0, K, (N,), generator=g)}

    def run(b, s):
        st = _st(s)
        _call("ogs_query_select", Q, K, D, _p(b["text"]), _p(b["leaf"]), _p(b["valid"]), _p(b["centers"]), 6, 10.0, 0.9, 10,
              _p(sim), _p(selected), _p(count), st)
        _call("ogs_query_classify", N, _p(b["leaf_ind"]), K, Q, _p(sim), _p(cls), _p(pred), st)
        return [sim, selected, count, cls, pred]
    return Prepared(inputs, run, out=[sim, selected, count, cls, pred])


def _c_radix(variant):
    def build(dev):
        """the radix self-test: three launches per pass (variant 0) or one launch per pass with look-back (variant 1), 4 passes"""
        from opengaussian_amd import _lib
        L = _lib.lib()
        n = 5000
        keys1 = torch.empty(n, dtype=torch.int32, device=dev)
        vals0 = torch.empty(n, dtype=torch.int32, device=dev)
        vals1 = torch.empty(n, dtype=torch.int32, device=dev)
        keys0 = torch.empty(n, dtype=torch.int32, device=dev)
        tmp = _u8(L.ogs_selftest_radix_tmp_bytes(n), dev)

        def inputs(seed):
            g = _gen(seed, 33)
            keys = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g).to(torch.int32)
            keys[torch.rand(n, generator=g) < 0.3] = -1                 # 0xFFFFFFFF: what the drop mode leaves out
            return {"keys": keys}

        def run(b, s):
            with on(s):
                keys0.copy_(b["keys"])
                vals0.copy_(torch.arange(n, dtype=torch.int32, device=dev))
            res = C.c_int32(-1)
            _call("ogs_selftest_radix_sort", _p(keys0), _p(vals0), _p(keys1), _p(vals1), n, 32, variant, 0, None, _p(tmp),
                  C.byref(res), _st(s))
            k, v = ((keys0, vals0), (keys1, vals1))[res.value & 1]
            kept = (res.value >> 1) if variant & 2 else n
            return [k[:kept], v[:kept]]
        return Prepared(inputs, run, out=[keys1, vals1], tmp=[tmp])
    return build


def _c_scan(dev):
    """the scan self-test on its two-launch route (reduce, apply), with everything optional: a gather, a device-side count
    below the capacity and the total.  The outputs past the count are not written: they keep the harness's dirt in every run."""
    from opengaussian_amd import _lib
    L = _lib.lib()
    n, m = 5000, 2503
    out = torch.empty(n, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    tmp = _u8(L.ogs_selftest_scan_tmp_bytes(n), dev)

    def inputs(seed):
        g = _gen(seed, 34)
        return {"in": torch.randint(0, 301, (m,), generator=g).to(torch.int32),
                "gather": torch.randint(0, m, (n,), generator=g).to(torch.int32),
                "n_dev": torch.randint(2500, n + 1, (1,), generator=g).to(torch.int32)}

    def run(b, s):
        _call("ogs_selftest_scan_u32", _p(b["in"]), _p(b["gather"]), _p(out), n, _p(total), _p(b["n_dev"]), _p(tmp), _st(s))
        return [out, total]
    return Prepared(inputs, run, out=[out, total], tmp=[tmp])


# ---- the table -------------------------------------------------------------------------------------------------------------------
GEOM, RENDER, BACKWARD = "ogs_raster_forward_geometry", "ogs_raster_forward_render", "ogs_raster_backward"
DEFER = ("ogs_raster_read_num_rendered_async", "ogs_raster_forward_render_deferred")

CASES = [
    # rasterizer, Python level
    Case("raster_tiny_forward", _raster(200, backward=False), ("ogs_raster_forward_tiny",), sentence=ASYNC_TINY),
    Case("raster_tiny_backward", _raster(200), ("ogs_raster_forward_tiny", GEOM, BACKWARD), blocks_host=True,
         sentence=BLOCK_TINY_BWD, compare=_raster_compare(True, 5), bar_from=RASTER_BAR),
    Case("raster_streaming_blocking", _raster(800, blocking=True), (GEOM, RENDER, BACKWARD), blocks_host=True,
         sentence=BLOCK_GEOMETRY, compare=_raster_compare(True, 5), bar_from=RASTER_BAR),
    Case("raster_streaming_deferred", _raster(800), (GEOM, *DEFER, BACKWARD), blocks_host=True, sentence=BLOCK_DEFERRED_PY,
         compare=_raster_compare(True, 5), bar_from=RASTER_BAR),
    Case("raster_emitted_debug", _raster(1300, backward=False, emitted=True), (GEOM, "ogs_raster_read_num_emitted"),
         blocks_host=True, sentence=BLOCK_EMITTED),
    Case("rasterize_fused", _raster(600, "fused"), (GEOM, BACKWARD), blocks_host=True, sentence=BLOCK_DEFERRED_PY,
         compare=_raster_compare(True, 6), bar_from=RASTER_BAR),
    Case("rasterize_groups", _raster(600, "groups", blocking=True), (GEOM, RENDER, BACKWARD), blocks_host=True,
         sentence=BLOCK_GROUPED, compare=_raster_compare(True, 5), bar_from=RASTER_BAR),
    Case("rasterize_group_stats", _group_stats, (GEOM, "ogs_raster_forward_group_stats"), blocks_host=True, sentence=BLOCK_GROUPED),
    Case("rasterize_model_streaming", _raster_model(600, True),
         ("ogs_raster_forward_geometry_raw", "ogs_raster_backward_raw", "ogs_model_activate"), blocks_host=True,
         sentence=BLOCK_DEFERRED_PY, compare=[BITS] * 8 + [RASTER_GRAD] * 6, bar_from=RASTER_BAR),
    Case("rasterize_model_tiny", _raster_model(200, False), ("ogs_raster_forward_tiny_raw", "ogs_model_activate"),
         sentence="include/ogs_model.h: the raw entry points keep the contract of include/ogs_raster.h; " + ASYNC_TINY),
    Case("visible_radii_markVisible", _visible, (GEOM, "ogs_mark_visible"), sentence=ASYNC_GEOM_NULL),
    Case("kept_pass_walks", _kept_walks, ("ogs_raster_label_map", "ogs_raster_label_votes", "ogs_raster_feature_votes",
                                          "ogs_raster_feature_map"), sentence=ASYNC_QUERY_WALK,
         fixed_outputs=(3, 7)),
    Case("render_full_pass", _render(False), (GEOM, BACKWARD), blocks_host=True, sentence=BLOCK_DEFERRED_PY,
         compare=[BITS] * 4 + [RASTER_GRAD], bar_from=RASTER_BAR,
         fixed_outputs=(0, 2, 3)),
    Case("render_kept_reblend", _render(True), ("ogs_raster_forward_reblend", BACKWARD), sentence=ASYNC_REBLEND,
         compare=[BITS] * 4 + [RASTER_GRAD], bar_from=RASTER_BAR,
         fixed_outputs=(0, 2, 3)),
    Case("kept_pass_admit_then_reblend", _kept_admit, (GEOM, "ogs_raster_compact_kept", "ogs_raster_forward_reblend", BACKWARD),
         blocks_host=True, sentence=BLOCK_KEPT_ADMIT, compare=[BITS] * 8 + [RASTER_GRAD], bar_from=RASTER_BAR),
    Case("render_feature_map_backward", _feature_map_backward, (GEOM, "ogs_raster_feature_map", "ogs_raster_feature_votes"),
         blocks_host=True, sentence=BLOCK_DEFERRED_PY,
         fixed_outputs=(1,)),
    # masks, losses
    Case("mask_stack", _masks("mask"), ("ogs_mask_feature_sums", "ogs_mask_feature_sums_backward", "ogs_mask_feature_sqdev",
                                        "ogs_mask_cohesion", "ogs_mask_cohesion_backward", "ogs_separation_loss"),
         compare=MASK_COMPARE, bar_from=MASK_BAR),
    Case("mask_labels", _masks("label"), ("ogs_label_feature_sums", "ogs_label_feature_sums_backward", "ogs_label_feature_sqdev",
                                          "ogs_label_cohesion", "ogs_label_cohesion_backward", "ogs_separation_loss"),
         compare=MASK_COMPARE, bar_from=MASK_BAR),
    Case("image_losses", _losses, ("ogs_loss_photometric_forward", "ogs_loss_photometric_backward", "ogs_loss_masked_forward",
                                   "ogs_loss_masked_backward")),
    # optimiser, densification
    Case("fused_adam_step", _adam, ("ogs_adam_step",), sentence=ASYNC_ADAM),
    Case("add_densification_stats", _densify("stats"), ("ogs_densify_stats",)),
    Case("prune_points", _densify("prune"), ("ogs_rows_gather",)),
    Case("densify_and_prune", _densify("densify"), ("ogs_densify_plan", "ogs_densify_map", "ogs_rows_gather",
                                                    "ogs_densify_split_children"), blocks_host=True, sentence=BLOCK_PLAN),
    # k-means
    Case("quantize_kmeans", _quantize, ("ogs_kmeans_lloyd", "ogs_kmeans_gather", "ogs_kmeans_accumulate", "ogs_kmeans_update",
                                        "ogs_kmeans_assign"),
         bar_from="tests/test_21_kmeans_edges_gpu.py::test_two_identical_calls_give_the_same_bits[A4]"),
    Case("wide_kmeans", _wide, ("ogs_kmeans_wide_assign", "ogs_kmeans_wide_update", "ogs_kmeans_wide_lloyd", "ogs_kmeans_wide_seed"),
         sentence=ASYNC_WIDE,
         fixed_outputs=(13,)),
    Case("build_codebook_seeded", _codebook, ("ogs_kmeans_wide_seed", "ogs_kmeans_wide_lloyd"), blocks_host=True,
         sentence=BLOCK_CODEBOOK),
    # kNN
    Case("knn_lists", _knn_lists, ("ogs_knn_neighbors", "ogs_knn_index_build", "ogs_knn_query", "ogs_knn_radius_count",
                                   "ogs_knn_dbscan", "ogs_knn_components", "ogs_knn_transpose"), sentence=ASYNC_KNN_PY),
    Case("knn_filters", _knn_filters, ("ogs_knn_group_ksum", "ogs_knn_neighbors"), sentence=ASYNC_KNN),
    Case("knn_graph", _knn_graph, ("ogs_knn_aggregate", "ogs_knn_aggregate_t", "ogs_knn_edge_dots", "ogs_knn_transpose",
                                   "ogs_knn_smoothness_fwd", "ogs_knn_smoothness_bwd"), sentence=ASYNC_KNN),
    # query
    Case("query_text", _query_text, ("ogs_query_select", "ogs_query_classify"), sentence=ASYNC_SELECT),
    Case("query_tables", _query_tables, ("ogs_query_confusion", "ogs_query_split_count", "ogs_query_split_scan",
                                         "ogs_query_split_scatter"), blocks_host=True, sentence=BLOCK_CONFUSION + "; " + BLOCK_SPLIT),
    # other
    Case("refine_sam_masks", _refine, ("ogs_refine_visibility", "ogs_refine_footprint_labels", "ogs_refine_footprint_labels_block",
                                       "ogs_refine_vote", "ogs_refine_expand", "ogs_refine_finalize", GEOM),
         blocks_host=True, sentence=BLOCK_REFINE),
    Case("sh_grad_exchange_rebuild", _sh_exchange, ("ogs_sh_grad_from_views",)),
    # the C ABI, caller-owned buffers dirtied on the stream
    Case("c_knn_radius_dbscan", _c_knn_radius, ("ogs_knn_index_build", "ogs_knn_radius_count", "ogs_knn_dbscan"), "c",
         sentence=ASYNC_KNN),
    Case("c_knn_graph", _c_knn_graph, ("ogs_knn_transpose", "ogs_knn_smoothness_fwd", "ogs_knn_smoothness_bwd", "ogs_knn_components",
                                       "ogs_knn_aggregate_t"), "c", sentence=ASYNC_KNN),
    Case("c_wide_kmeans", _c_wide, ("ogs_kmeans_wide_assign", "ogs_kmeans_wide_update", "ogs_kmeans_wide_inertia",
                                    "ogs_kmeans_wide_lloyd", "ogs_kmeans_wide_seed"), "c", sentence=ASYNC_WIDE + " / " + ASYNC_SEED,
         fixed_outputs=(14,)),
    Case("c_query_tables", _c_query, ("ogs_query_confusion", "ogs_query_split_count", "ogs_query_split_scan",
                                      "ogs_query_split_scatter"), "c"),
    Case("c_mask_sums", _c_masks("mask"), ("ogs_mask_feature_sums", "ogs_mask_feature_sums_backward", "ogs_mask_cohesion",
                                           "ogs_mask_cohesion_backward"), "c", compare=C_MASK_COMPARE, bar_from=MASK_BAR),
    Case("c_label_sums", _c_masks("label"), ("ogs_label_feature_sums", "ogs_label_feature_sums_backward", "ogs_label_cohesion",
                                             "ogs_label_cohesion_backward"), "c", compare=C_MASK_COMPARE, bar_from=MASK_BAR),
    Case("c_raster_deferred_forward", _c_raster(True), (GEOM, *DEFER), "c", sentence=ASYNC_DEFERRED),
    Case("c_raster_forward_backward", _c_raster(False), (GEOM, RENDER, BACKWARD), "c", blocks_host=True, sentence=BLOCK_GEOMETRY,
         compare=[BITS] * 4 + [RASTER_GRAD] * 6, bar_from=RASTER_BAR),
    Case("c_raster_group_stats", _c_group_stats, (GEOM, "ogs_raster_forward_group_stats"), "c", blocks_host=True,
         sentence=BLOCK_GEOMETRY),
    Case("c_raster_tiny", _c_tiny(False), ("ogs_raster_forward_tiny",), "c", sentence=ASYNC_TINY),
    Case("c_raster_tiny_raw", _c_tiny(True), ("ogs_raster_forward_tiny_raw",), "c",
         sentence="include/ogs_model.h: the raw entry points keep the contract of include/ogs_raster.h; " + ASYNC_TINY),
    Case("c_raster_raw_forward_backward", _c_raster_raw, ("ogs_raster_forward_geometry_raw", RENDER, "ogs_raster_backward_raw"), "c",
         blocks_host=True, sentence=BLOCK_GEOMETRY, compare=[BITS] * 4 + [RASTER_GRAD] * 7, bar_from=RASTER_BAR),
    Case("c_raster_kept_state", _c_raster_kept, (GEOM, RENDER, "ogs_raster_read_num_emitted", "ogs_raster_export_binning",
                                                 "ogs_raster_compact_kept", "ogs_raster_forward_reblend"), "c", blocks_host=True,
         sentence=BLOCK_GEOMETRY + "; " + BLOCK_EMITTED),
    Case("c_kmeans", _c_kmeans, ("ogs_kmeans_lloyd", "ogs_kmeans_accumulate", "ogs_kmeans_update", "ogs_kmeans_assign",
                                 "ogs_kmeans_gather"), "c",
         fixed_outputs=(3,)),
    Case("c_densify_plan_map", _c_densify, ("ogs_densify_plan", "ogs_densify_map"), "c", blocks_host=True, sentence=BLOCK_PLAN),
    Case("c_query_text", _c_query_text, ("ogs_query_select", "ogs_query_classify"), "c"),
    Case("c_radix_three_launches", _c_radix(0), ("ogs_selftest_radix_sort",), "c", blocks_host=True, sentence=BLOCK_RADIX),
    Case("c_radix_one_launch", _c_radix(1), ("ogs_selftest_radix_sort",), "c", blocks_host=True, sentence=BLOCK_RADIX),
    Case("c_radix_drop_mode", _c_radix(3), ("ogs_selftest_radix_sort",), "c", blocks_host=True, sentence=BLOCK_RADIX),
    Case("c_losses", _c_losses, ("ogs_loss_photometric_forward", "ogs_loss_photometric_backward", "ogs_loss_masked_forward",
                                 "ogs_loss_masked_backward", "ogs_separation_loss"), "c"),
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Cases of self-test hooks.  CASES is what profiles/stream_contract.json holds, name by name; these are what
# profiles/stream_contract_hooks.json holds, name by name (`python -m tests.stream_harness --measure` writes both), and the one
# delay of the tests is held against the host times of both files.  Everything that walks the table walks these too:
# tests/test_80_stream_contract_gpu.py runs them behind the delay like any case, tests/test_stream_table_host.py counts them
# and demands their profile entries.  A hook only: every entry point of the product belongs in CASES.
HOOK_CASES = [
    Case("c_scan_gather_count_total", _c_scan, ("ogs_selftest_scan_u32",), "c", sentence=ASYNC_SCAN),
]
ALL_CASES = CASES + HOOK_CASES
ALL_BY_NAME = {c.name: c for c in ALL_CASES}
assert len(ALL_BY_NAME) == len(ALL_CASES)
