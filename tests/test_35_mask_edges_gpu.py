"""GPU: the dense-stack mask kernels (mask_ops.mask_feature_mean / cohesion_loss over csrc/mask_ops.hip) at the edges of
their tiling -- a lane owns 4 pixels, a wave a 256-pixel strip, a workgroup 1024 pixels, the stack is walked 8 masks at a
time, and a pointer that is not 16-byte aligned takes the scalar loads -- against oracle/mask_oracle.py in float64 on the
CPU.  The project's bars: values rtol 2e-5 / atol 1e-6, gradients 1e-4 of the largest entry, counts exact, the variance
2e-4 relative.  The separation loss has no part here (tests/test_34_separation_edges_gpu.py): the scalar under the
gradient is mean.square().sum() + cohesion, as in test_30's full-size test, so that no rank decision enters.

The variance of mask_feature_mean(return_var=True) where it cancels, measured on an MI355X (relative error against the
float64 oracle on the large mask; printed by test_variance_of_smooth_features):
  one level:  two-pass float32 on the CPU 1.8e-08; the device, stack and label image, two calls each: 7.5e-08 .. 1.1e-07
  two levels: two-pass float32 on the CPU 4.8e-08; the device: 4.8e-08 .. 4.1e-07;  the 300-pixel mask: 3.1e-08 at worst
  The one-pass form sum f^2 - 2 mean sum f + n mean^2 these calls replaced (scripts/mask_bench.py --variance, one level,
  8 calls): 8.1e-06 .. 1.4e-04 on the stack, 1.0e-05 .. 9.1e-05 on the label image -- under the 2e-4 bar in those calls,
  a third of what a CPU emulation of its summation order predicted, and different on every call.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# H*W -> (H, W): rows of one pixel height, or near-square images
SHAPES = {1: (1, 1), 3: (1, 3), 4: (2, 2), 5: (1, 5), 255: (15, 17), 256: (16, 16), 257: (1, 257), 1023: (31, 33),
          1024: (32, 32), 1025: (25, 41), 1028: (4, 257), 2051: (7, 293)}


def near(a, b, rtol=2e-5, atol=1e-6):
    np.testing.assert_allclose(a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy(), rtol=rtol, atol=atol)


def grad_near(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max())


def stage(mod, fm, masks, sw):
    """mean.square().sum() + cohesion, differentiated; float64 throughout when `mod` is the oracle"""
    from oracle import mask_oracle as mo
    kw = {"dtype": torch.float64} if mod is mo else {}
    mean = mod.mask_feature_mean(fm, masks, image_mask=sw, **kw)
    coh = mod.cohesion_loss(fm, masks, mean, **kw)
    (mean.square().sum() + coh).backward()
    return mean.detach(), coh.detach()


def against_oracle(gpu_device, feat, masks, sil):
    """values, counts, variance and both gradients of one case; feat [C,H,W], masks [N,H,W] bool, sil [1,H,W] or None (CPU)"""
    from opengaussian_amd import mask_ops as mk
    from oracle import mask_oracle as mo
    f64 = feat.double().requires_grad_(True)
    s64 = None if sil is None else sil.double().requires_grad_(True)
    mean_ref, coh_ref = stage(mo, f64, masks, s64)
    fm = feat.to(gpu_device).requires_grad_(True)
    sw = None if sil is None else sil.to(gpu_device).requires_grad_(True)
    mg = masks.to(gpu_device)
    mean, coh = stage(mk, fm, mg, sw)
    near(mean, mean_ref)
    near(coh, coh_ref)
    grad_near(fm.grad, f64.grad)
    if sil is not None:
        grad_near(sw.grad, s64.grad)
    _, var_ref, cnt_ref = mo.mask_feature_mean(feat, masks, return_var=True, dtype=torch.float64)
    mean_v, var, cnt = mk.mask_feature_mean(feat.to(gpu_device), mg, return_var=True)
    near(mean_v, mo.mask_feature_mean(feat, masks, dtype=torch.float64))
    near(var, var_ref, rtol=2e-4, atol=1e-7)
    assert torch.equal(cnt.cpu().double(), cnt_ref)                       # unweighted counts: integers, exact


# ---- pixel counts around the lane, the wave strip and the workgroup strip -----------------------------------------------
def edge_masks(HW, N, g):
    m = torch.zeros(N, HW, dtype=torch.bool)
    m[0, HW - 1] = True                                                  # only the last pixel: one lane of the last partial strip
    m[1, 0] = True                                                       # only pixel 0
    m[3] = True                                                          # full; m[2] stays empty
    m[4:] = torch.rand(N - 4, HW, generator=g) < 0.3                     # overlapping
    return m


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("C", [3, 6])
@pytest.mark.parametrize("HW", list(SHAPES))
def test_pixel_counts(gpu_device, HW, C, weighted):
    """1, 3, 5: the scalar tail (i0 + j < n); 4, 1028: the float4 tail (i0 < n); 255 .. 257 and 1023 .. 1025: one pixel
    short of, exactly and one past a wave's and a workgroup's strip; 2051: three workgroups, odd"""
    H, W = SHAPES[HW]
    g = torch.Generator().manual_seed(35 * HW + C)
    feat = torch.rand(C, H, W, generator=g)
    sil = torch.rand(1, H, W, generator=g) * 0.9 + 0.05 if weighted else None
    against_oracle(gpu_device, feat, edge_masks(HW, 9, g).view(9, H, W), sil)


# ---- stack sizes around the walk's unroll of 8 --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ones", "hole"])
@pytest.mark.parametrize("HW", [1025, 1028])
@pytest.mark.parametrize("N", [1, 7, 8, 9, 16, 17])
def test_stack_sizes(gpu_device, N, HW, kind):
    """ones: every mask holds every pixel (overlap everywhere; a dropped or repeated mask of the last partial group of 8
    shows in every sum); hole: random masks, with the first pixel, one in the middle and the last in no mask at all"""
    H, W = SHAPES[HW]
    g = torch.Generator().manual_seed(1000 * N + HW)
    feat = torch.rand(6, H, W, generator=g)
    sil = torch.rand(1, H, W, generator=g) * 0.9 + 0.05
    if kind == "ones":
        masks = torch.ones(N, HW, dtype=torch.bool)
    else:
        masks = torch.rand(N, HW, generator=g) < 0.5
        masks[:, [0, 513, HW - 1]] = False
    against_oracle(gpu_device, feat, masks.view(N, H, W), sil)
    if kind == "hole":
        from opengaussian_amd import mask_ops as mk
        fm = feat.to(gpu_device).requires_grad_(True)
        sw = sil.to(gpu_device).requires_grad_(True)
        stage(mk, fm, masks.view(N, H, W).to(gpu_device), sw)
        for p in (0, 513, HW - 1):                                       # a pixel in no mask: exactly zero gradients
            assert float(fm.grad.flatten(1)[:, p].abs().max()) == 0.0 and float(sw.grad.flatten()[p]) == 0.0


# ---- each backward kernel on its own --------------------------------------------------------------------------------------
def overlapping_case(seed=17, C=6, N=17, HW=1025):
    H, W = SHAPES[HW]
    g = torch.Generator().manual_seed(seed)
    feat = torch.rand(C, H, W, generator=g)
    masks = (torch.rand(N, H, W, generator=g) < 0.4)
    masks[N - 1] = False
    sil = torch.rand(1, H, W, generator=g) * 0.9 + 0.05
    mean = torch.rand(N, C, generator=g)
    coef = torch.randn(N, C, generator=g)
    return feat, masks, sil, mean, coef


def test_cohesion_backward_with_an_independent_mean(gpu_device):
    """dmean alone (the mean a leaf, the map constant) and dfeat alone (the map a leaf, the mean constant), under an
    upstream scale of 2.5; overlapping masks at C = 6, N = 17"""
    from opengaussian_amd import mask_ops as mk
    from oracle import mask_oracle as mo
    feat, masks, _, mean, _ = overlapping_case()
    fg, mg = feat.to(gpu_device), masks.to(gpu_device)
    mu64 = mean.double().requires_grad_(True)
    ref = mo.cohesion_loss(feat.double(), masks, mu64, dtype=torch.float64)
    (2.5 * ref).backward()
    mu = mean.to(gpu_device).requires_grad_(True)
    got = mk.cohesion_loss(fg, mg, mu)
    (2.5 * got).backward()
    near(got, ref)
    grad_near(mu.grad, mu64.grad)
    assert float(mu.grad[-1].abs().max()) == 0.0                         # the empty mask
    f64 = feat.double().requires_grad_(True)
    (2.5 * mo.cohesion_loss(f64, masks, mean.double(), dtype=torch.float64)).backward()
    fm = fg.clone().requires_grad_(True)
    (2.5 * mk.cohesion_loss(fm, mg, mean.to(gpu_device))).backward()
    grad_near(fm.grad, f64.grad)


@pytest.mark.parametrize("wshape", ["hw", "1hw"])
def test_sums_backward_weight_and_map_apart(gpu_device, wshape):
    """the scalar is sum(mean * coef) with a random coef, so that the count column of the table carries a gradient:
    dweight = sum_n mask * (sum_c coef feat + coef_cnt).  The weight a leaf and the map constant, then the reverse;
    weights of shape [H, W] and [1, H, W] (the gradient comes back in the shape given)"""
    from opengaussian_amd import mask_ops as mk
    from oracle import mask_oracle as mo
    feat, masks, sil, _, coef = overlapping_case(seed=18)
    if wshape == "hw":
        sil = sil[0]
    fg, mg, cg = feat.to(gpu_device), masks.to(gpu_device), coef.to(gpu_device)
    s64 = sil.double().requires_grad_(True)
    ref = mo.mask_feature_mean(feat.double(), masks, image_mask=s64, dtype=torch.float64)
    (ref * coef.double()).sum().backward()
    sw = sil.to(gpu_device).requires_grad_(True)
    got = mk.mask_feature_mean(fg, mg, image_mask=sw)
    (got * cg).sum().backward()
    near(got, ref)
    assert sw.grad.shape == sil.shape
    grad_near(sw.grad, s64.grad)
    f64 = feat.double().requires_grad_(True)
    (mo.mask_feature_mean(f64, masks, image_mask=sil.double(), dtype=torch.float64) * coef.double()).sum().backward()
    fm = fg.clone().requires_grad_(True)
    (mk.mask_feature_mean(fm, mg, image_mask=sil.to(gpu_device)) * cg).sum().backward()
    grad_near(fm.grad, f64.grad)


# ---- pointers the vector path cannot take -----------------------------------------------------------------------------------
def offset_view(t, requires_grad=False):
    """(base, view): `t` as a contiguous view one element into a larger buffer on t's device"""
    base = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    base[1:] = t.flatten()
    base.requires_grad_(requires_grad)
    return base, base[1:].view(t.shape)


@pytest.mark.parametrize("which", ["feat", "masks", "weight", "all"])
def test_views_at_an_odd_storage_offset(gpu_device, which):
    """H*W = 1028 is a multiple of 4, so only the pointer test of vec_ok keeps these calls off the float4 / u32 loads:
    the map and the weight 4 bytes, the bool stack 1 byte into their buffers.  Equal to the aligned call and the oracle;
    the gradients arrive in the views' bases, one element in"""
    from opengaussian_amd import mask_ops as mk
    from oracle import mask_oracle as mo
    feat, masks, sil, _, _ = overlapping_case(seed=19, N=9, HW=1028)
    f64, s64 = feat.double().requires_grad_(True), sil.double().requires_grad_(True)
    mean_ref, coh_ref = stage(mo, f64, masks, s64)
    fa = feat.to(gpu_device).requires_grad_(True)
    sa = sil.to(gpu_device).requires_grad_(True)
    ma = masks.to(gpu_device)
    assert fa.data_ptr() % 16 == 0 and sa.data_ptr() % 16 == 0 and ma.data_ptr() % 4 == 0
    mean_a, coh_a = stage(mk, fa, ma, sa)
    fbase, fv = offset_view(feat.to(gpu_device), True) if which in ("feat", "all") else (None, feat.to(gpu_device).requires_grad_(True))
    sbase, sv = offset_view(sil.to(gpu_device), True) if which in ("weight", "all") else (None, sil.to(gpu_device).requires_grad_(True))
    mv = offset_view(ma)[1] if which in ("masks", "all") else ma
    if fbase is not None:
        assert fv.is_contiguous() and fv.data_ptr() % 16 == 4
    if sbase is not None:
        assert sv.is_contiguous() and sv.data_ptr() % 16 == 4
    if mv is not ma:
        assert mv.is_contiguous() and mv.dtype == torch.bool and mv.data_ptr() % 4 == 1
    mean, coh = stage(mk, fv, mv, sv)
    for want_mean, want_coh in ((mean_a, coh_a), (mean_ref, coh_ref)):
        near(mean, want_mean)
        near(coh, want_coh)
    if fbase is not None:
        assert float(fbase.grad[0]) == 0.0
        dfeat = fbase.grad[1:].view(feat.shape)
    else:
        dfeat = fv.grad
    if sbase is not None:
        assert float(sbase.grad[0]) == 0.0
        dsil = sbase.grad[1:].view(sil.shape)
    else:
        dsil = sv.grad
    for want_f, want_s in ((fa.grad, sa.grad), (f64.grad, s64.grad)):
        grad_near(dfeat, want_f)
        grad_near(dsil, want_s)


# ---- dtype and layout of the stack ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["uint8", "int32", "float", "onehot_int64"])
def test_stack_dtypes_and_layouts(gpu_device, form):
    """0/1 stacks of other types, and the permuted (non-contiguous) int64 one-hot of get_SAM_mask_and_feat, against the
    bool stack.  (Values other than 0 / 1 are outside the documented contract: nothing is asserted on them.)"""
    from opengaussian_amd import mask_ops as mk
    feat, masks, sil, _, _ = overlapping_case(seed=20, N=9, HW=1025)
    fa, sa = feat.to(gpu_device).requires_grad_(True), sil.to(gpu_device).requires_grad_(True)
    mean_a, coh_a = stage(mk, fa, masks.to(gpu_device), sa)
    mg = masks.to(gpu_device)
    if form == "onehot_int64":
        other = mg.permute(1, 2, 0).long().contiguous().permute(2, 0, 1)
        assert not other.is_contiguous()
    else:
        other = mg.to({"uint8": torch.uint8, "int32": torch.int32, "float": torch.float32}[form])
    fm, sw = feat.to(gpu_device).requires_grad_(True), sil.to(gpu_device).requires_grad_(True)
    mean, coh = stage(mk, fm, other, sw)
    near(mean, mean_a)
    near(coh, coh_a)
    grad_near(fm.grad, fa.grad)
    grad_near(sw.grad, sa.grad)


# ---- the variance where it cancels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2])
def test_variance_of_smooth_features(gpu_device, levels):
    """association.pseudo_labels thresholds this variance at 0.006 on rendered features that are smooth inside a mask: a
    constant per channel plus 0.05 of noise (plus, with two levels, a second constant on half of the blocks).  There
    sum f^2 - 2 mean sum f + n mean^2 loses to cancellation what sum (f - mean)^2 keeps.  One mask of about 85 % of
    360 x 640, one of a few hundred pixels, one empty; dense stack and label image; two calls (the sums arrive through
    float atomics in another order every time)"""
    from opengaussian_amd import mask_ops as mk
    from oracle import mask_oracle as mo
    C, H, W, BAR = 6, 360, 640, 2e-4
    g = torch.Generator().manual_seed(3600 + levels)
    level = torch.tensor([0.9, -0.8, 0.5, 0.7, -0.6, 0.3])[:, None, None]
    feat = level + 0.05 * torch.randn(C, H, W, generator=g)
    if levels == 2:
        blocks = (torch.arange(H)[:, None] // 40 + torch.arange(W)[None, :] // 40) % 2
        feat = feat + 0.08 * blocks
    labels = torch.zeros(H, W, dtype=torch.long)
    labels[:, :544] = 1                                                  # 85 % of the pixels
    labels[100:115, 600:620] = 2                                         # 300 pixels
    masks = torch.stack([labels == 1, labels == 2, labels == 3])
    assert int(masks[0].sum()) == 360 * 544 and int(masks[1].sum()) == 300 and int(masks[2].sum()) == 0
    mean_ref, var_ref, cnt_ref = mo.mask_feature_mean(feat, masks, return_var=True, dtype=torch.float64)
    var32 = mo.mask_feature_mean(feat, masks, return_var=True, dtype=torch.float32)[1]
    rel = lambda v: ((v.double().cpu() - var_ref).abs() / var_ref.clamp_min(1e-30))[:2]
    assert float(rel(var32).max()) <= BAR                                # input condition: two-pass float32 is good enough
    fg = feat.to(gpu_device)
    for name, m in (("stack", masks.to(gpu_device)), ("labels", mk.LabelMasks(labels.to(gpu_device), 3))):
        errs = []
        for _ in range(2):
            mean, var, cnt = mk.mask_feature_mean(fg, m, return_var=True)
            errs.append(rel(var))
            near(mean, mean_ref)
            assert torch.equal(cnt.cpu().double(), cnt_ref)
            assert float(var[2]) == 0.0
        print(f"variance levels={levels} {name}: oracle {var_ref[:2].tolist()} two-pass fp32 on the CPU {rel(var32).tolist()} "
              f"device, two calls {[e.tolist() for e in errs]}")
        for e in errs:
            assert float(e.max()) <= BAR


# ---- the raw second moments of the C ABI -----------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("C", [3, 6])
@pytest.mark.parametrize("HW", [257, 1025, 1028])
def test_feature_sums_with_squares(gpu_device, HW, C, weighted):
    """ogs_mask_feature_sums / ogs_label_feature_sums with with_squares = 1 (no caller in the package passes it; the one-pass
    variance of scripts/mask_bench.py --variance does): row n = sum w f[c] | sum w | sum w f[c]^2 over the pixels of mask n,
    all 2C + 1 columns against float64 on the same inputs.  257: two waves; 1025: two workgroups on the scalar path; 1028:
    two on the vector path; N = 9 disjoint masks, one past the stack walk's unroll of 8.  The bound of a row is the worst
    case of ANY order of summing its n_pix terms in fp32 -- n_pix - 1 additions and the two roundings of w * f * f:
    (n_pix + 2) * 2^-24 * sum |term|."""
    from opengaussian_amd import _lib, mask_ops as mk
    H, W = SHAPES[HW]
    N = 9
    g = torch.Generator().manual_seed(4000 + 35 * HW + C)
    feat = torch.rand(C, H, W, generator=g) * 2 - 1
    sil = torch.rand(H, W, generator=g) * 0.9 + 0.05 if weighted else None
    labels = torch.randint(0, N + 1, (H, W), generator=g, dtype=torch.int32)       # 0: in no mask
    stack = torch.stack([labels == n + 1 for n in range(N)])
    f64 = feat.double().flatten(1)                                                 # [C, HW]
    w64 = (torch.ones(HW, dtype=torch.float64) if sil is None else sil.double().flatten())
    terms = torch.cat([w64 * f64, w64[None], w64 * f64 * f64])                     # [2C+1, HW], the table's column order
    member = stack.flatten(1).double()                                             # [N, HW]
    want = member @ terms.t()                                                      # [N, 2C+1]
    bound = (member.sum(1, keepdim=True) + 2) * 2.0 ** -24 * (member @ terms.abs().t())
    fg, wg = feat.to(gpu_device), None if sil is None else sil.to(gpu_device)
    lib, ptr = _lib.lib(), _lib.ptr
    for name, m in (("ogs_mask_feature_sums", stack.to(gpu_device).view(torch.uint8)),
                    ("ogs_label_feature_sums", labels.to(gpu_device))):
        table = torch.full((N, mk.TABLE_STRIDE), float("nan"), device=gpu_device)
        _lib.check(getattr(lib, name)(ptr(fg), ptr(m), ptr(wg), C, N, HW, 1, ptr(table),
                                      torch.cuda.current_stream().cuda_stream), name)
        err = (table[:, :2 * C + 1].double().cpu() - want).abs()
        print(f"{name} HW={HW} C={C} weighted={weighted}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (name, err, bound)
