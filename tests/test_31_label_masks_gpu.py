"""GPU: the label form of the stage-1 mask reductions (mask_ops.LabelMasks -> ogs_label_* in include/ogs_mask.h) against
the reference goldens, the dense HIP path and the CPU oracle.  Same fold and same float atomics as the dense kernels, so
test_30's tolerances: values rtol 2e-5 / atol 1e-6, gradients 1e-4 of the largest entry (the variance 2e-4, as there).
Table sums come from float atomics: nothing here asserts bit-identity on them (exact zeros excepted).

The separation loss weights every pair by the RANK of its inverse distance inside its row (argsort().argsort()), so it
is discontinuous where two inverse distances of a row meet: a swap moves a weight by 0.9 / (N - 1), far more than
1e-4 of a gradient.  With features drawn uniformly every mean sits near 0.5 and 96 of them leave gaps down to 3e-11
in a row: the float32 oracle then misses the gradient tolerance against the float64 oracle (1.2e-9 against 1.1e-9 on
135x240, N = 96, C = 3; ten ranks differ), and no float32 path can meet it.  The inputs here are therefore built by
separable(): a colour per label plus texture, colours redrawn until every row's inverse distances (of the float64
oracle's means, for the weights the test uses) lie at least GAP apart.  GAP = 2e-6: a float32 mean of values below
1.5 is good to about 1e-7, |d/dm 1/(1+d^2)| <= 0.65, two means and up to six channels move an inverse distance by at
most 3e-7, its own rounding adds 6e-8; GAP leaves five times that."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden.make_mask_golden import CASES as GOLDEN_CASES, case_inputs

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "mask_golden.npz"))
DISJOINT = [c for c in GOLDEN_CASES if not c[5]]                    # seeds 0, 1, 3


def near(a, b, rtol=2e-5):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-6)


def grad_near(got, want):
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy() if torch.is_tensor(want) else want
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()


def stack_of(labels, N):
    """the [N,H,W] bool stack a label image stands for: row n where labels == n + 1, everything else in no row"""
    ids = torch.arange(1, N + 1, device=labels.device)
    return labels[None] == ids[:, None, None]


GAP = 2e-6


def rank_gap(mean):
    """per row, the smallest distance between two of the inverse distances the separation loss ranks (the diagonal is
    filled with 0 there, and so here)"""
    N = mean.shape[0]
    inv = 1.0 / ((mean[:, None] - mean[None]).pow(2).sum(2) + 1)
    s = inv.masked_fill(torch.eye(N, dtype=torch.bool), 0).sort(dim=1).values
    return (s[:, 1:] - s[:, :-1]).min(dim=1).values


def separable(labels, N, C, seed, weights=(True,)):
    """feat [C,H,W] and silhouette [1,H,W] on the CPU with well-conditioned ranks (see the module's docstring): every
    row 1..N must own a pixel, pixels in no row carry texture alone.  `weights`: the means that are to be well apart,
    with the silhouette (True) and without (False)"""
    from oracle import mask_oracle as mo
    g = torch.Generator().manual_seed(seed)
    H, W = labels.shape
    sil = torch.rand(1, H, W, generator=g)
    texture = torch.randint(0, 1229, (C, H, W), generator=g) / 4096          # [0, 0.3) in steps of 2^-12, as the colours:
    draw = lambda n: torch.randint(0, 4096, (n, C), generator=g) / 4096         # texture + colour is exact in float32
    row = torch.where((labels >= 1) & (labels <= N), labels, 0)
    colour = draw(N + 1)
    colour[0] = 0
    masks = stack_of(labels, N)
    assert N >= 2 and bool(masks.flatten(1).any(1).all())

    def means(feat):
        return [mo.mask_feature_mean(feat, masks, image_mask=sil if w else None, dtype=torch.float64) for w in weights]

    def rows_too_close(means):
        return (torch.stack([rank_gap(m) for m in means]).amin(0) < GAP).nonzero().flatten()

    # mean(texture + colour) = mean(texture) + colour * mean(1); mean(1) < 1 where a count is clamped up to 1
    of_texture, of_one = means(texture), means(torch.ones_like(texture))

    def means_with(colour):
        return [t + one * colour[1:] for t, one in zip(of_texture, of_one)]

    bad = rows_too_close(means_with(colour))
    for _ in range(4000):                                 # redraw one colour at a time, keep what leaves fewer rows
        if bad.numel() == 0:
            feat = (texture + colour[row].permute(2, 0, 1)).contiguous()
            assert rows_too_close(means(feat)).numel() == 0
            return feat, sil
        trial = colour.clone()
        trial[bad[0] + 1] = draw(1)[0]
        trial_bad = rows_too_close(means_with(trial))
        if trial_bad.numel() < bad.numel():
            colour, bad = trial, trial_bad
    raise AssertionError(f"no well-separated colours for N = {N}")


def stage1(mk, feat, masks, sil, sep=None, coh=None):
    """train.py:450-456: separation + 0.1 * cohesion on the silhouette-weighted means; value and both gradients"""
    fm = feat.detach().requires_grad_(True)               # not a copy: a sliced or offset map stays what it is
    sw = None if sil is None else sil.detach().requires_grad_(True)
    mean = mk.mask_feature_mean(fm, masks, image_mask=sw)
    c = (coh or mk.cohesion_loss)(fm, masks, mean)
    loss = (sep or mk.separation_loss)(mean, 1000) + 0.1 * c
    loss.backward()
    return {"mean": mean.detach(), "cohesion": c.detach(), "loss": loss.detach(), "dfeat": fm.grad,
            "dsil": None if sw is None else sw.grad}


def same_results(got, want):
    near(got["mean"], want["mean"])
    near(got["cohesion"], want["cohesion"])
    near(got["loss"], want["loss"])
    grad_near(got["dfeat"], want["dfeat"])
    if want["dsil"] is not None:
        grad_near(got["dsil"], want["dsil"])


# ---- the reference's goldens -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DISJOINT, ids=lambda c: f"s{c[0]}")
def test_label_path_matches_reference_goldens(gpu_device, case):
    """seed 1 is 31x29: H*W % 4 != 0, the scalar load path"""
    from opengaussian_amd import mask_ops as mk
    seed, C, H, W, N, _ = case
    feat, masks, sil, _ = case_inputs(*case)
    assert int(masks.sum(0).max()) <= 1                                 # disjoint
    labels = (masks.long() * torch.arange(1, N + 1)[:, None, None]).sum(0)     # row index + 1 where a row is set
    feat, sil = feat.to(gpu_device), sil.to(gpu_device)
    lm = mk.LabelMasks(labels.to(gpu_device), N)
    k = f"s{seed}"
    near(mk.mask_feature_mean(feat, lm, image_mask=sil), GOLD[k + "_mean_w"])
    near(mk.mask_feature_mean(feat, lm), GOLD[k + "_mean"])
    mean, var, cnt = mk.mask_feature_mean(feat, lm, return_var=True)
    near(mean, GOLD[k + "_mean"]); near(var, GOLD[k + "_var"], 2e-4)
    np.testing.assert_array_equal(cnt.cpu().numpy(), GOLD[k + "_cnt"])
    mean_w = torch.from_numpy(GOLD[k + "_mean_w"]).to(gpu_device)
    np.testing.assert_allclose(float(mk.cohesion_loss(feat, lm, mean_w)), float(GOLD[k + "_cohesion"]), rtol=2e-5)
    r = stage1(mk, feat, lm, sil)
    grad_near(r["dfeat"], GOLD[k + "_dfeat"])
    grad_near(r["dsil"], GOLD[k + "_dsil"])
    np.testing.assert_allclose(float(r["loss"]), float(GOLD[k + "_separation"]) + 0.1 * float(GOLD[k + "_cohesion"]),
                               rtol=2e-5)
    with pytest.raises(RuntimeError, match="not differentiable"):
        mk.mask_feature_mean(feat.clone().requires_grad_(True), lm, return_var=True)[0].sum().backward()


# ---- label path == dense HIP path == oracle --------------------------------------------------------------------------
def _present(labels, N, g):
    """make every label 1..N own at least one pixel (no accidental empty rows: their tied zero means are a case of
    their own)"""
    flat = labels.flatten()
    flat[torch.randperm(flat.numel(), generator=g)[:N]] = torch.arange(1, N + 1)
    return flat.view_as(labels)


def _random(H, W, N):
    g = torch.Generator().manual_seed(H * 1000 + W)
    return _present(torch.randint(0, N + 1, (H, W), generator=g), N, g), N


def _halves():
    labels = torch.ones(64, 80, dtype=torch.long)
    labels[:, 40:] = 2
    return labels, 2


def _blocks():
    g = torch.Generator().manual_seed(96)
    ids = torch.cat([torch.randperm(96, generator=g) + 1, torch.randint(0, 97, (39,), generator=g)])    # 9 x 15 blocks
    return ids.view(9, 15).repeat_interleave(15, 0).repeat_interleave(16, 1), 96


def _salt_and_pepper():
    g = torch.Generator().manual_seed(300)
    flat = torch.randint(0, 301, (40 * 52,), generator=g)
    flat[:256] = torch.randperm(256, generator=g) + 1                  # the first wave's strip: 256 distinct labels
    flat[256:300] = torch.arange(257, 301)
    return flat.view(40, 52), 300


SHAPES = {
    "hw60": lambda: _random(6, 10, 4),                                  # less than one wave
    "16x64": lambda: _random(16, 64, 5),                                # exactly one workgroup
    "16x65": lambda: _random(16, 65, 5),                                # + a remainder; H*W % 4 != 0: scalar path
    "halves": _halves,                                                  # every workgroup's atomics on the same two rows
    "blocks96": _blocks,                                                # 135 x 240, N = 96 in blocks of 15 x 16
    "salt300": _salt_and_pepper,                                        # 40 x 52, up to 256 distinct labels per strip
}


@pytest.mark.parametrize("C", [3, 6])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_label_path_equals_dense_path_and_oracle(gpu_device, shape, C):
    from opengaussian_amd import mask_ops as mk
    from oracle import mask_oracle as mo
    labels, N = SHAPES[shape]()
    H, W = labels.shape
    feat, sil = separable(labels, N, C, 11 + C)
    masks = stack_of(labels, N)
    want = stage1(mo, feat, masks, sil, sep=mk._separation_loss_torch)               # CPU oracle, autograd
    dense = stage1(mk, feat.to(gpu_device), masks.to(gpu_device), sil.to(gpu_device))
    lm = mk.LabelMasks(labels.to(gpu_device), N)
    got = stage1(mk, feat.to(gpu_device), lm, sil.to(gpu_device))
    same_results(got, dense)
    same_results(got, want)
    if shape == "salt300":
        m_ref, v_ref, c_ref = mo.mask_feature_mean(feat, masks, return_var=True)
        mean, var, cnt = mk.mask_feature_mean(feat.to(gpu_device), lm, return_var=True)
        near(mean, m_ref); near(var, v_ref, 2e-4)
        np.testing.assert_array_equal(cnt.cpu().numpy(), c_ref.numpy())


def test_all_pixels_invalid(gpu_device):
    from opengaussian_amd import mask_ops as mk
    H, W, N = 20, 28, 3
    g = torch.Generator().manual_seed(5)
    feat, sil = torch.rand(6, H, W, generator=g).to(gpu_device), torch.rand(1, H, W, generator=g).to(gpu_device)
    labels = torch.zeros(H, W, dtype=torch.long, device=gpu_device)
    got = stage1(mk, feat, mk.LabelMasks(labels, N), sil)
    dense = stage1(mk, feat, stack_of(labels, N), sil)
    assert got["mean"].shape == (N, 6) and float(got["mean"].abs().max()) == 0.0
    assert float(got["dfeat"].abs().max()) == 0.0 and float(got["dsil"].abs().max()) == 0.0
    assert float(got["cohesion"]) == float(dense["cohesion"]) == 0.0
    _, var, cnt = mk.mask_feature_mean(feat, mk.LabelMasks(labels, N), return_var=True)
    assert float(var.abs().max()) == 0.0 and cnt.tolist() == [1.0] * N          # counts clamp at 1


def test_no_masks(gpu_device):
    from opengaussian_amd import mask_ops as mk
    H, W = 20, 28
    feat = torch.rand(6, H, W, device=gpu_device)
    labels = torch.randint(0, 5, (H, W), device=gpu_device)             # every label is above N = 0
    for masks in (mk.LabelMasks(labels, 0), torch.zeros(0, H, W, dtype=torch.bool, device=gpu_device)):
        fm = feat.clone().requires_grad_(True)
        mean = mk.mask_feature_mean(fm, masks)
        assert mean.shape == (0, 6)
        loss = mk.cohesion_loss(fm, masks, mean) + mean.sum()
        loss.backward()
        assert float(loss) == 0.0 and fm.grad.shape == feat.shape and float(fm.grad.abs().max()) == 0.0


# ---- labels outside 1..N -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 6])
def test_out_of_range_labels_lie_in_no_mask(gpu_device, C):
    from opengaussian_amd import mask_ops as mk
    H, W, N = 24, 36, 5
    g = torch.Generator().manual_seed(77)
    labels, _ = _random(H, W, N)
    bad = torch.tensor([-1, -7, N + 1, 2 ** 30])
    where = torch.rand(H, W, generator=g) < 0.3
    labels = torch.where(where, bad[torch.randint(0, 4, (H, W), generator=g)], labels)
    labels = _present(labels, N, g)
    for b in bad.tolist():
        assert int((labels == b).sum()) > 0
    feat, sil = (t.to(gpu_device) for t in separable(labels, N, C, 77))
    dense = stage1(mk, feat, stack_of(labels, N).to(gpu_device), sil)   # the stack has those pixels in no row
    got = stage1(mk, feat, mk.LabelMasks(labels.to(gpu_device), N), sil)
    same_results(got, dense)
    outside = ((labels < 1) | (labels > N)).to(gpu_device)
    assert float(got["dfeat"][:, outside].abs().max()) == 0.0 and float(got["dsil"][0][outside].abs().max()) == 0.0


@pytest.mark.parametrize("bad", [(-1, -7, 6), (-1, -7, 6, 2 ** 30)], ids=["next_row", "far"])
def test_out_of_range_labels_never_address_the_tables(gpu_device, bad):
    """the C ABI with every table followed directly by a guard: label N + 1 would be the guard's first row.  The row
    inputs (mean, gl) carry a spare row, so that nothing here can read outside its buffers either."""
    from opengaussian_amd import _lib, mask_ops as mk
    from opengaussian_amd._lib import check, ptr
    lib = _lib.lib()
    C, H, W, N, S = 6, 24, 36, 5, mk.TABLE_STRIDE
    HW = H * W
    g = torch.Generator().manual_seed(78)
    labels, _ = _random(H, W, N)
    where = torch.rand(H, W, generator=g) < 0.3
    labels = _present(torch.where(where, torch.tensor(bad)[torch.randint(0, len(bad), (H, W), generator=g)], labels), N, g)
    lab = labels.to(torch.int32).to(gpu_device)
    masks = stack_of(labels, N).to(torch.uint8).to(gpu_device).contiguous()
    feat, sil = torch.rand(C, H, W, generator=g).to(gpu_device), torch.rand(H, W, generator=g).to(gpu_device)
    mean = torch.rand(N + 1, C, generator=g).to(gpu_device)
    gl = torch.rand(N + 1, generator=g).to(gpu_device)
    stream = torch.cuda.current_stream().cuda_stream
    GUARD = -12345.0

    def guarded():
        buf = torch.full(((N + 8) * S,), GUARD, device=gpu_device)
        return buf, buf[:N * S].view(N, S), buf[N * S:]

    def run(label_form):
        name = "label" if label_form else "mask"
        m = lab if label_form else masks
        out = {}
        for sq in (0, 1):
            buf, table, guard = guarded()
            check(getattr(lib, f"ogs_{name}_feature_sums")(ptr(feat), ptr(m), ptr(sil), C, N, HW, sq, ptr(buf), stream), name)
            out[f"sums{sq}"], out[f"guard_sums{sq}"] = table[:, :(2 * C + 1 if sq else C + 1)].clone(), guard.clone()
        buf, table, guard = guarded()
        check(getattr(lib, f"ogs_{name}_cohesion")(ptr(feat), ptr(m), ptr(mean), C, N, HW, ptr(buf), stream), name)
        out["cohesion"], out["guard_cohesion"] = table[:, :2].clone(), guard.clone()
        buf, table, guard = guarded()
        dfeat = torch.empty(C, H, W, device=gpu_device)
        check(getattr(lib, f"ogs_{name}_cohesion_backward")(ptr(feat), ptr(m), ptr(mean), ptr(gl), C, N, HW, ptr(dfeat),
                                                           ptr(buf), stream), name)
        out["dmean"], out["guard_dmean"], out["dfeat"] = table[:, :C].clone(), guard.clone(), dfeat
        return out

    got, want = run(True), run(False)
    for k in ("guard_sums0", "guard_sums1", "guard_cohesion", "guard_dmean"):
        assert bool((got[k] == GUARD).all()), k
    for k in ("sums0", "sums1", "cohesion"):
        near(got[k], want[k])
    grad_near(got["dmean"], want["dmean"]); grad_near(got["dfeat"], want["dfeat"])


# ---- pointers the vector path cannot take; image_mask forms ----------------------------------------------------------
def test_unaligned_label_view_and_sliced_feature_map(gpu_device):
    from opengaussian_amd import mask_ops as mk
    labels, N = _random(16, 64, 5)
    H, W = labels.shape
    feat, sil = separable(labels, N, 6, 9)
    img, sil = torch.cat([torch.rand(3, H, W), feat]).to(gpu_device), sil.to(gpu_device)
    aligned = mk.LabelMasks(labels.to(gpu_device), N)
    want = stage1(mk, img[3:9].clone(), aligned, sil)
    buf = torch.zeros(H * W + 1, dtype=torch.int32, device=gpu_device)
    buf[1:] = labels.flatten().to(gpu_device)
    view = mk.LabelMasks(buf[1:].view(H, W), N)                         # one element into a larger buffer
    assert view.labels.data_ptr() % 16 == 4 and view.labels.data_ptr() == buf.data_ptr() + 4
    same_results(stage1(mk, img[3:9].clone(), view, sil), want)
    assert img[3:9].data_ptr() != img.data_ptr()
    same_results(stage1(mk, img[3:9], aligned, sil), want)
    same_results(stage1(mk, img[3:9], view, sil), want)


def test_image_mask_forms(gpu_device):
    from opengaussian_amd import mask_ops as mk
    labels, N = _random(16, 65, 5)
    H, W = labels.shape
    feat, sil = (t.to(gpu_device) for t in separable(labels, N, 6, 10, weights=(True, False)))
    lm, masks = mk.LabelMasks(labels.to(gpu_device), N), stack_of(labels, N).to(gpu_device)
    for weight in (None, sil[0], sil):
        got, want = stage1(mk, feat, lm, weight), stage1(mk, feat, masks, weight)
        same_results(got, want)
        if weight is not None:
            assert got["dsil"].shape == weight.shape


# ---- the drop-in -----------------------------------------------------------------------------------------------------------
def test_drop_in_wiring_equals_reference_layout(gpu_device):
    """train.py:441-456 with mask_ops.get_SAM_mask_and_feat against the reference's own mask_bool layout"""
    from opengaussian_amd import mask_ops as mk
    H, W = 48, 64
    g = torch.Generator().manual_seed(4864)
    levels, start = [], 0
    for n in (4, 6, 9, 13):
        coarse = torch.randint(-1, n, (H // 8, W // 8), generator=g)
        local = coarse.repeat_interleave(8, 0).repeat_interleave(8, 1)
        local[0, :8] = n - 1
        levels.append(torch.where(local >= 0, local + start, local))
        start += n
    gt = torch.stack(levels).to(gpu_device)
    mask_id, masks, invalid = mk.get_SAM_mask_and_feat(gt, level=3)
    feat, sil = (t.to(gpu_device) for t in separable(mask_id.cpu(), 13, 6, 4865))
    assert isinstance(masks, mk.LabelMasks) and masks.labels.device == gt.device and masks.num_mask == 13
    assert mask_id.dtype == torch.int64 and torch.equal(invalid, mask_id == 0)
    onehot = F.one_hot(mask_id.long(), masks.num_mask + 1).permute(2, 0, 1)[1:]          # opengs_utlis.py:146-148,181
    assert torch.equal(masks.dense(), onehot.bool())
    same_results(stage1(mk, feat, masks, sil), stage1(mk, feat, onehot, sil))
