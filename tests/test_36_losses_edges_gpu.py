"""GPU: the fused image losses (opengaussian_amd/losses.py over csrc/losses.hip) at the edges of their index arithmetic --
the 11-tap window and its zero padding, the 32 x 32 tile and its halo, the float4 / scalar choice of the masked pair and
its grid-stride loop -- against tests/golden/loss_edges_golden*.npz, produced by the reference's own functions in fp64
(tests/golden/make_loss_edges_golden.py), and, where no array is stored, against tests/loss_restatement.py in fp64 on the
device (tests/test_losses_edges_host.py pins the one to the other on the CPU).

Bounds, as in tests/test_33_losses_gpu.py.  Values: max(2e-5, 4 * v32) relative.  Gradients: max(1e-4, 4 * e32) of the largest
expected entry OF THE REGION COMPARED -- the whole image and each band of make_loss_edges_golden.bands (the image border,
the tile seams, the corners), so that a wrong band cannot hide behind a larger entry elsewhere.  v32 / e32 are the
deviations of the reference's own fp32 run from its fp64 run, read from the fixture, per case and per region; 1e-4 where
none is stored.  No pixel is left out of any comparison.
"""
import numpy as np
import pytest
import torch

from tests import loss_restatement as lr
from tests.golden import make_loss_edges_golden as me

pytestmark = pytest.mark.gpu
GOLD = me.load_golden()
CASE = {c: i for i, c in enumerate(me.PHOTO_CASES)}
UPSTREAM_CASES = [CASE[(33, 33, "near")], CASE[(70, 75, "delta")]]


def _num(v):
    return float(v.detach()) if torch.is_tensor(v) else float(v)


def _np64(v):
    return v.detach().double().cpu().numpy() if torch.is_tensor(v) else np.asarray(v, np.float64)


def _value_ok(got, want, v32, what):
    got, want, bound = _num(got), _num(want), max(2e-5, 4.0 * float(v32))
    if want == 0.0:
        print(f"{what}: value got {got:.9g} want 0")
        assert got == 0.0, what
        return
    print(f"{what}: value got {got:.9g} want {want:.9g} rel {abs(got - want) / abs(want):.2e} bound {bound:.2e}")
    assert abs(got - want) <= bound * abs(want), what


def _grad_ok(got, want, e32, what, where=None):
    """largest deviation over the largest expected entry, both over `where` (bool [H, W]) when given"""
    got, want, bound = _np64(got), _np64(want), max(1e-4, 4.0 * float(e32))
    assert got.shape == want.shape and np.isfinite(got).all(), what
    if where is not None:
        got, want = got[..., where], want[..., where]
    top = float(np.abs(want).max())
    if top == 0.0:
        print(f"{what}: grad expected all 0, largest got {np.abs(got).max():.2e}")
        assert float(np.abs(got).max()) == 0.0, what
        return
    err = float(np.abs(got - want).max()) / top
    print(f"{what}: grad err {err:.2e} of max {top:.3e}, bound {bound:.2e}")
    assert err <= bound, what


def _regions_ok(got, want, index, which, what):
    """the whole image and every non-empty band, each with its own stored e32 and its own ruler"""
    H, W, _ = me.PHOTO_CASES[index]
    assert tuple(got.shape) == (3, H, W)
    _grad_ok(got, want, GOLD[f"p{index}_e32_{which}"], f"{what} whole")
    for band, where in me.bands(H, W).items():
        if where.any():
            _grad_ok(got, want, GOLD[f"p{index}_e32_{which}_{band}"], f"{what} {band}", where)


# ---- photometric -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(me.PHOTO_CASES)), ids=me.PHOTO_IDS)
def test_photometric_values_and_gradients_on_image_and_bands(gpu_device, index):
    """lambda = 0.2, lambda = 1 and ssim() alone, every case, whole image and bands"""
    from opengaussian_amd import losses
    img_c, gt_c = me.photo_inputs(index)
    img, gt = img_c.to(gpu_device), gt_c.to(gpu_device)
    k, pid = f"p{index}_", me.PHOTO_IDS[index]
    want_l1, want_ssim, grad_ssim = float(GOLD[k + "l1"]), float(GOLD[k + "ssim"]), GOLD[k + "grad_ssim"]
    sign_over_n = me.l1_gradient(img_c, gt_c)
    for lam, tag, which in ((0.2, "loss02", "loss02"), (1.0, "loss10", "ssim")):
        x = img.clone().requires_grad_(True)
        loss, l1 = losses.photometric_loss(x, gt, lam)
        loss.backward()
        _value_ok(loss, (1.0 - lam) * want_l1 + lam * (1.0 - want_ssim), GOLD[k + "v32_" + tag], f"photo {pid} {tag}")
        _value_ok(l1, want_l1, GOLD[k + "v32_l1"], f"photo {pid} Ll1")
        _regions_ok(x.grad, (1.0 - lam) * sign_over_n - lam * grad_ssim, index, which, f"photo {pid} {tag}")
    x = img.clone().requires_grad_(True)
    ss = losses.ssim(x, gt)
    ss.backward()
    _value_ok(ss, want_ssim, GOLD[k + "v32_ssim"], f"photo {pid} ssim")
    _value_ok(losses.l1_loss(img, gt), want_l1, GOLD[k + "v32_l1"], f"photo {pid} l1_loss")
    _regions_ok(x.grad, grad_ssim, index, "ssim", f"photo {pid} ssim")


@pytest.mark.parametrize("lam,u,v", me.UPSTREAM, ids=["lam%g-u%g-v%g" % r for r in me.UPSTREAM])
@pytest.mark.parametrize("index", UPSTREAM_CASES, ids=[me.PHOTO_IDS[i] for i in UPSTREAM_CASES])
def test_upstream_scalars_and_lambda(gpu_device, index, lam, u, v):
    """(u loss + v Ll1).backward(): d / d img = a sign / N + b grad_ssim with a = u (1 - lambda) + v, b = -u lambda"""
    from opengaussian_amd import losses
    img_c, gt_c = me.photo_inputs(index)
    img, gt = img_c.to(gpu_device), gt_c.to(gpu_device)
    H, W, kind = me.PHOTO_CASES[index]
    x = img.clone().requires_grad_(True)
    loss, l1 = losses.photometric_loss(x, gt, lam)
    if u == 0.0:
        l1.backward()                                       # `loss` unused: its upstream gradient is None
    elif v == 0.0:
        (u * loss).backward()
    else:
        (u * loss + v * l1).backward()                      # both outputs of one call
    a, b = u * (1.0 - lam) + v, -u * lam
    want = a * me.l1_gradient(img_c, gt_c) + b * GOLD[f"p{index}_grad_ssim"]
    e32 = max(float(GOLD[f"p{index}_e32_loss02"]), float(GOLD[f"p{index}_e32_ssim"]))
    what = f"upstream {me.PHOTO_IDS[index]} lam {lam} u {u} v {v}"
    _grad_ok(x.grad, want, e32, what)
    got = x.grad.cpu()
    if b == 0.0:                                            # exactly a sign / N: nothing where the images agree
        same = img_c == gt_c
        assert bool(same.any()), "the case has no entry with img == gt"
        assert float(got[same].abs().max()) == 0.0, what
    if kind == "delta":
        bound, top = max(1e-4, 4.0 * e32), float(np.abs(want).max())
        for c, y, xx in me.delta_pixels(H, W):
            assert img_c[c, y, xx] != gt_c[c, y, xx]
            assert abs(float(got[c, y, xx]) - want[c, y, xx]) <= bound * top, (what, c, y, xx)
            if lam == 1.0:                                  # a = 0: no trace of the sign term, whose size is 1 / N
                assert abs(float(got[c, y, xx]) + GOLD[f"p{index}_grad_ssim"][c, y, xx]) <= bound * top


@pytest.mark.parametrize("index", UPSTREAM_CASES, ids=[me.PHOTO_IDS[i] for i in UPSTREAM_CASES])
def test_second_backward_over_a_retained_graph_gives_the_same_bits(gpu_device, index):
    from opengaussian_amd import losses
    img, gt = (t.to(gpu_device) for t in me.photo_inputs(index))
    x = img.clone().requires_grad_(True)
    loss, l1 = losses.photometric_loss(x, gt, 0.2)
    loss.backward(retain_graph=True)
    first, x.grad = x.grad, None
    loss.backward(retain_graph=True)
    assert first is not x.grad and float(first.abs().max()) > 0 and torch.equal(first, x.grad)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_half_precision_images(gpu_device, dtype):
    """the kernels run in fp32 on the up-cast image; the gradient comes back in the image's dtype"""
    from opengaussian_amd import losses
    img, gt = (t.to(gpu_device) for t in me.photo_inputs(CASE[(33, 33, "near")]))
    xh = img.to(dtype).requires_grad_(True)
    loss_h, l1_h = losses.photometric_loss(xh, gt, 0.2)
    loss_h.backward()
    xf = xh.detach().float().requires_grad_(True)
    loss_f, l1_f = losses.photometric_loss(xf, gt, 0.2)
    loss_f.backward()
    assert loss_h.dtype == torch.float32 and torch.equal(loss_h.detach(), loss_f.detach()) and torch.equal(l1_h, l1_f)
    assert xh.grad.dtype == dtype and xh.grad.shape == xh.shape
    assert float(xf.grad.abs().max()) > 0 and torch.equal(xh.grad, xf.grad.to(dtype))


# ---- masked L1 / L2 --------------------------------------------------------------------------------------------------
LOSSES = (("l1", 1), ("l2", 2))


def _fn(mod, name):
    return getattr(mod, name + "_loss")


def _restated(name, x, t, mask, weight, scale=1.0):
    """(value, dx) of the fp64 restatement on x's device"""
    x64 = x.detach().double().requires_grad_(True)
    v = _fn(lr, name)(x64, t.double(), mask, None if weight is None else weight.double())
    (scale * v).backward()
    return v.detach(), x64.grad


def _masked_ok(name, x, t, mask, weight, what, key=None):
    """One loss on device tensors against the fixture entry `key` where it is stored, else the fp64 restatement; exactly 0
    outside the mask.  Returns (value, dx)."""
    from opengaussian_amd import losses
    xx = x if x.requires_grad else x.detach().clone().requires_grad_(True)        # a caller's own leaf keeps its storage
    v = _fn(losses, name)(xx, t, mask, weight)
    v.backward()
    dx, xx.grad = xx.grad, None
    want, want_dx = _restated(name, x, t, mask, weight)
    e32 = 0.0
    if key is not None:
        want = float(GOLD[f"{key}_{name}"])
        if f"{key}_{name}_dx" in GOLD:
            want_dx, e32 = GOLD[f"{key}_{name}_dx"], GOLD[f"{key}_{name}_e32"]
    assert v.dtype == torch.float32 and dx.shape == x.shape
    _value_ok(v, want, 0.0, what)
    _grad_ok(dx, want_dx, e32, what)
    if mask is not None:
        outside = ~mask.expand_as(x)
        if bool(outside.any()):
            assert float(dx[outside].abs().max()) == 0.0, what
    return v.detach(), dx


def _to(dev, inputs):
    return tuple(None if v is None else v.to(dev) for v in inputs)


@pytest.mark.parametrize("hw", list(me.MASKED_HW), ids=["hw%d" % n for n in me.MASKED_HW])
def test_masked_element_counts(gpu_device, hw):
    """HW around the float4, wave and workgroup sizes; C = 3 and 6; every mask / weight layout; L1 and L2"""
    seen = 0
    for index, (n, C, kind) in enumerate(me.MASKED_CASES):
        if n != hw:
            continue
        x, t, mask, weight = _to(gpu_device, me.masked_inputs(index))
        assert x.shape == (C, *me.MASKED_HW[hw]) and (mask is None) == (kind == "none")
        for name, _ in LOSSES:
            _masked_ok(name, x, t, mask, weight, f"masked {me.masked_key(index)} {name}", me.masked_key(index))
            seen += 1
    assert seen == 2 * 5 * 2


def _off_by_one(v):
    """the same values, contiguous, one element (a bool: one byte) into a larger buffer"""
    buf = torch.empty(v.numel() + 1, dtype=v.dtype, device=v.device)
    buf[1:] = v.reshape(-1)
    out = buf[1:].view(v.shape)
    assert out.is_contiguous() and out.storage_offset() == 1 and out.data_ptr() % (4 * v.element_size()) != 0
    return out


@pytest.mark.parametrize("moved", ["x", "t", "mask", "weight", "all"])
def test_masked_storage_offsets(gpu_device, moved):
    """(6, 16, 20) is float4-eligible; any one pointer off its alignment sends the call down the scalar path.  dx does not
    depend on the path (per-element formula, integer denominator); the value may differ by its summation order."""
    aligned = dict(zip(("x", "t", "mask", "weight"), _to(gpu_device, me.random_masked(6, 16, 20, "weight", 3100))))
    assert all(v.data_ptr() % 16 == 0 for v in aligned.values()) and aligned["mask"].shape == (1, 16, 20)
    args = {k: _off_by_one(v) if moved in (k, "all") else v for k, v in aligned.items()}
    args["x"] = args["x"].requires_grad_(True) if moved in ("x", "all") else args["x"]
    for name, _ in LOSSES:
        v0, dx0 = _masked_ok(name, *aligned.values(), f"offsets aligned {name}")
        v1, dx1 = _masked_ok(name, *args.values(), f"offsets {moved} moved {name}")
        assert torch.equal(dx0, dx1), (moved, name)
        ulp = float(np.spacing(np.float32(abs(float(v0)))))
        print(f"offsets {moved} {name}: value {float(v0):.9g} vs {float(v1):.9g}, ulp {ulp:.2e}")
        assert abs(float(v0) - float(v1)) <= ulp, (moved, name)


@pytest.mark.parametrize("shape", [(3, 299, 293), (6, 420, 420)], ids=["scalar-3x299x293", "float4-6x420x420"])
def test_masked_second_grid_stride_trip(gpu_device, shape):
    """A launch is capped at 1024 workgroups of 256 threads.  (3, 299, 293): HW odd, 262 821 scalar steps = 1027 workgroups
    wanted; (6, 420, 420): 264 600 float4 steps = 1034 wanted.  The first workgroups go round twice."""
    C, H, W = shape
    steps = C * H * W // 4 if (H * W) % 4 == 0 else C * H * W
    assert 1024 < -(-steps // 256) < 1040 and ((H * W) % 4 == 0) == (C == 6)
    x, t, mask, weight = _to(gpu_device, me.random_masked(C, H, W, "weight", 3200 + C))
    assert mask.shape == (1, H, W) and weight.shape == (1, H, W)
    for name, _ in LOSSES:
        _masked_ok(name, x, t, mask, weight, f"stride {shape} weight {name}")
        _masked_ok(name, x, t, mask, None, f"stride {shape} one_hw {name}")


@pytest.mark.parametrize("index", range(len(me.EXTREME_CASES)), ids=me.extreme_key)
def test_masked_extremes(gpu_device, index):
    (C, H, W), kind = me.EXTREME_CASES[index]
    x, t, mask, weight = _to(gpu_device, me.extreme_inputs(index))
    inside = mask.expand_as(x)
    for name, p in LOSSES:
        v, dx = _masked_ok(name, x, t, mask, weight, f"extreme {me.extreme_key(index)} {name}", me.extreme_key(index))
        if kind == "all_true":
            assert bool(inside.all())
        elif kind == "last_only":                           # denominator 1: dx is the plain per-element derivative
            assert int(mask.sum()) == 1 and int((dx != 0).sum()) == C
            d = (x - t)[:, H - 1, W - 1].double()
            want = torch.sign(d) if p == 1 else 2.0 * d
            assert float((dx[:, H - 1, W - 1].double() - want).abs().max()) <= 1e-6
        elif kind == "zero_weight":
            assert float(v) == 0.0 and float(dx.abs().max()) == 0.0
        elif kind == "negw":
            neg = inside & (weight.expand_as(x) < 0) & (x != t)
            assert int(neg.sum()) > 100
            d = (x - t)[neg]
            assert bool((torch.sign(dx[neg]) == (torch.sign(d) if p == 1 else -torch.sign(d))).all())
            if p == 2:
                assert float(GOLD[me.extreme_key(index) + "_l2"]) != 0.0
        else:
            same = inside & (x == t)
            assert int(same.sum()) > 0.03 * int(inside.sum())
            assert float(dx[same].abs().max()) == 0.0      # by value: L1's sign(0) is 0, L2's 2 d w is 0


def test_masked_upstream_scale_and_retained_graph(gpu_device):
    from opengaussian_amd import losses
    x, t, mask, weight = _to(gpu_device, me.random_masked(6, 33, 47, "weight", 3300))
    for name, _ in LOSSES:
        xx = x.clone().requires_grad_(True)
        v = _fn(losses, name)(xx, t, mask, weight)
        (-3.0 * v).backward(retain_graph=True)
        first, xx.grad = xx.grad, None
        _grad_ok(first, _restated(name, x, t, mask, weight, scale=-3.0)[1], 0.0, f"masked upstream -3 {name}")
        (-3.0 * v).backward(retain_graph=True)
        assert first is not xx.grad and float(first.abs().max()) > 0 and torch.equal(first, xx.grad), name
