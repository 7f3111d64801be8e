"""GPU: the grouped label-statistics pass (rasterizer.rasterize_group_stats, ogs_raster_forward_group_stats) against the
images of rasterize_groups on the same call -- exact counts and maximum alpha, fixed-point feature sums within 1e-5 of a float64
sum over the images, the same bits on a second run, and no G*H*W-sized memory."""
import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

W, H, F = 75, 53, 60.0                 # neither a multiple of 16
THRESHOLDS = (0.0, 0.8, 0.9, 0.999)
LABEL_COUNTS = (0, 1, 57)


def _scene(P, G, Cn, seed, dev):
    sc, cam = helpers.tiny_scene(P, W, H, F, seed=seed, log_scale_mean=-2.5)
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(-1, G + 3, (P,), generator=g, dtype=torch.int32)         # -1 and ids >= G render nothing
    feat = torch.rand(P, Cn, generator=g) * 2.0 - 0.5
    t = lambda x: x.to(dev).contiguous()
    return dict(means3D=t(sc.means3D), opacities=t(sc.opacities), scales=t(sc.scales), rotations=t(sc.rotations),
                ids=t(ids), feat=t(feat)), cam


def _labels(L, seed, dev):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(-1, max(L, 1), (H, W), generator=g, dtype=torch.int32).to(dev)


def _images(s, G, rs):
    from opengaussian_amd.rasterizer import GaussianRasterizer, rasterize_groups
    P = s["means3D"].shape[0]
    m2 = torch.zeros(P, 3, device=s["means3D"].device)
    if G == 1:
        m = s["ids"] == 0
        color, radii_sub, _, alpha = GaussianRasterizer(rs)(
            means3D=s["means3D"][m], means2D=m2[m], opacities=s["opacities"][m], colors_precomp=s["feat"][m],
            scales=s["scales"][m], rotations=s["rotations"][m])
        radii = torch.zeros(P, dtype=torch.int32, device=m.device)
        radii[m] = radii_sub
        return color[None], alpha[None], radii
    color, radii, _, alpha = rasterize_groups(s["means3D"], m2, s["opacities"], s["ids"], G, rs, colors_precomp=s["feat"],
                                              scales=s["scales"], rotations=s["rotations"])
    return color, alpha, radii


def _expected(color, alpha, labels, L, thr):
    """count / feat_sum (float64) / max_alpha straight from the images"""
    G, Cn = color.shape[:2]
    a = alpha[:, 0].double().cpu().numpy()
    col = color.double().cpu().numpy()
    lab = labels.cpu().numpy()
    bucket = np.where((lab >= 0) & (lab < L), lab, L)
    count = np.zeros((G, L + 1), np.int64)
    fsum = np.zeros((G, L + 1, Cn), np.float64)
    for g in range(G):
        sel = a[g] > thr
        b = bucket[sel]
        count[g] = np.bincount(b, minlength=L + 1)
        for c in range(Cn):
            fsum[g, :, c] = np.bincount(b, weights=col[g, c][sel], minlength=L + 1)
    return count, fsum, alpha.amax(dim=(1, 2, 3)).cpu()


def _stats(s, G, labels, L, rs, thr):
    from opengaussian_amd.rasterizer import rasterize_group_stats
    return rasterize_group_stats(s["means3D"], s["opacities"], s["ids"], G, labels, L, rs, s["feat"], scales=s["scales"],
                                 rotations=s["rotations"], alpha_threshold=thr)


@pytest.mark.parametrize("G", [1, 7, 300])
@pytest.mark.parametrize("Cn", [3, 6])
def test_group_stats_match_grouped_images(gpu_device, G, Cn):
    dev = gpu_device
    s, cam = _scene(3000, G, Cn, seed=G + Cn, dev=dev)
    rs = helpers.settings_for(cam, (0.25, -0.5, 0.75), 3, dev)            # a non-zero background, tiled over C
    with torch.no_grad():
        color, alpha, radii_img = _images(s, G, rs)
        assert float(alpha.max()) > 0.9, "the scene must reach the high thresholds"
        for L in LABEL_COUNTS:
            labels = _labels(L, G + L, dev)
            for thr in THRESHOLDS:
                max_alpha, count, fsum, radii = _stats(s, G, labels, L, rs, thr)
                want_count, want_fsum, want_max = _expected(color, alpha, labels, L, thr)
                what = f"G={G} C={Cn} L={L} thr={thr}"
                assert count.dtype == torch.int64 and tuple(count.shape) == (G, L + 1), what
                assert tuple(fsum.shape) == (G, L + 1, Cn) and fsum.dtype == torch.float32, what
                assert np.array_equal(count.cpu().numpy(), want_count), what
                assert torch.equal(max_alpha.cpu().view(torch.int32), want_max.view(torch.int32)), what
                got = fsum.double().cpu().numpy()
                err = np.abs(got - want_fsum) - 1e-5 * np.abs(want_fsum)
                assert err.max() <= 1e-6, f"{what}: feat_sum off by {err.max()}"
                assert torch.equal(radii, radii_img), what
                again = _stats(s, G, labels, L, rs, thr)
                for x, y in zip((max_alpha, count, fsum, radii), again):
                    assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                       y.view(torch.int32) if y.dtype == torch.float32 else y), f"{what}: run to run"


def test_group_stats_empty_cases(gpu_device):
    """D = 0 (no Gaussian in any group), P = 0, G = 0: zeros, no error; a negative threshold counts the background"""
    from opengaussian_amd.rasterizer import rasterize_group_stats
    dev = gpu_device
    s, cam = _scene(500, 7, 6, seed=3, dev=dev)
    rs = helpers.settings_for(cam, (0.1, 0.2, 0.3), 3, dev)
    labels = _labels(5, 3, dev)
    with torch.no_grad():
        none = torch.full_like(s["ids"], -1)
        ma, cnt, fs, radii = rasterize_group_stats(s["means3D"], s["opacities"], none, 7, labels, 5, rs, s["feat"],
                                                   scales=s["scales"], rotations=s["rotations"], alpha_threshold=0.5)
        assert not ma.any() and not cnt.any() and not fs.any() and not radii.any()
        # every pixel at alpha 0 with the background colour: thr < 0 counts them all
        ma, cnt, fs, _ = rasterize_group_stats(s["means3D"], s["opacities"], none, 7, labels, 5, rs, s["feat"],
                                               scales=s["scales"], rotations=s["rotations"], alpha_threshold=-1.0)
        lab = labels.flatten().long().cpu()
        want = torch.bincount(torch.where((lab >= 0) & (lab < 5), lab, torch.full_like(lab, 5)), minlength=6)
        assert torch.equal(cnt.cpu(), want[None].expand(7, 6))
        bg6 = torch.tensor([0.1, 0.2, 0.3] * 2, dtype=torch.float64)
        assert torch.allclose(fs.double().cpu(), want[None, :, None].double() * bg6, rtol=1e-6, atol=1e-6)
        e = lambda t: t[:0].contiguous()
        ma, cnt, fs, radii = rasterize_group_stats(e(s["means3D"]), e(s["opacities"]), e(s["ids"]), 3, labels, 5, rs,
                                                   e(s["feat"]), scales=e(s["scales"]), rotations=e(s["rotations"]))
        assert not ma.any() and not cnt.any() and not fs.any() and radii.numel() == 0
        ma, cnt, fs, _ = rasterize_group_stats(s["means3D"], s["opacities"], s["ids"], 0, labels, 5, rs, s["feat"],
                                               scales=s["scales"], rotations=s["rotations"])
        assert ma.numel() == 0 and tuple(cnt.shape) == (0, 6)


def test_group_stats_rejects_bad_arguments(gpu_device):
    from opengaussian_amd import _lib
    from opengaussian_amd.rasterizer import rasterize_group_stats
    dev = gpu_device
    s, cam = _scene(200, 3, 3, seed=5, dev=dev)
    rs = helpers.settings_for(cam, (0.0, 0.0, 0.0), 3, dev)
    lib = _lib.lib()
    st = _lib.OgsGroupStatsArgs()
    st.num_labels = -1
    assert lib.ogs_raster_forward_group_stats(_lib.OgsRasterFwdArgs(), st, 0, None) == -1
    st.num_labels = 4                   # labels == NULL
    assert lib.ogs_raster_forward_group_stats(_lib.OgsRasterFwdArgs(), st, 0, None) == -1
    feat = s["feat"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="no backward"):
        rasterize_group_stats(s["means3D"], s["opacities"], s["ids"], 3, _labels(4, 0, dev), 4, rs, feat,
                              scales=s["scales"], rotations=s["rotations"])


def test_group_stats_memory_at_640_groups(gpu_device):
    """640 leaves of a 648 x 484 view, P = 200 k: the pass stays far below one [G, H, W] fp32 image stack"""
    from opengaussian_amd.rasterizer import rasterize_group_stats
    from opengaussian_amd.synthetic import make_camera, make_scene
    dev = gpu_device
    Wb, Hb, G, L = 648, 484, 640, 120
    sc = make_scene(200_000, Wb, Hb, 500.0, 500.0, seed=7)
    cam = make_camera(Wb, Hb, 500.0, 500.0)
    rs = helpers.settings_for(cam, (0.0, 0.0, 0.0), 3, dev)
    g = torch.Generator().manual_seed(7)
    t = lambda x: x.to(dev).contiguous()
    m3, op, scl, rot = t(sc.means3D), t(sc.opacities), t(sc.scales), t(sc.rotations)
    ids = t(torch.randint(-1, G, (m3.shape[0],), generator=g, dtype=torch.int32))
    feat = t(torch.rand(m3.shape[0], 6, generator=g))
    labels = t(torch.randint(-1, L, (Hb, Wb), generator=g, dtype=torch.int32))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    with torch.no_grad():
        ma, cnt, fs, _ = rasterize_group_stats(m3, op, ids, G, labels, L, rs, feat, scales=scl, rotations=rot,
                                               alpha_threshold=0.8)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - base
    assert rise < G * Hb * Wb * 4 // 4, f"peak rise {rise / 2**20:.1f} MiB"
    assert int(cnt.sum()) > 0 and float(ma.max()) > 0.8
