"""fp32 restatements, in numpy, of the two sides of the bounded tile rect (csrc/preprocess_fwd.hip):

  * `emit_rect`: the rect preprocess_one ("8b") leaves for duplicate_kernel -- the reference rect cut down to the bounding box of
    the reach ellipse;
  * `box_test`: duplicate_kernel's per-(Gaussian, tile) test, max_power_in_box(...) >= thr (csrc/ogs_common.h).

Every operation is one IEEE fp32 operation in the kernels' order (the file is compiled without contraction), except the logarithm:
the device's fast log and numpy's differ by ~1e-6, which the 1e-4 the bound adds to the threshold covers.  The containment the
kernels rely on -- every tile of the reference rect that passes `box_test` lies inside `emit_rect` -- is checked on the CPU over
random and adversarial Gaussians (tests/test_1b_bounded_rect_gpu.py::test_bound_contains_box_test_cpu), and on the GPU by the
binning comparisons of the same file.
"""
import numpy as np

F = np.float32
K_THR_MARGIN = F(0.01)
TILE = 16


def _tr(v):
    v = np.where(np.abs(v) < F(3.0e38), v, F(0.0)).astype(F)
    return np.clip(v, F(-2.0e9), F(2.0e9)).astype(np.int64)


def conic_radius(ca, cb, cc):
    """steps 5 and 6 of preprocess_one: fp32 conic and the reference radius of the 2D covariance (ca, cb, cc)"""
    ca, cb, cc = (np.asarray(v, F) for v in (ca, cb, cc))
    det = ca * cc - cb * cb
    with np.errstate(all="ignore"):
        det_inv = F(1.0) / det
        A, B, Cc = cc * det_inv, -cb * det_inv, ca * det_inv
        mid = F(0.5) * (ca + cc)
        sq = np.sqrt(np.maximum(F(0.1), mid * mid - det))
        lam = np.maximum(mid + sq, mid - sq)
        rad = np.ceil(F(3.0) * np.sqrt(lam))
    rad = np.where(np.abs(rad) < F(3.0e38), rad, F(0.0)).astype(F)
    return A, B, Cc, rad, det != 0


def reference_rect(px, py, rad, gx, gy):
    k = F(TILE)
    x0 = np.minimum(gx, np.maximum(0, _tr((px - rad) / k)))
    y0 = np.minimum(gy, np.maximum(0, _tr((py - rad) / k)))
    x1 = np.minimum(gx, np.maximum(0, _tr((px + rad + k - F(1.0)) / k)))
    y1 = np.minimum(gy, np.maximum(0, _tr((py + rad + k - F(1.0)) / k)))
    return x0, x1, y0, y1


def emit_rect(px, py, rad, A, B, Cc, opacity, gx, gy):
    """(x0, x1, y0, y1) of the emitted rect, max exclusive; an empty rect comes back as all zeros"""
    px, py, rad, A, B, Cc, opacity = (np.asarray(v, F) for v in (px, py, rad, A, B, Cc, opacity))
    rx0, rx1, ry0, ry1 = reference_rect(px, py, rad, gx, gy)
    with np.errstate(all="ignore"):
        Rr = rad + F(17.0)
        tmax = (F(0.5) * (A + Cc) + np.abs(B)) * (Rr * Rr)
        t = F(2.0) * ((np.log(F(255.0) * opacity).astype(F) + K_THR_MARGIN) + (F(1.0e-4) + F(1.25e-6) * tmax))
        dcf = (A.astype(np.float64) * Cc.astype(np.float64) - B.astype(np.float64) * B.astype(np.float64)).astype(F)
        pad = F(1.0e-6) * (np.maximum(np.abs(px), np.abs(py)) + Rr) + F(1.0e-3)
        hx = np.sqrt(t * (Cc / dcf)) * F(1.00001) + pad
        hy = np.sqrt(t * (A / dcf)) * F(1.00001) + pad
        k = F(TILE)
        bx0 = np.maximum(rx0, _tr(np.ceil((px - hx - F(15.0)) / k)))
        by0 = np.maximum(ry0, _tr(np.ceil((py - hy - F(15.0)) / k)))
        bx1 = np.minimum(rx1, _tr(np.floor((px + hx) / k)) + 1)
        by1 = np.minimum(ry1, _tr(np.floor((py + hy) / k)) + 1)
        ellipse = (A > 0) & (Cc > 0) & (dcf > 0) & (rx1 - rx0 <= 255)      # wider rects are flagged without a test: not cut
        bounded = ellipse & ~(t < 0) & (hx < F(3.0e38)) & (hy < F(3.0e38))
        none = (ellipse & (t < 0)) | (bounded & ((bx1 <= bx0) | (by1 <= by0)))
    pick = lambda b, r: np.where(none, 0, np.where(bounded, b, r))
    return pick(bx0, rx0), pick(bx1, rx1), pick(by0, ry0), pick(by1, ry1)


def max_power_in_box(A, B, Cc, xlo, xhi, ylo, yhi):
    with np.errstate(all="ignore"):
        nbA, nbC = -B / A, -B / Cc

        def q(dx, dy):
            return F(-0.5) * (A * dx * dx + Cc * dy * dy) - B * dx * dy

        clampy = lambda v: np.minimum(np.maximum(v, ylo), yhi)
        clampx = lambda v: np.minimum(np.maximum(v, xlo), xhi)
        m = q(xlo, clampy(nbC * xlo))
        m = np.fmax(m, q(xhi, clampy(nbC * xhi)))
        m = np.fmax(m, q(clampx(nbA * ylo), ylo))
        m = np.fmax(m, q(clampx(nbA * yhi), yhi))
        X = np.maximum(np.abs(xlo), np.abs(xhi))
        Y = np.maximum(np.abs(ylo), np.abs(yhi))
        m = m + F(8e-7) * (F(0.5) * (A * X * X + Cc * Y * Y) + np.abs(B) * X * Y)
    inside = (xlo <= 0) & (xhi >= 0) & (ylo <= 0) & (yhi >= 0)
    return np.where(inside, F(0.0), m).astype(F)


def box_test(px, py, A, B, Cc, opacity, tx, ty):
    """duplicate_kernel's reach test of tile (tx, ty), per pair"""
    with np.errstate(all="ignore"):
        thr = -(np.log(F(255.0) * opacity).astype(F) + K_THR_MARGIN)
        X0, Y0 = (tx * TILE).astype(F), (ty * TILE).astype(F)
        m = max_power_in_box(A, B, Cc, px - X0 - F(15.0), px - X0, py - Y0 - F(15.0), py - Y0)
        return m >= thr


def containment_violations(px, py, ca, cb, cc, opacity, W, H):
    """Pairs (Gaussian, tile of its reference rect) that pass box_test but lie outside emit_rect; also returns the number of
    reference pairs, of emitted pairs and of pairs that pass the test."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    px, py, opacity = (np.asarray(v, F) for v in (px, py, opacity))
    A, B, Cc, rad, ok = conic_radius(ca, cb, cc)
    rx0, rx1, ry0, ry1 = reference_rect(px, py, rad, gx, gy)
    ok &= (rad > 0) & ((rx1 - rx0) * (ry1 - ry0) != 0)
    ex0, ex1, ey0, ey1 = emit_rect(px, py, rad, A, B, Cc, opacity, gx, gy)
    some = ok & (ex1 > ex0)
    assert ((ex0 >= rx0) & (ex1 <= rx1) & (ey0 >= ry0) & (ey1 <= ry1) & (ey1 > ey0))[some].all(), \
        "an emitted rect leaves its reference rect"
    w = np.where(ok, rx1 - rx0, 0)
    cnt = w * np.where(ok, ry1 - ry0, 0)
    g = np.repeat(np.arange(px.size), cnt)
    local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ty = ry0[g] + local // w[g]
    tx = rx0[g] + local % w[g]
    reach = box_test(px[g], py[g], A[g], B[g], Cc[g], opacity[g], tx, ty)
    inside = (tx >= ex0[g]) & (tx < ex1[g]) & (ty >= ey0[g]) & (ty < ey1[g])
    emitted = int(((ex1 - ex0) * (ey1 - ey0))[ok].sum())
    return int((reach & ~inside).sum()), int(cnt.sum()), emitted, int(reach.sum())


def random_cov2d(rng, n, smin, smax, ratio_lo, ratio_hi):
    """2D covariances as preprocess_one ends up with them: R diag(s1^2, s2^2) R^T + 0.3 I, in fp32"""
    s1 = np.exp(rng.uniform(np.log(smin), np.log(smax), n))
    s2 = s1 / np.exp(rng.uniform(np.log(ratio_lo), np.log(ratio_hi), n))
    th = rng.uniform(0, np.pi, n)
    c, s = np.cos(th), np.sin(th)
    ca = (c * c * s1 * s1 + s * s * s2 * s2).astype(F) + F(0.3)
    cc = (s * s * s1 * s1 + c * c * s2 * s2).astype(F) + F(0.3)
    cb = (c * s * (s1 * s1 - s2 * s2)).astype(F)
    return ca, cb, cc
