"""Shared helpers for the parity tests: build seeded scenes, run the HIP path through the drop-in API and
the CPU oracle on identical inputs."""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from opengaussian_amd.synthetic import make_camera, make_scene


def tiny_scene(P, W, H, f, seed=0, log_scale_mean=-3.0, with_ties=False):
    sc = make_scene(P, W, H, f, f, seed=seed, log_scale_mean=log_scale_mean)
    cam = make_camera(W, H, f, f)
    if with_ties and P >= 8:
        # exact depth ties (same z) to exercise the stable tie-break by Gaussian index
        sc.means3D[1::4, 2] = sc.means3D[0::4, 2][: sc.means3D[1::4].shape[0]]
    return sc, cam


def tanfovs(W, H, fx, fy=None):
    """(tanfovx, tanfovy) of a W x H image with focal lengths fx, fy in pixels (fy=None: the same focal length)."""
    return W / (2 * fx), H / (2 * (fx if fy is None else fy))


def rotation_matrix(axis, angle):
    """Rodrigues rotation about `axis` by `angle` radians, float64 [3,3]."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def _quat_of_rotation(R):
    """unit quaternion (r, x, y, z) of a proper rotation matrix, float64 (largest-component branch: no division by ~0)."""
    R = np.asarray(R, np.float64)
    assert abs(np.linalg.det(R) - 1.0) < 1e-6 and np.abs(R @ R.T - np.eye(3)).max() < 1e-6, "not a rotation"
    q = np.array([1.0 + R[0, 0] + R[1, 1] + R[2, 2], 1.0 + R[0, 0] - R[1, 1] - R[2, 2],
                  1.0 - R[0, 0] + R[1, 1] - R[2, 2], 1.0 - R[0, 0] - R[1, 1] + R[2, 2]])
    i = int(q.argmax())
    if i == 0:
        q = np.array([q[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif i == 1:
        q = np.array([R[2, 1] - R[1, 2], q[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif i == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], q[2], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], q[3]])
    return q / np.linalg.norm(q)


def _quat_mul(a, b):
    """Hamilton product a * b of (r, x, y, z) quaternions: R(a * b) = R(a) R(b); b may be [P,4]."""
    ar, ax, ay, az = a
    br, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([ar * br - ax * bx - ay * by - az * bz, ar * bx + ax * br + ay * bz - az * by,
                     ar * by - ax * bz + ay * br + az * bx, ar * bz + ax * by - ay * bx + az * br], axis=-1)


def _poses():
    """name -> (R, t) of W2C = [R | t].  Quarter turns and the two half turns are signed permutation matrices: exact in fp32, so
    a transposed or mis-indexed rotation block is a gross error, not rounding.  "general" leaves no entry of the view and
    projection matrices at zero or one.  "down_neg_z": the camera looks down the world's -z axis (half turn about x).
    Translations are of scene size (the scenes span z = 2 .. 10 in the camera frame)."""
    q = lambda rows: np.array(rows, np.float64)
    return {
        "quarter_x": (q([[1, 0, 0], [0, 0, -1], [0, 1, 0]]), (0.7, -0.4, 1.3)),
        "quarter_y": (q([[0, 0, 1], [0, 1, 0], [-1, 0, 0]]), (-1.5, 0.8, 2.0)),
        "quarter_z": (q([[0, -1, 0], [1, 0, 0], [0, 0, 1]]), (2.2, 1.1, -0.9)),
        "roll_180": (q([[-1, 0, 0], [0, -1, 0], [0, 0, 1]]), (-0.6, 1.7, 3.1)),
        "down_neg_z": (q([[1, 0, 0], [0, -1, 0], [0, 0, -1]]), (1.2, -2.3, 0.8)),
        "general": (rotation_matrix((0.3, -0.8, 0.5), 2.1), (0.7, -0.4, 1.3)),
        "general_b": (rotation_matrix((-0.6, 0.2, 0.75), -1.3), (-3.0, 2.5, 4.0)),
    }


POSES = _poses()


def general_camera(W, H, fx, fy, R, t):
    """Camera with W2C = [R | t] (X_cam = R X_world + t) and separate focal lengths."""
    return make_camera(W, H, fx, fy, R=torch.as_tensor(np.asarray(R), dtype=torch.float32),
                       t=torch.as_tensor(np.asarray(t), dtype=torch.float32))


def scene_to_world(sc, R, t):
    """The scene `sc`, given in the frame of a camera [R | t], in world coordinates: X_w = R^T (X_c - t) and every Gaussian's
    orientation composed with R^T (Sigma_w = R^T Sigma_c R), so the posed camera sees what the identity camera saw of `sc`.
    Arithmetic in float64, rounded to fp32 once.  SH coefficients are kept (the view direction they are evaluated at moves
    with the frame, so SH colours differ from the camera-frame scene's; precomputed colours do not)."""
    from opengaussian_amd.synthetic import Scene
    R = np.asarray(R, np.float64)
    t = np.asarray(t, np.float64)
    Xw = (sc.means3D.double().numpy() - t[None, :]) @ R                       # rows: (R^T (x - t))^T = (x - t)^T R
    qw = _quat_mul(_quat_of_rotation(R.T), sc.rotations.double().numpy())
    qw = qw / np.linalg.norm(qw, axis=1, keepdims=True)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32).contiguous()
    return Scene(f32(Xw), sc.scales.clone(), f32(qw), sc.opacities.clone(), sc.shs.clone(), sc.ins_feat.clone())


def push_beyond_clamp(sc, W, H, fx, fy, share, scale=0.4, seed=0):
    """Move `share` of the centres of a CAMERA-FRAME scene to (1.35 .. 1.75) x tanfov -- past the +-1.3 x tanfov clamp of
    tx/tz, ty/tz (Appendix A.1 step 4) -- in x only, in y only and in both, both signs, and give them scale `scale` so that
    their footprints still reach the image.  Rows in front of the near plane only.  Returns the moved row indices."""
    g = torch.Generator().manual_seed(90_000 + seed)
    tanx, tany = tanfovs(W, H, fx, fy)
    front = torch.nonzero(sc.means3D[:, 2] > 0.5).reshape(-1)
    rows = front[torch.randperm(front.numel(), generator=g)[: int(round(share * sc.means3D.shape[0]))]]
    n = rows.numel()
    z = sc.means3D[rows, 2]
    far = (torch.rand(2, n, generator=g) * 0.4 + 1.35) * (torch.randint(0, 2, (2, n), generator=g) * 2.0 - 1.0)
    near = torch.rand(2, n, generator=g) * 1.8 - 0.9
    kind = torch.arange(n) % 3                                                 # 0: x beyond, 1: y beyond, 2: both
    u = torch.where(kind != 1, far[0], near[0])
    v = torch.where(kind != 0, far[1], near[1])
    sc.means3D[rows, 0] = u * z * tanx
    sc.means3D[rows, 1] = v * z * tany
    sc.scales[rows] = scale * (0.5 + torch.rand(n, 3, generator=g))
    return rows.numpy()


def posed_scene(P, W, H, fx, fy, R, t, seed=0, log_scale_mean=-3.0, beyond_clamp=0.0, clamp_scale=0.4):
    """make_scene drawn in the camera frame as tiny_scene does, moved to the world frame of the camera [R | t] (fx != fy
    allowed).  beyond_clamp: share of the centres pushed past the tx/tz, ty/tz clamp (push_beyond_clamp)."""
    sc = make_scene(P, W, H, fx, fy, seed=seed, log_scale_mean=log_scale_mean)
    if beyond_clamp:
        push_beyond_clamp(sc, W, H, fx, fy, beyond_clamp, scale=clamp_scale, seed=seed)
    return scene_to_world(sc, R, t), general_camera(W, H, fx, fy, R, t)


def oracle_inputs(sc, cam, use_sh=True, use_cov=False, feat=None):
    from oracle import raster_oracle as ro
    inp = dict(means3D=sc.means3D.numpy(), opacities=sc.opacities.numpy(),
               viewmatrix=cam.world_view_transform.numpy(), projmatrix=cam.full_proj_transform.numpy(),
               campos=cam.camera_center.numpy())
    if use_cov:
        inp["cov3D_precomp"] = ro.cov3d_from_scale_rot(sc.scales.numpy(), sc.rotations.numpy(), 1.0)
    else:
        inp["scales"] = sc.scales.numpy()
        inp["rotations"] = sc.rotations.numpy()
    if feat is not None:
        inp["colors_precomp"] = feat.numpy()
    elif use_sh:
        inp["shs"] = sc.shs.numpy()
    else:
        inp["colors_precomp"] = sc.ins_feat[:, :3].contiguous().numpy()
    return inp


def settings_for(cam, bg, sh_degree, device, debug=False, scale_modifier=1.0):
    from opengaussian_amd.rasterizer import GaussianRasterizationSettings
    import math
    return GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width,
        tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        bg=torch.as_tensor(bg, dtype=torch.float32, device=device), scale_modifier=scale_modifier,
        viewmatrix=cam.world_view_transform.to(device), projmatrix=cam.full_proj_transform.to(device),
        sh_degree=sh_degree, campos=cam.camera_center.to(device), prefiltered=False, debug=debug)


def hip_forward(inp, cam, bg, sh_degree, device, requires_grad=False, debug=False, tiny=False, scale_modifier=1.0):
    """Run GaussianRasterizer on `device` with the same arrays as the oracle.  Returns (outputs, leaves).  The field of view
    comes from `cam` (tanfovx = W / (2 fx), tanfovy = H / (2 fy) separately).
    tiny=False forces the streaming path even for P <= TINY_MAX_P (callers export its binning state)."""
    from opengaussian_amd import rasterizer as R
    from opengaussian_amd.rasterizer import GaussianRasterizer
    saved = R.TINY_MAX_P
    if not tiny:
        R.TINY_MAX_P = 0
    try:
        return _hip_forward(inp, cam, bg, sh_degree, device, requires_grad, debug, scale_modifier)
    finally:
        R.TINY_MAX_P = saved


def _hip_forward(inp, cam, bg, sh_degree, device, requires_grad, debug, scale_modifier=1.0):
    from opengaussian_amd.rasterizer import GaussianRasterizer
    t = lambda k: (None if inp.get(k) is None else
                   torch.tensor(np.asarray(inp[k]), dtype=torch.float32, device=device, requires_grad=requires_grad))
    leaves = {k: t(k) for k in ("means3D", "opacities", "scales", "rotations", "cov3D_precomp", "shs", "colors_precomp")}
    P = leaves["means3D"].shape[0]
    leaves["means2D"] = torch.zeros(P, 3, dtype=torch.float32, device=device, requires_grad=requires_grad)
    rast = GaussianRasterizer(settings_for(cam, bg, sh_degree, device, debug, scale_modifier))
    out = rast(means3D=leaves["means3D"], means2D=leaves["means2D"], opacities=leaves["opacities"],
               shs=leaves["shs"], colors_precomp=leaves["colors_precomp"], scales=leaves["scales"],
               rotations=leaves["rotations"], cov3D_precomp=leaves["cov3D_precomp"])
    return out, leaves


def _export_binning_of(a, D, point_list, W, H, dev):
    """keys / ranges / n_contrib / raw point list of one pass through ogs_raster_export_binning; the lists are cut at the last
    tile range's end (the default mode drops the unreachable pairs, so its lists are shorter than num_rendered)."""
    from opengaussian_amd import _lib
    from opengaussian_amd._lib import ptr
    gx, gy = (W + 15) // 16, (H + 15) // 16
    keys = torch.zeros(max(D, 1), dtype=torch.int64, device=dev)
    ranges = torch.zeros(gx * gy, 2, dtype=torch.int32, device=dev)
    ncontrib = torch.zeros(H, W, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().ogs_raster_export_binning(C.byref(a), D, ptr(keys), ptr(ranges), ptr(ncontrib),
                                                    torch.cuda.current_stream().cuda_stream), "export_binning")
    torch.cuda.synchronize()
    ranges = ranges.cpu().numpy().view(np.uint32)
    n = int(ranges[:, 1].max()) if ranges.size else 0
    return (keys[:n].cpu().numpy().view(np.uint64), ranges, ncontrib.cpu().numpy().view(np.uint32),
            point_list[:n].cpu().numpy().view(np.uint32))


def hip_export_binning(color_tensor):
    """Sorted keys / ranges / n_contrib / point list of the pass that produced `color_tensor`, in the REFERENCE's form: the full
    (Gaussian, tile) list.  The rasterizer's default mode drops the pairs that cannot reach a pixel of their tile before the tile
    sort, so for a pass issued in that mode this helper (a) exports the culled binning the pass really used, (b) re-renders the
    saved inputs with `rasterizer.full_binning()` and exports the full binning, and (c) holds the two against each other:
      * the culled (key, Gaussian) list == the full list filtered by the device's reach flag, entry by entry, same order;
      * the culled tile ranges == the ranges of that filtered list;
      * colour and alpha of the two passes are BIT-identical, and the culled pass' n_contrib maps onto the full pass' one
        (same last contributor for every pixel);
    then returns the full binning, which the callers compare with the oracle's (and whose dropped pairs they check in float64:
    assert_reach_flags_keep_every_contributor)."""
    from opengaussian_amd import _lib
    from opengaussian_amd import rasterizer as R
    from opengaussian_amd._lib import OgsRasterFwdArgs, ptr
    ctx = color_tensor.grad_fn
    (m3, shs, cols, opac, scl, rot, cov, bg, view, proj, campos, radii, alpha, geom, image,
     point_list, sorted_rec, quad_list) = ctx.saved_tensors
    rs = ctx.raster_settings
    D = ctx.num_rendered
    W, H = int(rs.image_width), int(rs.image_height)
    dev = m3.device
    a = OgsRasterFwdArgs()
    a.P, a.W, a.H, a.C = ctx.P, W, H, ctx.Cn
    a.geom_buffer, a.image_buffer, a.point_list = ptr(geom), ptr(image), ptr(point_list)
    a.sorted_rec, a.quad_list = ptr(sorted_rec), ptr(quad_list)
    keys, ranges, ncontrib, raw = _export_binning_of(a, D, point_list, W, H, dev)
    if not getattr(ctx, "full_binning", False):
        assert ctx.num_groups == 1, "helper: grouped passes are exported in full-binning mode only"
        assert bool((raw >> 31).all()), "default mode: every pair left in the list is flagged reachable"
        e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
        scratch = (e(ctx.Cn, H, W), e(1, H, W), e(1, H, W), torch.empty(ctx.P, dtype=torch.int32, device=dev))
        with R.full_binning():
            a2 = R._fwd_args(rs, ctx.P, ctx.Cn, m3, shs, cols, opac, scl, rot, cov, bg, view, proj, campos, *scratch, None, 1)
            geom2, image2, pl2, sr2, ql2, D2 = R._streaming_render(a2, dev, _lib.lib(), False)
        assert D2 == D
        fkeys, franges, fncontrib, fraw = _export_binning_of(a2, D2, pl2, W, H, dev)
        assert len(fkeys) == D
        fl = (fraw >> 31).astype(bool)
        # (i) the culled list is the full list minus the unflagged pairs, in the same order
        np.testing.assert_array_equal(keys, fkeys[fl], err_msg="culled keys != full keys filtered by the reach flag")
        np.testing.assert_array_equal(raw & np.uint32(0x7FFFFFFF), (fraw & np.uint32(0x7FFFFFFF))[fl])
        kept_before = np.concatenate([[0], np.cumsum(fl)]).astype(np.uint32)          # kept entries before full position i
        want = np.stack([kept_before[franges[:, 0]], kept_before[franges[:, 1]]], axis=1)
        want[want[:, 0] == want[:, 1]] = 0                 # a tile that kept nothing has the empty range (0, 0), as an untouched tile
        np.testing.assert_array_equal(ranges, want, err_msg="culled tile ranges != ranges of the filtered list")
        # (iii) same images bit for bit, same last contributor per pixel
        assert torch.equal(scratch[0], color_tensor.detach()), "colour differs between the culled and the full pass"
        assert torch.equal(scratch[2], alpha), "alpha differs between the culled and the full pass"
        assert torch.equal(scratch[3], radii)
        gx = (W + 15) // 16
        tile_of_px = ((np.arange(H)[:, None] // 16) * gx + (np.arange(W)[None, :] // 16)).astype(np.int64)
        full_pos_of_kept = np.nonzero(fl)[0].astype(np.int64)
        nz = ncontrib > 0
        g_culled = ranges[tile_of_px, 0].astype(np.int64) + ncontrib.astype(np.int64) - 1
        mapped = np.zeros_like(fncontrib)
        mapped[nz] = (full_pos_of_kept[g_culled[nz]] - franges[tile_of_px, 0].astype(np.int64)[nz] + 1).astype(np.uint32)
        np.testing.assert_array_equal(mapped, fncontrib, err_msg="n_contrib of the culled pass does not map onto the full pass'")
        keys, ranges, ncontrib, raw = fkeys, franges, fncontrib, fraw
    # sorted values: Gaussian id in bits 0..30, bit 31 = "the pair can reach a pixel of its tile" (csrc/ogs_common.h)
    LAST_REACH_FLAGS[:] = [(raw >> 31).astype(bool)]
    return keys, ranges, ncontrib, raw & np.uint32(0x7FFFFFFF)


LAST_REACH_FLAGS = [None]       # reach flags of the most recent hip_export_binning call, parallel to its point list


def assert_reach_flags_keep_every_contributor(flags, keys, point_list, geom, W, H):
    """A pair flagged "cannot reach its tile" is dropped by pack: it must not be able to contribute.  Float64 check of
    every dropped (Gaussian, tile) pair: alpha = opacity * exp(power) stays below 1/255 on all 256 pixel centres."""
    dropped = np.nonzero(~flags)[0]
    if dropped.size == 0:
        return 0
    gx = (W + 15) // 16
    tile = (keys[dropped] >> np.uint64(32)).astype(np.int64)
    gid = point_list[dropped].astype(np.int64)
    x0 = (tile % gx) * 16.0
    y0 = (tile // gx) * 16.0
    px = x0[:, None, None] + np.arange(16, dtype=np.float64)[None, None, :]
    py = y0[:, None, None] + np.arange(16, dtype=np.float64)[None, :, None]
    dx = geom.xy[gid, 0].astype(np.float64)[:, None, None] - px
    dy = geom.xy[gid, 1].astype(np.float64)[:, None, None] - py
    A, B, Cc = (geom.conic[gid, k].astype(np.float64)[:, None, None] for k in range(3))
    power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
    alpha = geom.opacity[gid].astype(np.float64)[:, None, None] * np.exp(np.minimum(power, 0.0))
    alpha = np.where(power > 0, 0.0, alpha)
    worst = float(alpha.max())
    assert worst < 1.0 / 255.0, f"a dropped pair reaches alpha {worst} >= 1/255"
    return int(dropped.size)


def assert_close_modulo_threshold_flips(got, want, tol=1e-4, flip_tol=4e-3, max_pixels=2):
    """Image comparison at `tol`, allowing a bounded number of PIXELS to differ by one blending contribution.

    The reference skips a contribution when alpha < 1/255 and stops at T < 1e-4.  The
    device exp and the host exp differ in the last ulp, so for a pixel whose alpha lands within 1 ulp of 1/255 one
    contribution of size <= alpha * T * c ~ 4e-3 appears or disappears (scripts/diag_flip.py prints the offending
    alpha * 255 = 0.99999994 for the case that motivated this helper).  At most max(max_pixels, 1e-5 * pixels)
    pixels may do that, and none may be off by more than flip_tol."""
    got, want = np.asarray(got), np.asarray(want)
    diff = np.abs(got - want).reshape(-1, got.shape[-2], got.shape[-1]).max(0)
    assert diff.max() < flip_tol, f"max difference {diff.max()}"
    nbad = int((diff > tol).sum())
    assert nbad <= max(max_pixels, 1e-5 * diff.size), f"{nbad} pixels off by more than {tol} (max {diff.max()})"


NUDGES = (2e-5, -2e-5, 1e-4, -1e-4)      # relative opacity steps of the constructive flip attribution (see below)


def nudged_opacities(inp, rows, rel):
    """copy of the oracle inputs `inp` with the opacities of `rows` scaled by 1 + rel (fp32)"""
    out = dict(inp)
    op = np.array(inp["opacities"], dtype=np.float32, copy=True)
    flat = op.reshape(-1)
    flat[rows] = flat[rows] * np.float32(1.0 + rel)
    out["opacities"] = op
    return out


def lazy(fn):
    """memoised thunk"""
    box = []

    def get():
        if not box:
            box.append(fn())
        return box[0]
    return get


def assert_grads_close_modulo_threshold_flips(got, want, tol, want_fp32=None, flip_tol=1e-3, max_rows=2, what="",
                                              want_nudged=None):
    """Gradient comparison against the float64 oracle at `tol` (relative to the family's largest entry), with every
    Gaussian (row) that misses it ATTRIBUTED to an fp32 decision flip.

    The float64 oracle re-takes the blend's skip decisions (alpha >= 1/255, stop at T < 1e-4, Appendix A.3/A.4) in
    float64; any fp32 evaluation of the algorithm -- the device's, the reference's -- takes them in fp32.  For a
    (pixel, Gaussian) pair within rounding of a threshold the two blend different sets and every gradient of that
    Gaussian moves by one pixel's contribution (up to ~1e-2 of the family maximum for dL/dopacity).  `want_fp32`
    (a callable returning the oracle's OWN graph evaluated in fp32 autograd, oracle.render_backward_f64(dtype=float32))
    identifies exactly those rows: a row may miss `tol` against float64 only if the fp32 oracle misses it too, and
    then it must agree with the fp32 oracle to `flip_tol`.  At most max(max_rows, 1e-3 * rows) such rows.

    `want_nudged` (optional; callable (rows, rel) -> the float64 oracle's gradient of this family with the opacities of `rows`
    scaled by 1 + rel): a second, constructive attribution for the flips that the fp32 oracle does NOT share.  Two fp32
    evaluations of alpha = opacity * exp(power) differ by a few 1e-6 relative (contracted or separate multiply-adds in
    `power`, the last ulp of exp), up to ~1e-4 once their conics come from differently ordered fp32 arithmetic, so the
    device can take a decision the torch fp32 graph does not.  Scaling the Gaussian's opacity by 1 +- NUDGES moves its alphas
    across the threshold they are within that margin of -- and changes its gradient by that relative amount, nothing else.
    A row that misses `tol` unexplained by the fp32 oracle must then agree with one of the nudged float64 gradients TO `tol`:
    it is held as tightly as every other row, against the oracle that takes the device's decision.
    Returns the largest relative error among the rows held to `tol`."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() + 1e-30
    rows = lambda d: (np.abs(d) / scale).reshape(want.shape[0], -1).max(axis=1)
    err = rows(got - want)
    bad = err > tol
    if bad.any():
        assert want_fp32 is not None, f"{what}: rows {np.nonzero(bad)[0][:5]} off by up to {err.max():.2e}"
        w32 = np.asarray(want_fp32(), np.float64).reshape(want.shape)
        flipped = rows(w32 - want) > 0.5 * tol                      # the fp32 oracle itself leaves the float64 one here
        unexplained = bad & ~flipped
        nudged = np.zeros_like(bad)
        if unexplained.any() and want_nudged is not None and int(unexplained.sum()) <= max(max_rows, int(2e-3 * len(err))):
            for rel in NUDGES:
                idx = np.nonzero(unexplained)[0]
                if idx.size == 0:
                    break
                wn = np.asarray(want_nudged(idx, rel), np.float64).reshape(want.shape)
                ok = idx[rows(got - wn)[idx] <= tol]
                unexplained[ok] = False
                nudged[ok] = True
        assert not unexplained.any(), (f"{what}: rows {np.nonzero(unexplained)[0][:5]} off by up to {err[unexplained].max():.2e} "
                                       f"although the fp32 oracle agrees with float64 there")
        e32 = rows(got - w32)
        assert not (bad & ~nudged).any() or e32[bad & ~nudged].max() < flip_tol, f"{what}: flipped rows differ from the fp32 oracle by {e32[bad].max():.2e}"
        assert int(bad.sum()) <= max(max_rows, int(2e-3 * len(err))), f"{what}: {int(bad.sum())} rows attributed to fp32 decision flips"
    return float(err[~bad].max()) if (~bad).any() else 0.0


GRAD_ROW_REL_TOL = 2e-2     # rows above GRAD_ROW_FLOOR of the family maximum: relative error of the row's largest entry
GRAD_ROW_FLOOR = 1e-2


def assert_grad_family_close(got, want, tol=2e-4, what="", row_rel_tol=GRAD_ROW_REL_TOL, row_floor=GRAD_ROW_FLOOR):
    """Gradient family check with two rulers (VERDICT r2 "weak" item 4): (i) max error <= tol x the family's largest entry
    (the bar the rest of the suite uses); (ii) PER ROW: every Gaussian whose gradient is above `row_floor` of the family
    maximum must agree to `row_rel_tol` of ITS OWN largest entry -- so a medium-magnitude row cannot hide an order-of-
    magnitude error under the family maximum.  (Rows below the floor are covered by (i) only: their entries are within
    fp32 summation noise of much larger cancelling terms.)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    scale = np.abs(want).max()
    if scale == 0:
        assert np.abs(got).max() == 0, f"{what}: expected an all-zero gradient, got up to {np.abs(got).max()}"
        return 0.0
    err = np.abs(got - want).max() / scale
    assert err <= tol, f"{what}: max error {err:.2e} of the family maximum (bar {tol})"
    rows_w = np.abs(want).reshape(want.shape[0], -1).max(axis=1)
    rows_e = np.abs(got - want).reshape(want.shape[0], -1).max(axis=1)
    big = rows_w >= row_floor * scale
    if big.any():
        rel = (rows_e[big] / rows_w[big]).max()
        assert rel <= row_rel_tol, f"{what}: a row above {row_floor:.0e} of the family maximum is off by {rel:.2e} of its own size"
    return float(err)


def assert_grad_family_close_modulo_threshold_flips(got, want, tol, want_fp32, what=""):
    """assert_grad_family_close (both rulers), with the rows that the fp32 oracle itself moves away from the float64 one by
    more than tol / 2 -- the attribution rule of assert_grads_close_modulo_threshold_flips, which holds those rows to the
    fp32 oracle -- left out of the comparison.  At most max(2, 2e-3 * rows) rows; the fp32 oracle is evaluated only when
    the plain check fails."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    try:
        return assert_grad_family_close(got, want, tol, what=what)
    except AssertionError:
        if want_fp32 is None or got.shape != want.shape:
            raise
    w32 = np.asarray(want_fp32(), np.float64).reshape(want.shape)
    scale = np.abs(want).max() + 1e-30
    flipped = (np.abs(w32 - want) / scale).reshape(want.shape[0], -1).max(axis=1) > 0.5 * tol
    assert int(flipped.sum()) <= max(2, int(2e-3 * len(flipped))), f"{what}: {int(flipped.sum())} rows moved by the fp32 oracle"
    got = got.copy()
    got[flipped] = want[flipped]
    return assert_grad_family_close(got, want, tol, what=what)


# ---- k-means: per-row attribution of every difference (no fraction-based tolerances) ---------------
KM_TIE = 1e-5          # ids exact except rows whose best / second-best distance gap < 1e-5
KM_CENTER_TOL = 1e-4   # north_star tolerance on centres


KM_CHUNK_ELEMS = 1 << 22   # float64 elements of one [rows, k, d] difference block (32 MiB); the row chunk follows from it


def _km_row_distances(X, C, id_sets):
    """float64 Euclidean distances of every row of X to every centre of C, evaluated in row chunks so that memory does not
    grow with N * k * d: returns (row minimum [N], first argmin [N], [distance of row r to centre ids[r]] per entry of
    id_sets).  Every row's numbers are those of the one-block evaluation (the reduction runs over a row's own k x d block).
    The chunks run on a small thread pool for wall time only (N = 600 077, k = 256, d = 15 is 2.3 G differences): each
    writes its own rows, the result does not depend on the schedule; peak memory is 8 blocks of KM_CHUNK_ELEMS + temporaries."""
    n = len(X)
    dmin, amin = np.empty(n, np.float64), np.empty(n, np.int64)
    chosen = [np.empty(n, np.float64) for _ in id_sets]
    step = max(1, KM_CHUNK_ELEMS // max(C.size, 1))

    def chunk(lo):
        hi = min(n, lo + step)
        d = np.sqrt(((X[lo:hi, None, :] - C[None, :, :]) ** 2).sum(-1))
        dmin[lo:hi], amin[lo:hi] = d.min(1), d.argmin(1)
        r = np.arange(hi - lo)
        for out, ids in zip(chosen, id_sets):
            out[lo:hi] = d[r, ids[lo:hi]]

    with ThreadPoolExecutor(max_workers=8) as ex:        # NumPy releases the GIL in these loops; chunks write disjoint rows
        list(ex.map(chunk, range(0, n, step)))
    return dmin, amin, chosen


def assert_kmeans_centers_close(got, want, k_note=""):
    """EVERY centre row within KM_CENTER_TOL of the reference's (no fraction of rows is exempt)."""
    diff = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max(axis=1)
    assert diff.max() <= KM_CENTER_TOL, f"{int((diff > KM_CENTER_TOL).sum())} centre rows differ by > {KM_CENTER_TOL} {k_note}: {diff.max()}"


def kmeans_step_attribution(feat, c_prev, c_next_ref, ids_prev_ref, ids_prev_got, c_next_got, what="", c_prev_got=None):
    """ONE Lloyd iteration, the reference's (from its centres ``c_prev``) against the one under test (from
    ``c_prev_got``; default: the same centres, so that a near-tie flip cannot cascade):

    * arithmetic: every id -- of the result under test under ITS centres, of the reference's own trajectory under
      the reference's (its cdist goes through a matmul) -- is the float64 nearest centre up to a tie: the distance to
      the chosen centre exceeds the float64 minimum by < KM_TIE;
    * attribution of ids: where the two sides chose differently, the two candidate centres are within
      2 * KM_TIE + 2 * delta of each other for that row (delta = max difference of the previous centres: it
      shifts every distance by at most delta);
    * the centres under test equal the float64 mean of THEIR OWN members to 2e-5 (pure arithmetic);
    * attribution of centres: a cluster whose membership is identical on both sides agrees with the reference's next
      centre to KM_CENTER_TOL; one that gained / lost flipped rows may move by at most the sum of those rows'
      offsets |x - c| / n on top of that.
    Returns (number of flipped rows, max difference of the next centres)."""
    X = np.asarray(feat, np.float64)
    C = np.asarray(c_prev, np.float64)
    Cg = C if c_prev_got is None else np.asarray(c_prev_got, np.float64)
    delta = float(np.abs(Cg - C).max())
    got = np.asarray(ids_prev_got, np.int64)
    ref_given = None if ids_prev_ref is None else np.asarray(ids_prev_ref, np.int64)
    # distances under the reference's centres: row minimum, first argmin, distance to each side's chosen centre
    min_ref, arg_ref, chosen_ref = _km_row_distances(X, C, [got] + ([] if ref_given is None else [ref_given]))
    if c_prev_got is None:
        min_got, got_under_got = min_ref, chosen_ref[0]
    else:
        min_got, _, (got_under_got,) = _km_row_distances(X, Cg, [got])
    for name, chosen, dmin in (("under test", got_under_got, min_got),
                               ("reference", None if ref_given is None else chosen_ref[1], min_ref)):
        if chosen is None:
            continue
        excess = chosen - dmin
        assert (excess < KM_TIE).all(), (f"{what}: {name} ids are not the f64 nearest centre on rows that are NOT near ties: "
                                         f"rows {np.nonzero(excess >= KM_TIE)[0][:5]} excess {excess.max()}")
    ref = arg_ref if ref_given is None else ref_given
    ref_under_ref = min_ref if ref_given is None else chosen_ref[1]
    k = C.shape[0]
    cg, cr = np.asarray(c_next_got, np.float64), np.asarray(c_next_ref, np.float64)
    flipped = np.nonzero(got != ref)[0]
    gap = np.abs(chosen_ref[0][flipped] - ref_under_ref[flipped])
    assert (gap < 2 * KM_TIE + 2 * delta).all(), (f"{what}: ids differ on rows whose candidate centres are NOT within "
                                                  f"2*{KM_TIE} + 2*{delta:.2e}: rows {flipped[gap >= 2 * KM_TIE + 2 * delta][:5]}")
    for j in range(k):
        members = got == j
        n = int(members.sum())
        if n:
            mean = X[members].mean(0)
            assert np.abs(cg[j] - mean).max() < 2e-5, f"{what}: centre {j} is not the mean of its {n} members"
        else:
            assert np.abs(cg[j]).max() < 1e-5, f"{what}: empty cluster {j} must collapse to ~0 (kmeans_quantize.py:209)"
        touching = flipped[(got[flipped] == j) | (ref[flipped] == j)]
        allowed = KM_CENTER_TOL + sum(np.abs(X[r] - cr[j]).max() for r in touching) / max(min(n, int((ref == j).sum())), 1)
        assert np.abs(cg[j] - cr[j]).max() <= allowed, (f"{what}: centre {j} off by {np.abs(cg[j] - cr[j]).max()} with "
                                                          f"{len(touching)} flipped rows touching it (allowed {allowed})")
    return len(flipped), float(np.abs(cg - cr).max())


def kmeans_final_ids_attribution(feat, c_ref, ids_ref, c_got, ids_got, what=""):
    """End of a multi-iteration run: centres may differ by delta (itself bounded by the caller), which shifts every
    distance by <= delta -- so an id may differ from the reference's only where the two candidate centres are within
    KM_TIE + 2 * delta of each other for that row (float64, reference centres)."""
    X = np.asarray(feat, np.float64)
    C = np.asarray(c_ref, np.float64)
    delta = float(np.abs(np.asarray(c_got, np.float64) - C).max())
    got, ref = np.asarray(ids_got, np.int64), np.asarray(ids_ref, np.int64)
    bad = np.nonzero(got != ref)[0]
    if len(bad) == 0:
        return 0
    da = np.sqrt(((X[bad] - C[got[bad]]) ** 2).sum(-1))
    db = np.sqrt(((X[bad] - C[ref[bad]]) ** 2).sum(-1))
    gap = np.abs(da - db)
    assert (gap < KM_TIE + 2 * delta).all(), (f"{what}: ids differ on rows whose candidate centres are NOT within "
                                              f"{KM_TIE} + 2*{delta:.2e}: rows {bad[gap >= KM_TIE + 2 * delta][:5]}, gap {gap.max()}")
    return len(bad)
