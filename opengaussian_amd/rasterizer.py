"""Drop-in Python surface of the reference's rasterizer package.

Mirrors ``ashawkey_diff_gaussian_rasterization`` as the reference uses it
(/root/reference/gaussian_renderer/__init__.py:15,55-70,104-112; utils/sam_refinement_utils.py:21,347-402):
``GaussianRasterizationSettings`` (12-field NamedTuple), ``GaussianRasterizer(raster_settings=...)`` called with
keyword args ``means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp`` and
returning ``(color[3,H,W], radii[P] int32, depth[1,H,W], alpha[1,H,W])``; ``markVisible(positions)``.

Underneath is the C ABI of include/ogs_raster.h (HIP kernels for gfx950) bound with ctypes; torch only
provides device memory, the current stream and autograd.  There is no CPU path: non-GPU tensors raise.

Extension beyond the reference API: ``colors_precomp`` may carry 3, 6, 9 or 12
channels; one pass then bins/sorts once and blends all channels (``color`` is [C,H,W]).
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import _lib
from ._lib import OgsRasterBwdArgs, OgsRasterFwdArgs, OgsRawModel, OgsRawModelGrads, check, ptr

SUPPORTED_CHANNELS = (3, 6, 9, 12)
BACKWARD_CHANNELS = (3, 6, 9)          # the gradient record holds C + 7 <= 16 slots
# Passes with at most this many Gaussians (ungrouped) take the two-launch tiny path (ogs_raster_forward_tiny): the
# SAM refiner's P = 1 footprint renders and other very small subsets.  0 disables it (the parity tests that export the
# binning state of small scenes do).  Never larger than ogs_raster_tiny_max_points().
TINY_MAX_P = 256
# diagnostics (scripts/diag_repeat.py): when set to a list, every backward appends its raw gradient-record buffer
_DEBUG_KEEP_BWD_TMP = None
# diagnostics / tests: when set to a list, every streaming pass appends (num_rendered, pairs its render phase expanded) -- the
# second comes from a blocking read-back (ogs_raster_read_num_emitted); default-mode passes expand fewer pairs than they report
_DEBUG_EMITTED = None
# Capacity hint of the sync-free render phase: (P, W, H) -> num_rendered of the most recent passes at that size.
# The cameras of a training run take turns, so one pass's count does not predict the next one's: the
# capacity is 1.25x the MAXIMUM over the last _HINT_WINDOW passes -- after one sweep over the views it covers all of
# them; a scene that shrinks (pruning) lets the old maxima age out of the window.
_LAST_NUM_RENDERED: dict = {}
_HINT_WINDOW = 32
# how the render phase of every forward was sized: "blocking" (first pass at a size, grouped / debug passes: the
# reference's 4-byte read-back), "deferred" (sync-free, capacity from the hint), "overflow" (deferred result
# discarded, render phase redone with exact buffers)
# "raw_model": passes taken from the model's raw parameters (rasterize_model), counted besides the sizing mode they used
PASS_STATS = {"blocking": 0, "deferred": 0, "overflow": 0, "tiny": 0, "tiny_rerendered_for_backward": 0, "reblend": 0,
              "raw_model": 0}


def _hint_capacity(key):
    hist = _LAST_NUM_RENDERED.get(key)
    if not hist:
        return None
    return int(max(hist) * 1.25) + 4096


def _hint_record(key, D):
    from collections import deque
    if len(_LAST_NUM_RENDERED) > 256:      # subset renders come in many sizes: keep the hint table small
        _LAST_NUM_RENDERED.clear()
    hist = _LAST_NUM_RENDERED.get(key)
    if hist is None:
        hist = _LAST_NUM_RENDERED[key] = deque(maxlen=_HINT_WINDOW)
    hist.append(int(D))


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


_READBACK: dict = {}


def _readback_slot(dev):
    """One pinned int32 + one event per device, reused by every pass: the forward waits for the copy before it
    returns, so two passes never have a read-back in flight at the same time (pinned allocations are slow)."""
    slot = _READBACK.get(dev)
    if slot is None:
        slot = (torch.empty(1, dtype=torch.int32, pin_memory=True), torch.cuda.Event())
        _READBACK[dev] = slot
    return slot


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _f32c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """contiguous fp32 view/copy (inputs may be sliced / boolean-indexed views, :133,204-212).  Tensors that already
    are contiguous fp32 pass through untouched: a tiny pass is all host overhead, every torch call counts."""
    if t is None or t.numel() == 0:
        return None
    if t.dtype is torch.float32 and t.is_contiguous():
        return t.detach() if t.requires_grad else t
    return t.detach().to(torch.float32).contiguous()


_TINY_LIMIT = None
_TINY_SCRATCH: dict = {}


def _tiny_limit() -> int:
    global _TINY_LIMIT
    if _TINY_LIMIT is None:
        _TINY_LIMIT = int(_lib.lib().ogs_raster_tiny_max_points())
    return min(TINY_MAX_P, _TINY_LIMIT)


def _tiny_scratch(dev, stream: int, lib):
    """geom_buffer + geom_tmp of a tiny pass (<= 256 Gaussians, 12 channels: a few tens of KB), one pair per (device,
    stream): both are dead when the two launches of the pass have run, and passes on one stream are ordered."""
    key = (dev, stream)
    sc = _TINY_SCRATCH.get(key)
    if sc is None:
        n = int(lib.ogs_raster_tiny_max_points())
        sc = (torch.empty(int(lib.ogs_raster_geom_bytes(n, 12)), dtype=torch.uint8, device=dev),
              torch.empty(int(lib.ogs_raster_geom_tmp_bytes(n)), dtype=torch.uint8, device=dev))
        _TINY_SCRATCH[key] = sc
    return sc


_BG_TILED: dict = {}


def _tiled_bg(bg: torch.Tensor, Cn: int) -> torch.Tensor:
    """the 3-wide background tiled over a fused pass's channels; cached per (storage, version, stream): training passes the same
    background tensor every iteration and a `repeat` is a launch plus an allocation on a path that is all host time.
    Per stream, like _TINY_SCRATCH: the `repeat` runs on the stream of the pass that first asks, and nothing would order a pass
    on another stream that found the entry behind it (it blended an untiled, uninitialised background)."""
    key = (bg.data_ptr(), bg._version, Cn, bg.device, _stream())
    hit = _BG_TILED.get(key)
    if hit is None:
        if len(_BG_TILED) > 16:
            _BG_TILED.clear()
        hit = (bg, bg.repeat(Cn // 3))        # the source is held too: its address cannot be recycled while cached
        _BG_TILED[key] = hit
    return hit[1]


def _require_gpu(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); the MI355X rasterizer has no CPU path")


# ---- the steps every pass of the facade shares (_RasterizeGaussians, _RasterizeModel, _ReblendKept, the statistics passes) ----
def _pass_bg(rs, Cn: int, dev) -> torch.Tensor:
    """the settings' background as contiguous fp32 on `dev`, one entry per blended channel"""
    bg = _f32c(rs.bg.to(dev))
    if bg is None or bg.numel() != Cn:
        if bg is not None and bg.numel() == 3 and Cn > 3:
            # the facade's bg is 3-wide and the reference applies it to EVERY 3-channel pass (RGB, feat[:, :3],
            # feat[:, 3:6], gaussian_renderer/__init__.py:55-70,129-151): tile it over the fused channels
            bg = _tiled_bg(bg, Cn)
        else:
            raise RuntimeError(f"bg must have {Cn} entries")
    return bg


def _require_backward_channels(Cn: int, wants_grad: bool):
    if Cn not in BACKWARD_CHANNELS and wants_grad:
        # fail in the forward, not in the middle of loss.backward()
        raise RuntimeError(f"a {Cn}-channel pass is forward-only (backward supports {BACKWARD_CHANNELS} channels): "
                           "detach the inputs or split the pass")


def _pass_camera(rs, dev):
    """(viewmatrix, projmatrix, campos) of the settings as contiguous fp32 on `dev`"""
    return _f32c(rs.viewmatrix.to(dev)), _f32c(rs.projmatrix.to(dev)), _f32c(rs.campos.to(dev))


def _pass_outputs(P, Cn, H, W, dev, G=1):
    """(color, depth, alpha, radii) of a pass, in _fwd_args' order; a grouped pass has one image per group.
    P > 0: the kernels write every pixel of every tile and every radius, so no fill pass is needed; P == 0: zero images.
    Three separate image tensors (not views of one allocation): callers may modify an output in place."""
    alloc = torch.zeros if P == 0 else torch.empty
    lead = (G,) if G > 1 else ()
    return (alloc(*lead, Cn, H, W, dtype=torch.float32, device=dev), alloc(*lead, 1, H, W, dtype=torch.float32, device=dev),
            alloc(*lead, 1, H, W, dtype=torch.float32, device=dev), alloc(P, dtype=torch.int32, device=dev))


# Binning mode of the passes issued from this process (OgsRasterFwdArgs.full_binning, include/ogs_raster.h).  False (default): the
# (Gaussian, tile) pairs that cannot reach a pixel of their tile leave the list in the first pass of the tile sort.  True: the
# reference's full list is kept -- what tests/helpers.py::hip_export_binning compares with the oracle's binning entry by entry.
FULL_BINNING = os.environ.get("OGS_FULL_BINNING", "0") == "1"      # the environment variable is for A-B timing runs


class full_binning:
    """Context manager: passes issued inside keep the reference's full (Gaussian, tile) list (diagnostics / parity tests)."""

    def __enter__(self):
        global FULL_BINNING
        self._prev, FULL_BINNING = FULL_BINNING, True
        return self

    def __exit__(self, *exc):
        global FULL_BINNING
        FULL_BINNING = self._prev
        return False


# The forward blend zeroes the backward's gradient record on its way (OgsRasterFwdArgs.bwd_clear) instead of a fill launch at the
# start of ogs_raster_backward.  False withholds the pointer: the backward clears the record itself (A-B runs, tests).
HOST_BWD_CLEAR = True


def _grad_record_bytes(need, P, Cn, shs, cols, scl, rot, cov, pose=False) -> int:
    """Bytes of the gradient record ogs_raster_backward uses (and clears) for the gradient families `need` selects: 64 per
    Gaussian when only dL/dcolors_precomp of at most 8 channels is produced (features-only pass), else 128 (csrc/ogs_common.h
    grad_stride / feat_grad_stride; the backward supports Cn <= 9).  pose: the camera tensors train -- never features-only, the
    full record even when no per-Gaussian family is selected."""
    if pose:
        return P * 128
    want_cols = bool(need[3]) and cols is not None
    other = (need[0] or need[1] or (need[2] and shs is not None) or need[4] or (need[5] and scl is not None)
             or (need[6] and rot is not None) or (need[7] and cov is not None))
    feat_only = want_cols and not other
    feat_sums = Cn - (3 if shs is not None else 0)
    return P * (64 if (feat_only and feat_sums <= 8) else 128)


def _camera_leaves(rs):
    """(viewmatrix, projmatrix, campos) of the settings when autograd has to reach one of them, else (): the three trailing
    inputs of _RasterizeGaussians / _RasterizeModel.  Empty for every caller whose camera is a constant, whose call is then
    argument for argument what it was before the camera could train."""
    cam = (rs.viewmatrix, rs.projmatrix, rs.campos)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in cam):
        return cam
    return ()


def _pose_outputs(lib, b, P, dev):
    """allocates the three camera gradients and their scratch and points `b` at them; returns (g_view, g_proj, g_campos, tmp)"""
    g_view = torch.empty(16, dtype=torch.float32, device=dev)
    g_proj = torch.empty(16, dtype=torch.float32, device=dev)
    g_campos = torch.empty(3, dtype=torch.float32, device=dev)
    tmp = torch.empty(int(lib.ogs_raster_backward_pose_tmp_bytes(P)), dtype=torch.uint8, device=dev)
    b.dL_dviewmatrix, b.dL_dprojmatrix, b.dL_dcampos, b.pose_tmp = ptr(g_view), ptr(g_proj), ptr(g_campos), ptr(tmp)
    return g_view, g_proj, g_campos, tmp


def _pose_like(cam):
    """(shape, dtype, device) of the three camera inputs: what their gradients must look like (the tensors are not held)"""
    return tuple((t.shape, t.dtype, t.device) for t in cam)


def _pose_grads(need3, pose_out, like):
    """the gradients autograd gets for the three camera inputs: in their shapes, dtypes and devices, None where not needed.
    pose_out: what _pose_outputs returned, None for a pass whose camera is a constant"""
    if pose_out is None:
        return None, None, None
    return tuple(g.reshape(shape).to(device=dev, dtype=dtype) if n else None
                 for n, g, (shape, dtype, dev) in zip(need3, pose_out[:3], like))


def _fwd_args(rs, P, Cn, m3, shs, cols, opac, scl, rot, cov, bg, view, proj, campos, color, depth, alpha, radii, group_ids, G):
    a = OgsRasterFwdArgs()
    a.P, a.W, a.H, a.C = P, int(rs.image_width), int(rs.image_height), Cn
    a.sh_degree = int(rs.sh_degree)
    a.sh_coeffs = 0 if shs is None else int(shs.shape[1])
    a.tanfovx, a.tanfovy, a.scale_modifier = float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier)
    a.prefiltered, a.debug = int(bool(rs.prefiltered)), int(bool(rs.debug))
    a.bg, a.means3D, a.colors_precomp, a.shs, a.opacities = ptr(bg), ptr(m3), ptr(cols), ptr(shs), ptr(opac)
    a.scales, a.rotations, a.cov3D_precomp = ptr(scl), ptr(rot), ptr(cov)
    a.viewmatrix, a.projmatrix, a.campos = ptr(view), ptr(proj), ptr(campos)
    a.out_color, a.out_depth, a.out_alpha, a.radii = ptr(color), ptr(depth), ptr(alpha), ptr(radii)
    a.group_ids, a.num_groups = ptr(group_ids), G
    a.full_binning = int(FULL_BINNING)
    return a


def _bwd_args(ctx, lib, m3, cols, bg, view, proj, campos, radii, alpha, kept, upstream, g_m3, g_m2, g_col, record):
    """The OgsRasterBwdArgs fields the backwards of _RasterizeGaussians and _RasterizeModel share; the callers add sh_coeffs and
    their own inputs and gradients.  kept: (geom, image, point_list, sorted_rec, quad_list); upstream: backward()'s (grad_color,
    grad_depth, grad_alpha); record: _take_record's (bwd_tmp, is_clear).  Returns (b, hold): `b` carries raw pointers only, the
    caller keeps `hold` until its launch is queued -- the contiguous fp32 upstream gradients and, last, what _pose_outputs
    allocated when the camera trains (else None)."""
    rs, P, Cn = ctx.raster_settings, ctx.P, ctx.Cn
    W, H = int(rs.image_width), int(rs.image_height)
    geom, image, point_list, sorted_rec, quad_list = kept
    # depth and alpha stay None when no loss touched them (the kernels compile their terms out); the colour gradient is what
    # the backward launches over: zeros in its place
    gc, gd, ga = _f32c(upstream[0]), _f32c(upstream[1]), _f32c(upstream[2])
    if gc is None:
        gc = torch.zeros(*((ctx.num_groups,) if ctx.num_groups > 1 else ()), Cn, H, W, dtype=torch.float32, device=m3.device)
    b = OgsRasterBwdArgs()
    b.P, b.W, b.H, b.C = P, W, H, Cn
    b.sh_degree = int(rs.sh_degree)
    b.tanfovx, b.tanfovy, b.scale_modifier = float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier)
    b.debug = int(bool(rs.debug))
    b.num_rendered, b.geom_channels, b.num_groups = int(ctx.num_rendered), int(ctx.geom_channels), int(ctx.num_groups)
    b.geom_buffer, b.image_buffer, b.point_list = ptr(geom), ptr(image), ptr(point_list)
    b.sorted_rec, b.quad_list = ptr(sorted_rec), ptr(quad_list)
    b.bg, b.means3D, b.colors_precomp = ptr(bg), ptr(m3), ptr(cols)
    b.viewmatrix, b.projmatrix, b.campos = ptr(view), ptr(proj), ptr(campos)
    b.radii, b.out_alpha = ptr(radii), ptr(alpha)
    b.dL_dcolor, b.dL_ddepth, b.dL_dalpha = ptr(gc), ptr(gd), ptr(ga)
    b.dL_dmeans2D, b.dL_dcolors, b.dL_dmeans3D = ptr(g_m2), ptr(g_col), ptr(g_m3)
    b.bwd_tmp, b.bwd_tmp_is_clear = ptr(record[0]), int(record[1])
    pose_out = _pose_outputs(lib, b, P, m3.device) if ctx.pose_like is not None else None
    return b, (gc, gd, ga, pose_out)


# scratch sizes are pure functions of the shape: asked once per shape, not six ctypes calls per pass (a 100 k-Gaussian step is
# paced by the host)
@functools.lru_cache(maxsize=256)
def _geom_sizes(P, W, H, Cn, G):
    lib = _lib.lib()
    return (int(lib.ogs_raster_geom_bytes(P, Cn)), int(lib.ogs_raster_geom_tmp_bytes(P)),
            int(lib.ogs_raster_image_bytes_grouped(W, H, G)))


@functools.lru_cache(maxsize=1024)
def _render_sizes(count, W, H, Cn):
    lib = _lib.lib()
    return (int(lib.ogs_raster_binning_tmp_bytes(count, W, H)), int(lib.ogs_raster_sorted_bytes(count, Cn)),
            int(lib.ogs_raster_quad_list_bytes(count)))


def _streaming_render(a: OgsRasterFwdArgs, dev, lib, debug: bool, raw: Optional[OgsRawModel] = None):
    """The two-phase forward (geometry -> num_rendered -> render) on the buffers `a` already points to for inputs
    and outputs; allocates and returns (geom, image, point_list, sorted_rec, quad_list, num_rendered).
    raw: the geometry phase reads the model's raw parameters (include/ogs_model.h; `a` then has no shs / opacities / scales /
    rotations); the render phase is the same call either way."""
    P, W, H, Cn, G = int(a.P), int(a.W), int(a.H), int(a.C), max(int(a.num_groups), 1)
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device=dev)
    gb, gtb, ib = _geom_sizes(P, W, H, Cn, G)
    geom, geom_tmp, image = u8(gb), u8(gtb), u8(ib)
    a.geom_buffer, a.geom_tmp, a.image_buffer = ptr(geom), ptr(geom_tmp), ptr(image)
    stream = _stream()

    def alloc_render(count):
        btb, srb, qlb = _render_sizes(count, W, H, Cn)
        pl = torch.empty(max(count, 1), dtype=torch.int32, device=dev)
        bt, sr, ql = u8(btb), u8(srb), u8(qlb)
        a.point_list, a.binning_tmp, a.sorted_rec, a.quad_list = ptr(pl), ptr(bt), ptr(sr), ptr(ql)
        return pl, bt, sr, ql

    def geometry(n_ref):
        if raw is None:
            check(lib.ogs_raster_forward_geometry(C.byref(a), stream, n_ref), "ogs_raster_forward_geometry")
            return
        check(lib.ogs_raster_forward_geometry_raw(C.byref(a), C.byref(raw), stream, n_ref), "ogs_raster_forward_geometry_raw")
        # what the render phase's argument check wants to see (include/ogs_model.h): it reads none of them
        a.shs, a.opacities, a.scales, a.rotations = raw.features_dc, raw.opacity, raw.scaling, raw.rotation

    key = (P, W, H, G)
    # grouped passes: num_rendered follows the group ids of the call (cluster chunk, leaf range), which change
    # from call to call -> sized by the blocking read-back, like subset passes (their P is new every time)
    cap = None if (G > 1 or debug) else _hint_capacity(key)
    if cap is None:
        PASS_STATS["blocking"] += 1
        # first pass at this size: blocking 4-byte read-back of num_rendered (what the reference does every time)
        n = C.c_int64(0)
        geometry(C.byref(n))
        D = int(n.value)
        point_list, bin_tmp, sorted_rec, quad_list = alloc_render(D)
        check(lib.ogs_raster_forward_render(C.byref(a), D, stream), "ogs_raster_forward_render")
    else:
        # steady state: no GPU idle gap.  The render phase is enqueued for a capacity derived from the recent
        # passes at this size; the true count arrives through an async pinned copy and is only WAITED for after
        # everything is queued.  Overflow (scene changed a lot) -> redo the render phase with exact buffers.
        geometry(None)
        pinned, ev = _readback_slot(dev)
        check(lib.ogs_raster_read_num_rendered_async(C.byref(a), stream, pinned.data_ptr()),
              "ogs_raster_read_num_rendered_async")
        ev.record()
        PASS_STATS["deferred"] += 1
        point_list, bin_tmp, sorted_rec, quad_list = alloc_render(cap)
        check(lib.ogs_raster_forward_render_deferred(C.byref(a), cap, stream), "ogs_raster_forward_render_deferred")
        ev.synchronize()
        # the geometry phase of THIS pass (its depth sort) and every earlier launch have finished: anything a kernel reported
        # through the sticky status word (a one-launch radix pass whose bounded look-back wait ran out) raises here
        check(lib.ogs_check_async_status(), "ogs_check_async_status")
        D = int(pinned.item()) & 0xFFFFFFFF
        if D > cap:
            PASS_STATS["overflow"] += 1
            point_list, bin_tmp, sorted_rec, quad_list = alloc_render(D)
            check(lib.ogs_raster_forward_render(C.byref(a), D, stream), "ogs_raster_forward_render")
    _hint_record(key, D)
    if _DEBUG_EMITTED is not None:
        n = C.c_uint32(0)
        check(lib.ogs_raster_read_num_emitted(C.byref(a), stream, C.byref(n)), "ogs_raster_read_num_emitted")
        _DEBUG_EMITTED.append((D, int(n.value)))
    return geom, image, point_list, sorted_rec, quad_list, D


# ---- the pass behind _RasterizeGaussians and _RasterizeModel: each keeps its own input checks, argument positions and
# save_for_backward layout (code outside this file reads them); what runs between is here, once ----------------------------
def _init_ctx(ctx, rs, P, Cn, G):
    """what a pass that launched nothing (P == 0) leaves on its autograd node; _forward_pass overwrites its part"""
    ctx.raster_settings = rs
    ctx.P, ctx.Cn, ctx.num_groups, ctx.num_rendered, ctx.tiny = P, Cn, G, 0, False
    ctx.bwd_tmp, ctx.bwd_clear_bytes = None, 0
    ctx.full_binning = bool(FULL_BINNING)


def _forward_pass(ctx, a: OgsRasterFwdArgs, raw: Optional[OgsRawModel], dev, G, force_streaming, wants_grad, record_bytes):
    """Runs the forward `a` describes (raw: from the model's raw parameters) and leaves tiny / num_rendered / bwd_tmp /
    bwd_clear_bytes on `ctx`.  Returns the state backward needs, (geom, image, point_list, sorted_rec, quad_list), or None for
    a tiny pass, which keeps nothing.  record_bytes: the gradient record the backward of this pass will use, known from the
    requires_grad flags (_grad_record_bytes)."""
    lib = _lib.lib()
    debug = bool(a.debug)
    if G == 1 and not debug and int(a.P) <= _tiny_limit() and not force_streaming:
        # tiny pass: two launches, no read-back, nothing kept -- backward() re-renders through the streaming path
        stream = _stream()
        geom, geom_tmp = _tiny_scratch(dev, stream, lib)
        a.geom_buffer, a.geom_tmp = geom.data_ptr(), geom_tmp.data_ptr()
        if raw is None:
            check(lib.ogs_raster_forward_tiny(C.byref(a), stream), "ogs_raster_forward_tiny")
        else:
            check(lib.ogs_raster_forward_tiny_raw(C.byref(a), C.byref(raw), stream), "ogs_raster_forward_tiny_raw")
        PASS_STATS["tiny"] += 1
        ctx.tiny, ctx.num_rendered = True, -1
        return None
    bwd_tmp = None
    if HOST_BWD_CLEAR and G == 1 and not debug and wants_grad:
        # the gradient record of this pass' backward: allocated here, zeroed by the render phase on its way, held until the
        # backward runs
        bwd_tmp = torch.empty(int(lib.ogs_raster_backward_tmp_bytes(int(a.P))), dtype=torch.uint8, device=dev)
        a.bwd_clear, a.bwd_clear_bytes = ptr(bwd_tmp), record_bytes
    state = _streaming_render(a, dev, lib, debug, raw)
    ctx.num_rendered = state[5]
    if bwd_tmp is not None:
        # every render call of _streaming_render carried the pointer: the range is zero in stream order
        ctx.bwd_tmp, ctx.bwd_clear_bytes = bwd_tmp, record_bytes
    return state[:5]


def _backward_state(ctx, lib, saved, inputs, raw: Optional[OgsRawModel] = None):
    """(kept, scratch) for a backward: kept = (geom, image, point_list, sorted_rec, quad_list), saved by a streaming pass and
    rendered again for a tiny one.  saved: ctx.saved_tensors; inputs: _fwd_args' seven per-Gaussian tensors (means3D ..
    cov3D_precomp) of that re-render; raw: it reads the model's raw parameters.  scratch: the re-render's outputs, which the
    CALLER holds until its backward launch is queued (None for a streaming pass)."""
    if not ctx.tiny:
        return saved[13:], None
    # a tiny pass keeps nothing: re-render through the streaming path (scratch outputs) to obtain the binning
    # and blend state the backward kernels read.  Rare: the refiner's footprint renders never call backward.
    rs, P, Cn = ctx.raster_settings, ctx.P, ctx.Cn
    dev = saved[0].device
    # scratch outputs: held by the caller until the re-render has been enqueued AND everything else of its
    # backward has been allocated -- `a` only carries raw pointers, a tensor freed here would be handed out
    # again by the caching allocator while the kernels still write through the old pointer
    scratch = _pass_outputs(P, Cn, int(rs.image_height), int(rs.image_width), dev)
    a = _fwd_args(rs, P, Cn, *inputs, *saved[7:11], *scratch, None, 1)          # saved[7:11]: bg, view, proj, campos
    if raw is not None:
        a.sh_coeffs = ctx.M
    state = _streaming_render(a, dev, lib, False, raw)
    ctx.num_rendered = state[5]
    PASS_STATS["tiny_rerendered_for_backward"] += 1
    return state[:5], scratch


def _take_record(ctx, lib, needed_bytes, dev):
    """(bwd_tmp, is_clear): the gradient record the forward left zeroed, once -- after this backward it is dirty, a second
    backward over a retained graph takes a fresh buffer and the fill (as does a pass whose forward hosted no clear)"""
    bwd_tmp, ctx.bwd_tmp = ctx.bwd_tmp, None
    if bwd_tmp is None:
        return torch.empty(int(lib.ogs_raster_backward_tmp_bytes(ctx.P)), dtype=torch.uint8, device=dev), False
    is_clear, ctx.bwd_clear_bytes = ctx.bwd_clear_bytes >= needed_bytes, 0
    return bwd_tmp, is_clear


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings: GaussianRasterizationSettings, geom_channels: int = 0, sh_rgb_sink=None,
                group_ids=None, num_groups: int = 1, keep_sink=None, force_streaming: bool = False,
                viewmatrix=None, projmatrix=None, campos=None):
        # viewmatrix / projmatrix / campos (optional): the settings' camera tensors again, as autograd inputs (_camera_leaves) --
        # given when one of them requires grad; the pass reads the camera from the settings either way
        # force_streaming (internal, label_map): a P <= TINY_MAX_P pass takes the streaming path, which leaves the state a
        # label map walks; the default path selection is untouched
        rs = raster_settings
        ctx.geom_channels = int(geom_channels)
        ctx.sh_rgb_sink = sh_rgb_sink
        # outputs no loss touches (depth in every reference loss, alpha without RGBA data) must reach backward as
        # None, not as zero images: the kernels compile the corresponding terms out
        ctx.set_materialize_grads(False)
        G = max(int(num_groups), 1)
        pose = any(ctx.needs_input_grad[15:18])
        ctx.pose_like = _pose_like((viewmatrix, projmatrix, campos)) if pose else None
        if pose and G > 1:
            raise RuntimeError("camera gradients of a grouped pass are not supported: detach the camera tensors")
        if G > 1:
            if group_ids is None or group_ids.shape[0] != means3D.shape[0]:
                raise RuntimeError("a grouped pass needs group_ids [P]")
            group_ids = group_ids.detach().to(device=means3D.device, dtype=torch.int32).contiguous()
        else:
            group_ids = None
        _require_gpu(means3D, "means3D")
        dev = means3D.device
        P = int(means3D.shape[0])
        H, W = int(rs.image_height), int(rs.image_width)
        if means3D.dim() != 2 or means3D.shape[1] != 3:
            raise RuntimeError("means3D must have dimensions (num_points, 3)")

        m3 = _f32c(means3D)
        shs = _f32c(sh)
        cols = _f32c(colors_precomp)
        opac = _f32c(opacities)
        scl = _f32c(scales)
        rot = _f32c(rotations)
        cov = _f32c(cov3Ds_precomp)
        if shs is not None and cols is not None:
            Cn = 3 + int(cols.shape[1])        # fused pass: SH -> channels 0..2, colors_precomp -> the rest
        else:
            Cn = 3 if cols is None else int(cols.shape[1])
        if Cn not in SUPPORTED_CHANNELS:
            raise RuntimeError(f"the blended channel count must be 3, 6, 9 or 12, got {Cn}")
        need = ctx.needs_input_grad
        wants_grad = any(need[:8]) or pose
        _require_backward_channels(Cn, wants_grad)
        bg = _pass_bg(rs, Cn, dev)
        view, proj, campos = _pass_camera(rs, dev)
        color, depth, alpha, radii = _pass_outputs(P, Cn, H, W, dev, G)
        _init_ctx(ctx, rs, P, Cn, G)
        ctx.mark_non_differentiable(radii)
        if P == 0:
            # reference behaviour: zero images, nothing launched (SURVEY.md section 8(b) "Errors")
            ctx.save_for_backward()
            return color, radii, depth, alpha

        a = _fwd_args(rs, P, Cn, m3, shs, cols, opac, scl, rot, cov, bg, view, proj, campos, color, depth, alpha, radii,
                      group_ids, G)
        kept = _forward_pass(ctx, a, None, dev, G, force_streaming, wants_grad,
                             _grad_record_bytes(need, P, Cn, shs, cols, scl, rot, cov, pose))
        # the layout is read from outside: 13 inputs and outputs, then the kept state (absent after a tiny pass)
        ctx.save_for_backward(m3, shs, cols, opac, scl, rot, cov, bg, view, proj, campos, radii, alpha, *(kept or ()))
        if keep_sink is not None and G == 1 and kept is not None and ctx.num_rendered > 0:
            # frozen-geometry cache (KeptPasses below): what a re-blend of this pass needs
            _, image, _, sorted_rec, quad_list = kept
            keep_sink.append({"P": P, "W": W, "H": H, "Cn": Cn, "fused": shs is not None and cols is not None,
                              "D": ctx.num_rendered, "image": image, "sorted_rec": sorted_rec, "quad_list": quad_list,
                              "radii": radii, "full_binning": bool(FULL_BINNING)})
        return color, radii, depth, alpha

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_alpha):
        P, Cn = ctx.P, ctx.Cn
        if P == 0:
            return (None,) * 18
        lib = _lib.lib()
        saved = ctx.saved_tensors
        m3, shs, cols, opac, scl, rot, cov, bg, view, proj, campos, radii, alpha = saved[:13]
        kept, scratch = _backward_state(ctx, lib, saved, (m3, shs, cols, opac, scl, rot, cov))
        dev = m3.device
        need = ctx.needs_input_grad   # means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3D
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)

        g_m3 = z(P, 3) if need[0] else None
        g_m2 = z(P, 3) if need[1] else None
        # data-parallel mode (dp.ShGradExchange): hand out the rank-1 factor [P,3] instead of the dense dL/dsh
        sink = ctx.sh_rgb_sink if (need[2] and shs is not None) else None
        g_sh = z(*shs.shape) if (need[2] and shs is not None and sink is None) else None
        g_sh_rgb = z(P, 3) if sink is not None else None
        g_col = z(*cols.shape) if (need[3] and cols is not None) else None
        g_op = z(P, 1) if need[4] else None
        g_scl = z(P, 3) if (need[5] and scl is not None) else None
        g_rot = z(P, 4) if (need[6] and rot is not None) else None
        g_cov = z(P, 6) if (need[7] and cov is not None) else None

        record = _take_record(ctx, lib, _grad_record_bytes(need, P, Cn, shs, cols, scl, rot, cov, ctx.pose_like is not None), dev)
        b, hold = _bwd_args(ctx, lib, m3, cols, bg, view, proj, campos, radii, alpha, kept, (grad_color, grad_depth, grad_alpha),
                            g_m3, g_m2, g_col, record)
        b.sh_coeffs = 0 if shs is None else int(shs.shape[1])
        b.shs, b.opacities, b.scales, b.rotations, b.cov3D_precomp = ptr(shs), ptr(opac), ptr(scl), ptr(rot), ptr(cov)
        b.dL_dsh, b.dL_dopacity, b.dL_dscales, b.dL_drotations, b.dL_dcov3D = ptr(g_sh), ptr(g_op), ptr(g_scl), ptr(g_rot), ptr(g_cov)
        b.dL_dsh_rgb = ptr(g_sh_rgb)
        check(lib.ogs_raster_backward(C.byref(b), _stream()), "ogs_raster_backward")
        scratch = None          # (tiny pass re-render) stream-ordered: safe to recycle once the launches are queued
        if _DEBUG_KEEP_BWD_TMP is not None:
            _DEBUG_KEEP_BWD_TMP.append(record[0])
        if sink is not None:
            sink.append(g_sh_rgb)
        return (g_m3, g_m2, g_sh, g_col, g_op, g_scl, g_rot, g_cov, None, None, None, None, None, None, None) + \
            _pose_grads(need[15:18], hold[3], ctx.pose_like)


# ---- kept passes: the frozen-geometry cache ------------------------------------------------------------------------------
# From stage 1 on the reference trains `_ins_feat` alone: train.py:431-436 detaches every other Gaussian parameter, and the
# stage-1 calls render without the random footprint rescale (train.py:346-350).  For a given camera every such call rebuilds,
# entry for entry, the binning state of the previous one -- preprocess, both sorts, the duplication and pack are spent on
# reproducing bytes that already exist.  With 288 GB of HBM they can simply stay: a finished pass whose caller vouches for its
# geometry (`frozen_key`, renderer.py builds it from the parameters' storages and version counters) leaves image_buffer, the
# packed records, their quadrant streams and the radii behind (0.35 GB for a 1080p view of 1 M Gaussians, 0.08 GB for a
# ScanNet-class view whose tiles stop at 15 % of their lists: compacted to what the tiles packed), and the next pass with the same
# key is ogs_raster_forward_reblend: ONE launch, the forward blend over the kept streams with the records' feature channels taken
# from the caller's current tensor (the kept records are never written).
# Images, depth, alpha, radii and the feature gradients are bit for bit those of a full pass (tests/test_14_kept_pass_gpu.py).
class _KeptPass:
    __slots__ = ("key", "generation", "holds", "P", "W", "H", "Cn", "E", "fused", "D", "image", "sorted_rec", "quad_list", "radii",
                 "nbytes", "hits", "full_binning")


class KeptPasses:
    """One kept pass per SLOT (a camera); a slot whose key changed (parameters stepped, replaced, another image size ...) is
    dropped on lookup.  Admission stops at the byte budget -- nothing is evicted to make room: the training loop draws its
    cameras from a shuffled stack (train.py:296-299), the access pattern on which least-recently-used eviction hits nothing
    once the working set exceeds the budget, while a fixed resident subset keeps hitting for its share of the views."""

    def __init__(self, budget_bytes=None):
        self.budget_bytes = budget_bytes          # None: OGS_KEPT_PASSES_GB, default min(device / 4, free / 2) at first use
        self.slots: dict = {}
        self.nbytes = 0
        self.stats = {"hits": 0, "misses": 0, "stale": 0, "admitted": 0, "rejected_budget": 0, "dropped_old_generation": 0,
                      "rejected_out_of_memory": 0}

    def _budget(self, dev) -> int:
        if self.budget_bytes is None:
            env = os.environ.get("OGS_KEPT_PASSES_GB")
            if env is not None:
                self.budget_bytes = int(float(env) * (1 << 30))
            else:
                # a quarter of the device, but never more than half of what is free when the first pass asks: the cache must not
                # be what pushes the training process into an out-of-memory error
                free, total = torch.cuda.mem_get_info(dev)
                self.budget_bytes = int(min(total // 4, free // 2))
        return self.budget_bytes

    def enabled(self, dev) -> bool:
        return self._budget(dev) > 0

    def lookup(self, slot, key):
        e = self.slots.get(slot)
        if e is None:
            self.stats["misses"] += 1
            return None
        if e.key != key:
            self.drop(slot)
            self.stats["stale"] += 1
            self.stats["misses"] += 1
            return None
        e.hits += 1
        self.stats["hits"] += 1
        return e

    def drop(self, slot):
        e = self.slots.pop(slot, None)
        if e is not None:
            self.nbytes -= e.nbytes

    def clear(self):
        self.slots.clear()
        self.nbytes = 0

    def admit(self, slot, key, holds, kept: dict, generation=None) -> bool:
        """kept: what _RasterizeGaussians.forward left in its keep_sink.  The record array and the quadrant streams of the pass
        were sized for a CAPACITY (1.25 x the recent maximum of num_rendered, and the reachable pairs are about half of it) and
        laid out by the sorted list's tile ranges: the records and stream entries the tiles actually PACKED are moved into
        exact-size buffers (ogs_raster_compact_kept) -- one 8-byte read-back per admitted view.
        generation: what all passes over ONE state of the model share (renderer.py: the parameters' part of the key).  Entries
        of another generation can never hit again -- the model moved on, or another scene was loaded -- but cameras that are
        not revisited would hold their bytes (and the old parameters) forever: when the budget is short they go first."""
        dev = kept["image"].device
        lib = _lib.lib()
        W, H, Cn = kept["W"], kept["H"], kept["Cn"]
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        image = kept["image"]
        # image_buffer layout (include/ogs_raster.h, ogs_raster_compact_kept): ranges | n_contrib | counters | final_T | tile_order
        up = lambda n: (n + 255) // 256 * 256
        o_cnt = up(tiles * 8) + up(W * H * 4)
        packed = image[o_cnt:o_cnt + tiles * 20].view(torch.int32).view(tiles, 5)[:, 4].to(torch.int64)   # records per tile
        ends = torch.cumsum(packed, 0)
        used = int(ends[-1].item())                           # the one read-back of an admission
        if used <= 0:
            return False
        srb, qlb = int(lib.ogs_raster_sorted_bytes(used, Cn)), int(lib.ogs_raster_quad_list_bytes(used))
        nbytes = srb + qlb + image.numel() + kept["radii"].numel() * 4
        if self.nbytes + nbytes > self._budget(dev) and generation is not None:
            for old_slot in [sl for sl, en in self.slots.items() if en.generation != generation]:
                self.drop(old_slot)
                self.stats["dropped_old_generation"] += 1
        if self.nbytes + nbytes > self._budget(dev):
            self.stats["rejected_budget"] += 1
            return False
        e = _KeptPass()
        e.key, e.holds, e.generation = key, holds, generation
        e.P, e.W, e.H, e.Cn, e.fused, e.D = kept["P"], W, H, Cn, bool(kept["fused"]), used
        e.E = Cn - 3 if e.fused else Cn
        e.full_binning = kept["full_binning"]
        try:
            # the entry's own copy (4 B per Gaussian): the pass already handed `radii` to its caller, who may write into it
            e.radii = kept["radii"].clone()
            # the pass laid its records and quadrant streams out by the ranges of the sorted list, sized for a capacity; what is
            # kept is what the tiles PACKED (all a re-blend reads), re-laid out by the exclusive scan of those counts
            e.image = image.clone()
            new_ranges = torch.stack((ends - packed, ends), 1).to(torch.int32).contiguous()
            e.image[: tiles * 8] = new_ranges.view(-1).view(torch.uint8)
            e.sorted_rec = torch.empty(srb, dtype=torch.uint8, device=dev)
            e.quad_list = torch.empty(qlb, dtype=torch.uint8, device=dev)
        except torch.cuda.OutOfMemoryError:
            # the budget is a share of the device, not of what the training process left free: keeping a pass is optional
            self.stats["rejected_out_of_memory"] += 1
            return False
        check(lib.ogs_raster_compact_kept(W, H, Cn, ptr(image), ptr(kept["sorted_rec"]), ptr(kept["quad_list"]), ptr(e.image),
                                          ptr(e.sorted_rec), ptr(e.quad_list), _stream()), "ogs_raster_compact_kept")
        e.nbytes, e.hits = nbytes, 0
        self.drop(slot)
        self.slots[slot] = e
        self.nbytes += nbytes
        self.stats["admitted"] += 1
        return True


KEPT_PASSES = KeptPasses()


class KeptImages:
    """Outputs of a pass in which NOTHING trains: stage >= 1 renders RGB from frozen parameters on every call (the unfused RGB pass
    of the rescaled stage-2.1 calls, gaussian_renderer/__init__.py:104-112, and every stage-2.2 call, train.py:339-341) -- for a
    given camera, model state and background tensor the same image, depth, alpha and radii, bit for bit, every time.  45 MB per
    1080p view.  Same slots / keys / generations / budget rules as KeptPasses; a hit hands out CLONES (callers may modify what
    they get)."""

    def __init__(self, budget_bytes=None):
        self.budget_bytes = budget_bytes          # None: the budget of KEPT_PASSES (counted separately)
        self.slots: dict = {}
        self.nbytes = 0
        self.stats = {"hits": 0, "misses": 0, "stale": 0, "admitted": 0, "rejected_budget": 0}

    def _budget(self, dev) -> int:
        return KEPT_PASSES._budget(dev) if self.budget_bytes is None else self.budget_bytes

    def lookup(self, slot, key):
        e = self.slots.get(slot)
        if e is None or e[0] != key:
            if e is not None:
                self.drop(slot)
                self.stats["stale"] += 1
            self.stats["misses"] += 1
            return None
        self.stats["hits"] += 1
        return tuple(t.clone() for t in e[3])

    def drop(self, slot):
        e = self.slots.pop(slot, None)
        if e is not None:
            self.nbytes -= e[4]

    def clear(self):
        self.slots.clear()
        self.nbytes = 0

    def admit(self, slot, key, holds, outputs, generation=None) -> bool:
        dev = outputs[0].device
        nbytes = sum(t.numel() * t.element_size() for t in outputs)
        if self.nbytes + nbytes > self._budget(dev) and generation is not None:
            for old_slot in [sl for sl, en in self.slots.items() if en[1] != generation]:
                self.drop(old_slot)
        if self.nbytes + nbytes > self._budget(dev):
            self.stats["rejected_budget"] += 1
            return False
        try:
            kept = tuple(t.detach().clone() for t in outputs)
        except torch.cuda.OutOfMemoryError:
            return False
        self.drop(slot)
        self.slots[slot] = (key, generation, holds, kept, nbytes)
        self.nbytes += nbytes
        self.stats["admitted"] += 1
        return True


KEPT_IMAGES = KeptImages()


def clear_kept():
    """Forget every kept pass and kept image (after parameter values were written behind torch's back: torch ops on `.data`, a
    foreign kernel on `data_ptr()`; this library's own raw-pointer writers move the version counters themselves)."""
    KEPT_PASSES.clear()
    KEPT_IMAGES.clear()


class _ReblendKept(torch.autograd.Function):
    """forward: ogs_raster_forward_reblend on a kept pass; backward: the features-only ogs_raster_backward on the same state."""

    @staticmethod
    def forward(ctx, extra_feats, entry: _KeptPass, raster_settings: GaussianRasterizationSettings):
        rs = raster_settings
        ctx.set_materialize_grads(False)
        _require_gpu(extra_feats, "colors_precomp")
        dev = extra_feats.device
        lib = _lib.lib()
        P, W, H, Cn = entry.P, entry.W, entry.H, entry.Cn
        cols = _f32c(extra_feats)
        if cols is None or tuple(cols.shape) != (P, entry.E):
            raise RuntimeError(f"the kept pass blends {entry.E} caller channels of {P} Gaussians, got {tuple(extra_feats.shape)}")
        _require_backward_channels(Cn, ctx.needs_input_grad[0])
        bg = _pass_bg(rs, Cn, dev)
        color = torch.empty(Cn, H, W, dtype=torch.float32, device=dev)
        depth = torch.empty(1, H, W, dtype=torch.float32, device=dev)
        alpha = torch.empty(1, H, W, dtype=torch.float32, device=dev)
        a = _kept_args((P, W, H, Cn, entry.image, entry.sorted_rec, entry.quad_list))
        a.sh_coeffs = 1 if entry.fused else 0          # flag only: channels 0..2 of the kept records stay (header)
        a.debug = int(bool(rs.debug))
        a.bg, a.colors_precomp = ptr(bg), ptr(cols)
        a.out_color, a.out_depth, a.out_alpha = ptr(color), ptr(depth), ptr(alpha)
        check(lib.ogs_raster_forward_reblend(C.byref(a), _stream()), "ogs_raster_forward_reblend")
        PASS_STATS["reblend"] += 1
        ctx.entry, ctx.raster_settings = entry, rs
        ctx.save_for_backward(cols)
        radii = entry.radii.clone()                    # the kept pass' radii, as the caller's own tensor (backward reads the entry's)
        ctx.mark_non_differentiable(radii)
        return color, radii, depth, alpha

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_alpha):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        e, rs = ctx.entry, ctx.raster_settings
        (cols,) = ctx.saved_tensors
        dev = cols.device
        lib = _lib.lib()
        gc = _f32c(grad_color)
        if gc is None:
            return torch.zeros_like(cols), None, None
        g_col = torch.empty(e.P, e.E, dtype=torch.float32, device=dev)
        bwd_tmp = torch.empty(int(lib.ogs_raster_backward_tmp_bytes(e.P)), dtype=torch.uint8, device=dev)
        b = OgsRasterBwdArgs()
        b.P, b.W, b.H, b.C = e.P, e.W, e.H, e.Cn
        b.debug = int(bool(rs.debug))
        b.num_rendered, b.num_groups = int(e.D), 1
        b.colors_precomp = ptr(cols)
        b.shs = ptr(cols) if e.fused else None         # tested against NULL only in the features-only pass (header)
        b.radii, b.dL_dcolor = ptr(e.radii), ptr(gc)
        b.image_buffer, b.sorted_rec, b.quad_list, b.bwd_tmp = ptr(e.image), ptr(e.sorted_rec), ptr(e.quad_list), ptr(bwd_tmp)
        b.dL_dcolors = ptr(g_col)
        check(lib.ogs_raster_backward(C.byref(b), _stream()), "ogs_raster_backward")
        return g_col, None, None


def _kept_state(kept, who):
    """(P, W, H, Cn, image, sorted_rec, quad_list) of what a pass left in its keep_sink (a dict) or of a KeptPasses entry."""
    if isinstance(kept, _KeptPass):
        return kept.P, kept.W, kept.H, kept.Cn, kept.image, kept.sorted_rec, kept.quad_list
    if isinstance(kept, dict) and all(k in kept for k in ("P", "W", "H", "Cn", "image", "sorted_rec", "quad_list")):
        return (int(kept["P"]), int(kept["W"]), int(kept["H"]), int(kept["Cn"]), kept["image"], kept["sorted_rec"],
                kept["quad_list"])
    raise RuntimeError(f"{who} needs the state of an ungrouped streaming pass: the dict a pass leaves in keep_sink or a "
                       "KeptPasses entry (grouped and tiny passes keep none)")


def _kept_args(state):
    """the OgsRasterFwdArgs every call over a kept pass gives: sizes and the three kept buffers of a `_kept_state`"""
    P, W, H, Cn, image, sorted_rec, quad_list = state
    a = OgsRasterFwdArgs()
    a.P, a.W, a.H, a.C = P, W, H, Cn
    a.image_buffer, a.sorted_rec, a.quad_list = ptr(image), ptr(sorted_rec), ptr(quad_list)
    return a


def _int32_or_outside(t, upper, dev):
    """an integer tensor as contiguous int32 on `dev`; a value outside [0, upper) becomes -1 BEFORE the narrowing, so a 64-bit
    value outside the int32 range stays outside instead of wrapping into range"""
    t = t.detach().to(device=dev)
    if t.dtype is not torch.int32:
        t = torch.where((t >= 0) & (t < upper), t, torch.full_like(t, -1)).to(torch.int32)
    return t.contiguous()


def _check_rows(rows, P):
    if rows is None:
        return
    if not torch.is_tensor(rows) or rows.is_floating_point() or rows.is_complex() or rows.dtype is torch.bool:
        raise RuntimeError("rows must be an integer tensor")
    if rows.numel() != P:
        raise RuntimeError(f"the pass holds {P} Gaussians, rows has {rows.numel()} entries")


def _votes_rows(rows, num_rows, P):
    """the row count of a vote table: num_rows (required with `rows`), else one row per Gaussian"""
    _check_rows(rows, P)
    if rows is not None and num_rows is None:
        raise RuntimeError("num_rows must be given with rows")
    Rn = P if num_rows is None else int(num_rows)
    if Rn < 1 or Rn > 2 ** 31 - 1:
        raise RuntimeError(f"num_rows must be in [1, 2^31), got {num_rows}")
    return Rn


def _rows_int32(rows, Rn, dev):
    return None if rows is None else _int32_or_outside(rows.reshape(-1), Rn, dev)


def _check_votes_out(out, Rn, cols):
    if out is not None and (not torch.is_tensor(out) or out.dtype is not torch.int64 or tuple(out.shape) != (Rn, cols)
                            or not out.is_contiguous()):
        raise RuntimeError(f"out must be a contiguous int64 tensor [{Rn}, {cols}]")


def _require_gpu_all(state, **tensors):
    """the named arguments that were given, then the kept pass itself, in that order; returns the pass's device"""
    for name, t in tensors.items():
        if t is not None:
            _require_gpu(t, name)
    _require_gpu(state[4], "the kept pass")
    return state[4].device


def label_map(kept, labels, num_labels):
    """Per-pixel dominant label of a finished pass (ogs_raster_label_map, include/ogs_query.h): ONE launch over the kept quadrant
    streams, O(H * W) memory whatever `num_labels` is.

    kept: what an ungrouped streaming pass left in ``keep_sink``, or a ``KeptPasses`` entry.  labels: [P] integer tensor on the
    GPU; a value outside [0, num_labels) marks an unlabelled Gaussian, which occludes and never wins.
    Returns ``(label [H,W] int32, weight [H,W], second [H,W], alpha [H,W])``: the label with the largest summed blend weight
    (lowest label on an exact tie, -1 where no labelled Gaussian contributed), that weight, the runner-up label's weight, and
    the pass's own alpha image bit for bit.  Forward only; two calls give the same bytes."""
    state = _kept_state(kept, "label_map")
    P, W, H = state[:3]
    if not torch.is_tensor(labels):
        raise RuntimeError("labels must be a tensor")
    if labels.is_floating_point() or labels.is_complex() or labels.dtype is torch.bool:
        raise RuntimeError(f"labels must have an integer dtype, got {labels.dtype}")
    if labels.numel() != P:
        raise RuntimeError(f"the pass holds {P} Gaussians, labels has {labels.numel()} entries")
    L = int(num_labels)
    if L < 0 or L > 2 ** 31 - 1:
        raise RuntimeError(f"num_labels must be in [0, 2^31), got {num_labels}")
    dev = _require_gpu_all(state, labels=labels)
    lab = _int32_or_outside(labels.reshape(-1), L, dev)
    out_label = torch.empty(H, W, dtype=torch.int32, device=dev)
    weight = torch.empty(H, W, dtype=torch.float32, device=dev)
    second = torch.empty(H, W, dtype=torch.float32, device=dev)
    alpha = torch.empty(H, W, dtype=torch.float32, device=dev)
    lm = _lib.OgsLabelMapArgs()
    lm.labels, lm.num_labels = ptr(lab), L
    lm.out_label, lm.out_weight, lm.out_second, lm.out_alpha = ptr(out_label), ptr(weight), ptr(second), ptr(alpha)
    check(_lib.lib().ogs_raster_label_map(C.byref(_kept_args(state)), C.byref(lm), _stream()), "ogs_raster_label_map")
    return out_label, weight, second, alpha


def label_votes(kept, pixel_labels, num_labels, rows=None, num_rows=None, out=None):
    """Pixel labels lifted to Gaussians (ogs_raster_label_votes, include/ogs_query.h): ONE launch over the kept quadrant streams.

    kept: what an ungrouped streaming pass left in ``keep_sink``, or a ``KeptPasses`` entry.  pixel_labels: [H, W] integer tensor
    on the GPU; a value outside [0, num_labels) counts in column ``num_labels`` (no label).  rows: [P] integer tensor mapping
    every Gaussian to a table row (a leaf id, say), a row outside [0, num_rows) is not counted but still occludes; None: the
    Gaussian's own index, num_rows = P.
    Returns the int64 table [num_rows, num_labels + 1] in fixed point, quantum 2^-32 (``query.votes_as_float``):
    cell [r, l] = summed blend weight alpha * T that the Gaussians of row r put on the pixels of label l.  ``out`` (same shape,
    int64, on the GPU) is ACCUMULATED into and returned, so several views sum into one table; without it a zeroed table is made.
    Forward only; integer accumulation: two calls give the same bytes."""
    state = _kept_state(kept, "label_votes")
    P, W, H = state[:3]
    if not torch.is_tensor(pixel_labels):
        raise RuntimeError("pixel_labels must be a tensor")
    if pixel_labels.is_floating_point() or pixel_labels.is_complex() or pixel_labels.dtype is torch.bool:
        raise RuntimeError(f"pixel_labels must have an integer dtype, got {pixel_labels.dtype}")
    if tuple(pixel_labels.shape) != (H, W):
        raise RuntimeError(f"the pass is {H} x {W} pixels, pixel_labels is {tuple(pixel_labels.shape)}")
    L = int(num_labels)
    if L < 0 or L > 2 ** 31 - 2:
        raise RuntimeError(f"num_labels must be in [0, 2^31 - 1), got {num_labels}")
    Rn = _votes_rows(rows, num_rows, P)
    _check_votes_out(out, Rn, L + 1)
    dev = _require_gpu_all(state, pixel_labels=pixel_labels, rows=rows, out=out)
    lab = _int32_or_outside(pixel_labels, L, dev)
    row = _rows_int32(rows, Rn, dev)
    votes = torch.zeros(Rn, L + 1, dtype=torch.int64, device=dev) if out is None else out
    lv = _lib.OgsLabelVotesArgs()
    lv.pixel_labels, lv.num_labels = ptr(lab), L
    lv.rows, lv.num_rows = ptr(row), Rn
    lv.votes = ptr(votes)
    check(_lib.lib().ogs_raster_label_votes(C.byref(_kept_args(state)), C.byref(lv), _stream()), "ogs_raster_label_votes")
    if out is not None:
        _lib.mark_written(out)                         # the caller's table, accumulated into through its raw pointer
    return votes


def feature_votes(kept, features, valid=None, rows=None, num_rows=None, out=None):
    """A dense feature image lifted to Gaussians (ogs_raster_feature_votes, include/ogs_query.h): ONE call and one launch over the
    kept quadrant streams whatever D is.

    kept: what an ungrouped streaming pass left in ``keep_sink``, or a ``KeptPasses`` entry.  features: floating tensor [D, H, W]
    on the GPU (CLIP / DINO / LSeg maps, ``pesudo_ins_feat``, an error image, a depth residual), used as contiguous fp32.
    valid: optional bool or integer [H, W]; a zero pixel contributes to no column (it still occludes and is occluded).  rows:
    [P] integer tensor mapping every Gaussian to a table row (a leaf id, say), a row outside [0, num_rows) is not counted but
    still occludes; None: the Gaussian's own index, num_rows = P.
    Returns the int64 table [num_rows, D + 1] in fixed point, quantum 2^-32 (``query.votes_as_float``,
    ``query.features_from_votes``): cell [r, c < D] = sum over the valid pixels of alpha * T * F[c] of the Gaussians of row r, cell
    [r, D] the summed weight alpha * T itself.  ``out`` (same shape, int64, on the GPU) is ACCUMULATED into and returned, so
    several views sum into one table; without it a zeroed table is made.  Forward only; integer accumulation: two calls give the
    same bytes, and the channels may be split over several calls.

    Range contract (nothing is read back to check it): the features are finite; one partial (one Gaussian, one 8 x 8 quadrant)
    stays below 2^31 after scaling, i.e. ``64 * max|F| < 2^31``; a cell stays below 2^31 of summed magnitude.
    Cost: one walk of the pass per 32 columns plus 8 bytes of atomics per (Gaussian, quadrant, column); the atomics are more than
    half of the time from D = 16 on.  Against ``ceil((D + 1) / 9)`` features-only backward launches with F as the upstream
    gradient it is 1.6-1.9 x faster at D = 64 and 512; at D <= 16 (one or two such launches) the two routes cost the same
    within the spread of the measurement, and with ``rows`` at D = 16 the backward route was 2 % ahead.
    That route is not reproducible to the byte, has no ``valid`` / ``rows`` and needs a [P, D + 1] fp32 table."""
    state = _kept_state(kept, "feature_votes")
    P, W, H = state[:3]
    if not torch.is_tensor(features):
        raise RuntimeError("features must be a tensor")
    if not features.is_floating_point():
        raise RuntimeError(f"features must have a floating dtype, got {features.dtype}")
    if features.dim() != 3 or tuple(features.shape[1:]) != (H, W) or features.shape[0] < 1:
        raise RuntimeError(f"the pass is {H} x {W} pixels, features must be [D >= 1, {H}, {W}], got {tuple(features.shape)}")
    D = int(features.shape[0])
    if D > 2 ** 31 - 2:
        raise RuntimeError(f"features has {D} channels, the limit is 2^31 - 2")
    if valid is not None:
        if not torch.is_tensor(valid) or valid.is_floating_point() or valid.is_complex():
            raise RuntimeError("valid must be a bool or integer tensor")
        if tuple(valid.shape) != (H, W):
            raise RuntimeError(f"the pass is {H} x {W} pixels, valid is {tuple(valid.shape)}")
    Rn = _votes_rows(rows, num_rows, P)
    _check_votes_out(out, Rn, D + 1)
    dev = _require_gpu_all(state, features=features, valid=valid, rows=rows, out=out)
    feat = features.detach().to(device=dev, dtype=torch.float32).contiguous()
    ok = None if valid is None else (valid.detach().to(device=dev) != 0).to(torch.uint8).contiguous()
    row = _rows_int32(rows, Rn, dev)
    votes = torch.zeros(Rn, D + 1, dtype=torch.int64, device=dev) if out is None else out
    fv = _lib.OgsFeatureVotesArgs()
    fv.features, fv.num_channels = ptr(feat), D
    fv.valid = ptr(ok)
    fv.rows, fv.num_rows = ptr(row), Rn
    fv.votes = ptr(votes)
    check(_lib.lib().ogs_raster_feature_votes(C.byref(_kept_args(state)), C.byref(fv), _stream()), "ogs_raster_feature_votes")
    if out is not None:
        _lib.mark_written(out)
    return votes


def feature_map(kept, features, rows=None, channels_last=False, with_alpha=False):
    """A feature table rendered into the view of a finished pass (ogs_raster_feature_map, include/ogs_query.h): ONE call and one
    launch over the kept quadrant streams whatever D is -- the transpose of ``feature_votes``.

    kept: what an ungrouped streaming pass left in ``keep_sink``, or a ``KeptPasses`` entry.  features: floating tensor [R, D]
    on the GPU (lifted CLIP / DINO / LSeg features per Gaussian or per leaf, instance features), used as contiguous fp32; it
    must be finite.  rows: [P] integer tensor mapping every Gaussian to a row of the table (``leaf_ind``), a row outside [0, R)
    occludes and adds nothing; None: the Gaussian's own index, and R must be P.
    Returns the map, fp32 [D, H, W] (``channels_last``: [H, W, D]): per pixel and column the forward blend's own chain
    ``acc = fmaf(alpha * T, X[row, c], acc)`` in depth order with a zero background, bit for bit what ``ceil(D / 12)`` re-blends
    of a 12-channel kept pass over slices of ``X[rows]`` give.  ``with_alpha``: ``(map, alpha [H, W])``, the pass's own alpha
    image, so ``map / alpha`` is the blend-weighted mean feature and ``map + (1 - alpha) * bg`` adds a background.
    Forward only (``query.render_feature_map`` is differentiable in the features); no atomics: two calls give the same bytes.

    Cost: one walk of the pass per 64 columns (``ogs_feature_map_block_columns()``) plus the map itself, D * H * W * 4 bytes
    written once.  Against the re-blend route it is 2.1-2.4 x faster at D = 64 and 512 and needs neither a [P, D] copy of a
    per-leaf table nor a 12-channel kept pass; at D = 16 the two routes cost the same, and a map of up to 12 channels is ONE
    re-blend of a kept pass, which is the better call there (0.21 against 0.37 ms on the bench scene)."""
    state = _kept_state(kept, "feature_map")
    P, W, H = state[:3]
    if not torch.is_tensor(features):
        raise RuntimeError("features must be a tensor")
    if not features.is_floating_point():
        raise RuntimeError(f"features must have a floating dtype, got {features.dtype}")
    if features.dim() != 2 or features.shape[0] < 1 or features.shape[1] < 1:
        raise RuntimeError(f"features must be [R >= 1, D >= 1], got {tuple(features.shape)}")
    Rn, D = int(features.shape[0]), int(features.shape[1])
    if Rn > 2 ** 31 - 1 or D > 2 ** 31 - 1:
        raise RuntimeError(f"features is {Rn} x {D}, the limit is 2^31 - 1 each way")
    _check_rows(rows, P)
    if rows is None and Rn != P:
        raise RuntimeError(f"the pass holds {P} Gaussians, features has {Rn} rows (give rows to map Gaussians to rows)")
    dev = _require_gpu_all(state, features=features, rows=rows)
    feat = features.detach().to(device=dev, dtype=torch.float32).contiguous()
    row = _rows_int32(rows, Rn, dev)
    out = torch.empty((H, W, D) if channels_last else (D, H, W), dtype=torch.float32, device=dev)
    alpha = torch.empty(H, W, dtype=torch.float32, device=dev) if with_alpha else None
    fm = _lib.OgsFeatureMapArgs()
    fm.features, fm.num_channels = ptr(feat), D
    fm.rows, fm.num_rows = ptr(row), Rn
    fm.channels_last = int(bool(channels_last))
    fm.out_map, fm.out_alpha = ptr(out), ptr(alpha)
    check(_lib.lib().ogs_raster_feature_map(C.byref(_kept_args(state)), C.byref(fm), _stream()), "ogs_raster_feature_map")
    return (out, alpha) if with_alpha else out


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, sh_rgb_sink=None):
    """sh_rgb_sink (extension, data parallelism): a list.  When given, backward does NOT produce the dense
    dL/dsh (shs.grad stays None); it appends the [P,3] clamp-masked gradient of the SH-evaluated RGB instead, from
    which dp.ShGradExchange rebuilds the sum over views of dL/dsh (see include/ogs_raster.h, dL_dsh_rgb)."""
    cam = _camera_leaves(raster_settings)
    if cam:
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                         cov3Ds_precomp, raster_settings, 0, sh_rgb_sink, None, 1, None, False, *cam)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, 0, sh_rgb_sink)


def rasterize_fused(means3D, means2D, opacities, shs, extra_feats, raster_settings, scales=None, rotations=None,
                    cov3D_precomp=None, detach_extra_from_geometry=True, sh_rgb_sink=None, frozen_key=None):
    """ONE pass for what the reference renders in several (gaussian_renderer/__init__.py:104-163): RGB from SH in
    channels 0..2 plus `extra_feats` [P, 3|6|9] (e.g. the 6-D ins_feat) in the following channels -- one
    preprocess / sort / blend for all of them.  Returns (color [3+E,H,W], radii, depth, alpha).

    detach_extra_from_geometry=True reproduces the stage-1/2 training graph (train.py:431-436): the loss on the
    extra channels reaches only `extra_feats`; geometry, opacity and means2D receive gradient from the RGB /
    depth / alpha outputs alone -- bit-for-bit what two separate reference passes (RGB with all gradients, feature
    pass with everything else detached) would accumulate.

    frozen_key (extension): ``(slot, key, holds[, generation])`` -- the caller vouches that every input but `extra_feats` (and the
    background) is the same whenever `key` is the same (renderer.py: storages + version counters of the model's parameters,
    the camera, the image size).  When none of those inputs requires grad, the first pass of a slot is kept (KEPT_PASSES,
    budget OGS_KEPT_PASSES_GB, 0 = off) and later passes with an equal key re-blend it: one launch instead of the
    whole binning pipeline, same bits.  `holds` (any object) is kept alive with the entry so that the addresses in `key`
    cannot be recycled while it exists; `generation` (optional, hashable) names the model state the key belongs to: entries
    of other generations are dropped first when the budget is short."""
    empty = torch.Tensor([])
    args = (means3D, means2D, shs, extra_feats, opacities, empty if scales is None else scales,
            empty if rotations is None else rotations, empty if cov3D_precomp is None else cov3D_precomp, raster_settings,
            3 if detach_extra_from_geometry else 0, sh_rgb_sink)
    cam = _camera_leaves(raster_settings)
    if cam:
        # a camera that trains: nothing of the pass is frozen, whatever `frozen_key` vouches for
        return _RasterizeGaussians.apply(*args, None, 1, None, False, *cam)
    if frozen_key is None or not means3D.is_cuda or not KEPT_PASSES.enabled(means3D.device) or raster_settings.debug or \
            (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in
                                             (means3D, means2D, opacities, shs, scales, rotations, cov3D_precomp))):
        return _RasterizeGaussians.apply(*args)
    slot, key, holds = frozen_key[:3]
    generation = frozen_key[3] if len(frozen_key) > 3 else None
    key = (key, bool(FULL_BINNING), int(extra_feats.shape[-1]))
    entry = KEPT_PASSES.lookup(slot, key)
    if entry is not None:
        return _ReblendKept.apply(extra_feats, entry, raster_settings)
    sink: list = []
    out = _RasterizeGaussians.apply(*args, None, 1, sink)
    if sink:
        KEPT_PASSES.admit(slot, key, holds, sink[0], generation)
    return out


def _raw_model_struct(dc, rest, opac, scl, rot) -> OgsRawModel:
    raw = OgsRawModel()
    raw.features_dc, raw.features_rest, raw.scaling, raw.rotation, raw.opacity = ptr(dc), ptr(rest), ptr(scl), ptr(rot), ptr(opac)
    return raw


class _RasterizeModel(torch.autograd.Function):
    """The fused SH pass of _RasterizeGaussians taken from the model's raw parameters (include/ogs_model.h): the activations
    of the reference's getters (scene/gaussian_model.py:122-159) run inside the per-Gaussian kernels, forward and backward."""

    @staticmethod
    def forward(ctx, means3D, means2D, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw, extra_feats,
                raster_settings: GaussianRasterizationSettings, geom_channels: int = 0, viewmatrix=None, projmatrix=None,
                campos=None):
        rs = raster_settings
        ctx.geom_channels = int(geom_channels)
        ctx.set_materialize_grads(False)
        pose = any(ctx.needs_input_grad[10:13])         # as _RasterizeGaussians: the settings' camera tensors as inputs
        ctx.pose_like = _pose_like((viewmatrix, projmatrix, campos)) if pose else None
        for t, name in ((means3D, "means3D"), (features_dc, "features_dc"), (opacity_raw, "opacity_raw"),
                        (scaling_raw, "scaling_raw"), (rotation_raw, "rotation_raw")):
            _require_gpu(t, name)
        dev = means3D.device
        P = int(means3D.shape[0])
        H, W = int(rs.image_height), int(rs.image_width)
        if means3D.dim() != 2 or means3D.shape[1] != 3:
            raise RuntimeError("means3D must have dimensions (num_points, 3)")
        if tuple(features_dc.shape) != (P, 1, 3) or tuple(scaling_raw.shape) != (P, 3) or tuple(rotation_raw.shape) != (P, 4) \
                or opacity_raw.numel() != P:
            raise RuntimeError("raw model: features_dc [P,1,3], scaling [P,3], rotation [P,4], opacity [P,1] expected")
        M = 1
        if features_rest is not None and features_rest.numel() > 0:
            if features_rest.dim() != 3 or features_rest.shape[0] != P or features_rest.shape[2] != 3:
                raise RuntimeError("raw model: features_rest must be [P, M-1, 3]")
            _require_gpu(features_rest, "features_rest")
            M += int(features_rest.shape[1])
        m3, dc, rest = _f32c(means3D), _f32c(features_dc), _f32c(features_rest)
        opac, scl, rot = _f32c(opacity_raw), _f32c(scaling_raw), _f32c(rotation_raw)
        cols = _f32c(extra_feats)
        if cols is not None:
            _require_gpu(cols, "extra_feats")
        Cn = 3 + (0 if cols is None else int(cols.shape[1]))
        if Cn not in SUPPORTED_CHANNELS:
            raise RuntimeError(f"the blended channel count must be 3, 6, 9 or 12, got {Cn}")
        need = ctx.needs_input_grad
        wants_grad = any(need[:8]) or pose
        _require_backward_channels(Cn, wants_grad)
        bg = _pass_bg(rs, Cn, dev)
        view, proj, campos = _pass_camera(rs, dev)
        color, depth, alpha, radii = _pass_outputs(P, Cn, H, W, dev)
        _init_ctx(ctx, rs, P, Cn, 1)
        ctx.M = M
        ctx.mark_non_differentiable(radii)
        if P == 0:
            ctx.save_for_backward()
            return color, radii, depth, alpha
        PASS_STATS["raw_model"] += 1
        a = _fwd_args(rs, P, Cn, m3, None, cols, None, None, None, None, bg, view, proj, campos, color, depth, alpha, radii, None, 1)
        a.sh_coeffs = M
        kept = _forward_pass(ctx, a, _raw_model_struct(dc, rest, opac, scl, rot), dev, 1, False, wants_grad,
                             _RasterizeModel._record_bytes(need, P, Cn, dc, cols, scl, rot, pose))
        # the layout is read from outside: _RasterizeGaussians' with (dc, rest) for (shs, cols) and cols for cov
        ctx.save_for_backward(m3, dc, rest, opac, scl, rot, cols, bg, view, proj, campos, radii, alpha, *(kept or ()))
        return color, radii, depth, alpha

    @staticmethod
    def _record_bytes(need, P, Cn, dc, cols, scl, rot, pose=False) -> int:
        # in _RasterizeGaussians' order: means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3D
        return _grad_record_bytes((need[0], need[1], need[2] or need[3], need[7], need[4], need[5], need[6], False), P, Cn, dc,
                                  cols, scl, rot, None, pose)

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_alpha):
        P, Cn, M = ctx.P, ctx.Cn, ctx.M
        if P == 0:
            return (None,) * 13
        lib = _lib.lib()
        saved = ctx.saved_tensors
        m3, dc, rest, opac, scl, rot, cols, bg, view, proj, campos, radii, alpha = saved[:13]
        raw = _raw_model_struct(dc, rest, opac, scl, rot)
        kept, scratch = _backward_state(ctx, lib, saved, (m3, None, cols, None, None, None, None), raw)
        dev = m3.device
        need = ctx.needs_input_grad   # means3D, means2D, features_dc, features_rest, opacity, scaling, rotation, extra_feats
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        g_m3 = z(P, 3) if need[0] else None
        g_m2 = z(P, 3) if need[1] else None
        g_dc = z(P, 1, 3) if need[2] else None
        g_rest = z(P, M - 1, 3) if (need[3] and rest is not None) else None
        g_op = z(P, 1) if need[4] else None
        g_scl = z(P, 3) if need[5] else None
        g_rot = z(P, 4) if need[6] else None
        g_col = z(*cols.shape) if (need[7] and cols is not None) else None
        record = _take_record(ctx, lib, _RasterizeModel._record_bytes(need, P, Cn, dc, cols, scl, rot, ctx.pose_like is not None), dev)
        b, hold = _bwd_args(ctx, lib, m3, cols, bg, view, proj, campos, radii, alpha, kept, (grad_color, grad_depth, grad_alpha),
                            g_m3, g_m2, g_col, record)
        b.sh_coeffs = M
        grads = OgsRawModelGrads()
        grads.features_dc, grads.features_rest, grads.scaling, grads.rotation, grads.opacity = \
            ptr(g_dc), ptr(g_rest), ptr(g_scl), ptr(g_rot), ptr(g_op)
        check(lib.ogs_raster_backward_raw(C.byref(b), C.byref(raw), C.byref(grads), _stream()), "ogs_raster_backward_raw")
        scratch = None          # (tiny pass re-render) stream-ordered: safe to recycle once the launches are queued
        return (g_m3, g_m2, g_dc, g_rest, g_op, g_scl, g_rot, g_col, None, None) + _pose_grads(need[10:13], hold[3], ctx.pose_like)


def rasterize_model(means3D, means2D, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw, raster_settings,
                    extra_feats=None, detach_extra_from_geometry=True):
    """rasterize_fused (or, without `extra_feats`, the plain SH pass) from the reference model's RAW parameters -- `_features_dc`
    [P,1,3], `_features_rest` [P,M-1,3] (None or empty: M = 1), `_opacity` [P,1] logits, `_scaling` [P,3] log-scales,
    `_rotation` [P,4] unnormalised quaternions -- instead of the getters' outputs (scene/gaussian_model.py:122-159: exp,
    F.normalize, sigmoid, cat).  The activations run inside the per-Gaussian kernels and the gradients come back with respect
    to the raw parameters: no activated copies, no torch graph between the parameters and the rasterizer.  Same four outputs,
    bit for bit those of the existing pass fed with activate_model's outputs.  CPU tensors raise: there is no fallback."""
    return _RasterizeModel.apply(means3D, means2D, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw,
                                 extra_feats, raster_settings, 3 if (detach_extra_from_geometry and extra_feats is not None) else 0,
                                 *_camera_leaves(raster_settings))


def activate_model(features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw):
    """(scales [P,3], rotations [P,4], opacities [P,1], shs [P,M,3]): the reference's four getters as ONE kernel
    (ogs_model_activate), through the device functions the raw pass uses.  No autograd (the outputs are detached)."""
    for t, name in ((features_dc, "features_dc"), (opacity_raw, "opacity_raw"), (scaling_raw, "scaling_raw"),
                    (rotation_raw, "rotation_raw")):
        _require_gpu(t, name)
    dev = features_dc.device
    P = int(features_dc.shape[0])
    M = 1 + (int(features_rest.shape[1]) if features_rest is not None and features_rest.numel() > 0 else 0)
    dc, rest = _f32c(features_dc), _f32c(features_rest)
    opac, scl, rot = _f32c(opacity_raw), _f32c(scaling_raw), _f32c(rotation_raw)
    e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
    scales, rotations, opacities, shs = e(P, 3), e(P, 4), e(P, 1), e(P, M, 3)
    if P:
        raw = _raw_model_struct(dc, rest, opac, scl, rot)
        check(_lib.lib().ogs_model_activate(P, M, C.byref(raw), ptr(scales), ptr(rotations), ptr(opacities), ptr(shs), _stream()),
              "ogs_model_activate")
    return scales, rotations, opacities, shs


def rasterize_groups(means3D, means2D, opacities, group_ids, num_groups, raster_settings, shs=None,
                     colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
    """Batched subset rendering: ONE pass returns, for every g in [0, num_groups), the
    images the reference obtains by calling the rasterizer on the boolean-indexed subset ``group_ids == g``
    (its per-cluster loops, gaussian_renderer/__init__.py:203-225,327-345): one preprocess, one sort and one
    launch sequence instead of num_groups of each, and no index copies of the inputs.

    Returns (color [G,C,H,W], radii [P], depth [G,1,H,W], alpha [G,1,H,W]); Gaussians whose id is outside
    [0, num_groups) are not rendered (radii 0).  Gradients flow to the full-size inputs."""
    empty = torch.Tensor([])
    if (shs is None) == (colors_precomp is None):
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')
    return _RasterizeGaussians.apply(means3D, means2D, empty if shs is None else shs,
                                     empty if colors_precomp is None else colors_precomp, opacities,
                                     empty if scales is None else scales, empty if rotations is None else rotations,
                                     empty if cov3D_precomp is None else cov3D_precomp, raster_settings, 0, None,
                                     group_ids, int(num_groups))


def _stats_inputs(means3D, opacities, raster_settings, colors_precomp, scales, rotations, cov3D_precomp):
    """fp32 contiguous inputs of a forward-only pass (statistics, preprocess-only); raises when autograd would be asked
    for a gradient no such pass can give."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                       for t in (means3D, opacities, colors_precomp, scales, rotations, cov3D_precomp)):
        raise RuntimeError("statistics / preprocess-only passes have no backward: detach the inputs or use torch.no_grad()")
    _require_gpu(means3D, "means3D")
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    if (scales is None) != (rotations is None) or (scales is None) == (cov3D_precomp is None):
        raise RuntimeError("provide exactly one of (scales, rotations) / cov3D_precomp")
    dev = means3D.device
    cols = _f32c(colors_precomp)
    if cols is None or cols.dim() != 2 or cols.shape[0] != means3D.shape[0]:
        if means3D.shape[0] != 0:
            raise RuntimeError("colors_precomp must be [P, C]")
    Cn = int(colors_precomp.shape[-1])
    if Cn not in SUPPORTED_CHANNELS:
        raise RuntimeError(f"the blended channel count must be 3, 6, 9 or 12, got {Cn}")
    bg = _pass_bg(raster_settings, Cn, dev)         # as every other pass of the facade: the 3-wide background over all channels
    return (Cn, _f32c(means3D), _f32c(opacities), cols, _f32c(scales), _f32c(rotations), _f32c(cov3D_precomp), bg,
            *_pass_camera(raster_settings, dev))


def visible_radii(means3D, opacities, raster_settings, colors_precomp, scales=None, rotations=None, cov3D_precomp=None):
    """Preprocess only: the int32 radii [P] an ungrouped pass over the same inputs returns (the geometry phase alone, no
    binning, no blend).  A radius depends on its own Gaussian only, so ``radii > 0`` is bit for bit the visibility filter of
    the reference's RGB pass of the same camera -- what the association drivers select subsets by before a statistics pass."""
    Cn, m3, opac, cols, scl, rot, cov, bg, view, proj, campos = _stats_inputs(
        means3D, opacities, raster_settings, colors_precomp, scales, rotations, cov3D_precomp)
    P = int(means3D.shape[0])
    dev = means3D.device
    radii = torch.zeros(P, dtype=torch.int32, device=dev)
    if P == 0:
        return radii
    lib = _lib.lib()
    a = _fwd_args(raster_settings, P, Cn, m3, None, cols, opac, scl, rot, cov, bg, view, proj, campos, None, None, None,
                  radii, None, 1)
    gb, gtb, _ = _geom_sizes(P, int(a.W), int(a.H), Cn, 1)
    geom = torch.empty(gb, dtype=torch.uint8, device=dev)
    geom_tmp = torch.empty(gtb, dtype=torch.uint8, device=dev)
    a.geom_buffer, a.geom_tmp = ptr(geom), ptr(geom_tmp)
    check(lib.ogs_raster_forward_geometry(C.byref(a), _stream(), None), "ogs_raster_forward_geometry")
    return radii


def rasterize_group_stats(means3D, opacities, group_ids, num_groups, labels, num_labels, raster_settings, colors_precomp,
                          scales=None, rotations=None, cov3D_precomp=None, alpha_threshold=0.5):
    """Per-(subset, label) statistics of a grouped pass, without its images (include/ogs_raster.h,
    ogs_raster_forward_group_stats).  For every g in [0, num_groups) -- the subset ``group_ids == g``, rendered as
    rasterize_groups renders it -- and every label l of the int32 label image ``labels`` [H, W] (values in [0, num_labels);
    -1 or anything else: bucket num_labels, "no mask"):

      max_alpha [G] fp32          the maximum of the subset's alpha image;
      count     [G, L+1] int64    the pixels with alpha > alpha_threshold carrying label l;
      feat_sum  [G, L+1, C] fp32  the sum over those pixels of the blended colour, background term included -- the
                                  values rasterize_groups writes to `color` (int64 fixed-point accumulation: the same
                                  bits every run);
      radii     [P] int32         as rasterize_groups returns them (0 outside the groups).

    Same alpha and colour per pixel as rasterize_groups, bit for bit, so every threshold decision agrees with its images;
    nothing of size G*H*W is allocated.  Forward only (raises when an input requires grad under grad mode).  Uses the
    blocking num_rendered read-back, as every grouped pass."""
    Cn, m3, opac, cols, scl, rot, cov, bg, view, proj, campos = _stats_inputs(
        means3D, opacities, raster_settings, colors_precomp, scales, rotations, cov3D_precomp)
    rs = raster_settings
    G, L = int(num_groups), int(num_labels)
    if G < 0 or L < 0:
        raise RuntimeError(f"num_groups ({G}) and num_labels ({L}) must be >= 0")
    H, W = int(rs.image_height), int(rs.image_width)
    dev = means3D.device
    P = int(means3D.shape[0])
    if labels.numel() != H * W:
        raise RuntimeError(f"labels must have H*W = {H * W} entries, got {tuple(labels.shape)}")
    lab = labels.to(device=dev, dtype=torch.int32).contiguous()
    max_alpha = torch.zeros(G, dtype=torch.float32, device=dev)
    count = torch.zeros(G, L + 1, dtype=torch.int64, device=dev)
    feat_sum = torch.zeros(G, L + 1, Cn, dtype=torch.float32, device=dev)
    radii = torch.zeros(P, dtype=torch.int32, device=dev)
    if G == 0:
        return max_alpha, count, feat_sum, radii
    gid = group_ids.to(device=dev, dtype=torch.int32).contiguous()
    if gid.numel() != P:
        raise RuntimeError("group_ids must be [P]")
    sub = None
    if G == 1:
        # the C ABI reads num_groups <= 1 as the ungrouped pass: a single subset is the plain pass on its members
        sub = gid == 0
        idx = lambda t: None if t is None else t[sub].contiguous()
        m3, opac, cols, scl, rot, cov = idx(m3), idx(opac), idx(cols), idx(scl), idx(rot), idx(cov)
        P_pass, gid_pass = int(m3.shape[0]), None
        sub_radii = torch.zeros(P_pass, dtype=torch.int32, device=dev)
    else:
        P_pass, gid_pass, sub_radii = P, gid, radii
    lib = _lib.lib()
    a = _fwd_args(rs, P_pass, Cn, m3, None, cols, opac, scl, rot, cov, bg, view, proj, campos, None, None, None, sub_radii,
                  gid_pass, G)
    if P_pass == 0:
        # nothing is read per Gaussian without Gaussians; the argument check wants a colour source and one covariance form
        a.colors_precomp = a.scales = a.rotations = ptr(bg)
        a.cov3D_precomp = None
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device=dev)
    stream = _stream()
    keep = []
    D = 0
    if P_pass > 0:
        gb, gtb, _ = _geom_sizes(P_pass, W, H, Cn, 1)
        keep += [u8(gb), u8(gtb)]
        a.geom_buffer, a.geom_tmp = ptr(keep[0]), ptr(keep[1])
        n = C.c_int64(0)
        PASS_STATS["blocking"] += 1
        check(lib.ogs_raster_forward_geometry(C.byref(a), stream, C.byref(n)), "ogs_raster_forward_geometry")
        D = int(n.value)
    image = u8(lib.ogs_raster_stats_image_bytes(W, H, G))
    tmp = u8(lib.ogs_raster_stats_tmp_bytes(G, L, Cn))
    a.image_buffer = ptr(image)
    if D > 0:
        btb, _, _ = _render_sizes(D, W, H, Cn)
        pl, bt = torch.empty(D, dtype=torch.int32, device=dev), u8(btb)
        keep += [pl, bt]
        a.point_list, a.binning_tmp = ptr(pl), ptr(bt)
    st = _lib.OgsGroupStatsArgs()
    st.labels, st.num_labels, st.alpha_threshold = ptr(lab), L, float(alpha_threshold)
    st.max_alpha, st.count, st.feat_sum, st.stats_tmp = ptr(max_alpha), ptr(count), ptr(feat_sum), ptr(tmp)
    check(lib.ogs_raster_forward_group_stats(C.byref(a), C.byref(st), D, stream), "ogs_raster_forward_group_stats")
    if sub is not None:
        radii[sub] = sub_radii
    return max_alpha, count, feat_sum, radii


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """bool[P]: near-plane test (upstream `mark_visible`; unused by the reference's own code)."""
        _require_gpu(positions, "positions")
        rs = self.raster_settings
        with torch.no_grad():
            pos = _f32c(positions)
            P = 0 if pos is None else int(pos.shape[0])
            out = torch.zeros(P, dtype=torch.uint8, device=positions.device)
            if P:
                view = _f32c(rs.viewmatrix.to(positions.device))
                proj = _f32c(rs.projmatrix.to(positions.device))
                check(_lib.lib().ogs_mark_visible(P, ptr(pos), ptr(view), ptr(proj), ptr(out), _stream()),
                      "ogs_mark_visible")
        return out.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        empty = torch.Tensor([])
        shs = empty if shs is None else shs
        colors_precomp = empty if colors_precomp is None else colors_precomp
        scales = empty if scales is None else scales
        rotations = empty if rotations is None else rotations
        cov3D_precomp = empty if cov3D_precomp is None else cov3D_precomp
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, rs)
