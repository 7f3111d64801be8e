"""Multi-view SAM mask refinement (utils/sam_refinement_utils.py ``MultiViewSAMMaskRefiner``) on batched footprint kernels.

Drop-in for the reference's class: ``MultiViewSAMMaskRefiner(verbose_logging=False).refine_sam_masks(cameras, sam_masks,
gaussians, sam_level=0)`` returns one entry per camera -- ``None`` where the input mask is ``None``, else the remapped
``[L, H, W]`` mask (same dtype and device) with level ``sam_level`` replaced by the expanded mask -- and sets
``camera.depth_map``.

The reference renders ONE Gaussian per rasterizer call for every (Gaussian, camera) pair that passes the visibility test and
post-processes a full frame each time.  A single white Gaussian on black has closed form, so here a pair is a walk over the
Gaussian's tile rectangle on the geometry state the camera's depth pass already left behind (include/ogs_refine.h); a camera
costs a few launches whatever the number of pairs:

  visit 1 (per camera)  depth pass (streaming path, keeps its geometry state) -> ``depth_map``; ogs_refine_visibility;
                        dominant ids of the stage-1 Gaussians on the ORIGINAL masks (ogs_refine_footprint_labels)
  host                  stage 1: the reference's sequential relabelling touches N / stage1_stride Gaussians and whole label
                        classes, never pixels: it runs on a per-camera table original id -> current id (``stage1_tables``),
                        followed by the consistent 1..n remap of all levels (``consistent_id_mapping``), applied once
  visit 2 (per camera)  dominant id and q_max of every visible pair on the REMAPPED masks
  one launch            ogs_refine_vote: each Gaussian's winner over its cameras (first-met tie rule)
  visit 3 (per camera)  ogs_refine_expand into the camera's [H, W, K] accumulator, ogs_refine_finalize

Not reproduced: ``camera.pixel_value_tensor`` / ``unique_ids`` / ``id_to_idx`` are not set (the accumulator lives for one
camera at a time), the rerun / matplotlib visualisation is not produced (``verbose_logging`` is accepted and ignored).
Cameras whose mask is ``None`` get a depth map and take no further part.  There is no CPU path.

Memory held across the visits, not chunked: the visibility matrix and the dominant ids of the vote, ``N x cameras x 5`` bytes
(1 M Gaussians x 300 cameras: 1.5 GB), and 13 bytes per visible pair; ``ogs_refine_vote`` compares a Gaussian's cameras pairwise
(cameras^2 per Gaussian).  Sized for the reference's use -- tens of cameras per call; split the camera list for more.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from . import rasterizer as R
from ._lib import check, ptr

NO_VOTE = -(1 << 31)            # OGS_REFINE_NO_VOTE
DEFER_LARGE, DEFER_TABLE = -2, -3
_BLOCK_SCRATCH_BYTES = 64 << 20  # global label tables of one ogs_refine_footprint_labels_block launch (K above its LDS table)


# ---- stage 1 on label classes (host, CPU-testable) ----------------------------------------------------------------------
def stage1_tables(level_ids, stage1_pairs, current_max_id=0):
    """The reference's ``sync_segment_ids`` loop (:1055-1115, :1177-1200) on tables instead of pixels.

    level_ids[c]: the ids present in camera c's original level mask (``None`` for a camera without mask).
    stage1_pairs: per stage-1 Gaussian, in processing order, its ``[(camera, dominant id on the ORIGINAL mask), ...]``.
    Returns (tables, current_max_id): tables[c] maps every original id of camera c to the id its pixels carry afterwards.

    Per Gaussian with at least one pair: a fresh id max(current_max_id, largest id > 0 in any current mask) + 1; for every
    pair whose id is not -1 and which some pixel of that camera CURRENTLY carries, all those pixels take the new id.  An id an
    earlier Gaussian already relabelled no longer matches (the dominant ids were taken on the original masks)."""
    tables = [None if ids is None else {int(i): int(i) for i in ids} for ids in level_ids]
    current = [None if t is None else {i: i for i in t} for t in tables]          # current id -> original id
    for pairs in stage1_pairs:
        if not pairs:
            continue
        for cur in current:
            if cur:
                top = max(cur)
                if top > 0:
                    current_max_id = max(current_max_id, top)
        current_max_id += 1
        new_id = current_max_id
        for cam, dom in pairs:
            cur = current[cam]
            if cur is None or dom == -1 or dom not in cur:
                continue
            orig = cur.pop(dom)
            cur[new_id] = orig
            tables[cam][orig] = new_id
    return tables, current_max_id


def consistent_id_mapping(ids):
    """``create_consistent_id_mapping`` (:25-80) on a set of ids: ids > 0 sorted -> 1..n, 0 and -1 kept; anything else the
    reference leaves at the 0 its ``zeros_like`` started from."""
    mapping = {old: new for new, old in enumerate(sorted({int(i) for i in ids if i > 0}), 1)}
    mapping[0] = 0
    mapping[-1] = -1
    return mapping


def _remap(mask_level: torch.Tensor, uniq: torch.Tensor, new_ids) -> torch.Tensor:
    table = torch.tensor(new_ids, dtype=mask_level.dtype, device=mask_level.device)
    return table[torch.bucketize(mask_level.contiguous(), uniq)]


def remap_masks(sam_masks, sam_level, tables):
    """Apply stage 1 and the consistent remap in one step: level `sam_level` of camera c goes through tables[c] and then the
    mapping, every other level through the mapping alone.  Returns (mapping, remapped masks)."""
    uniq, all_ids = {}, set()
    for c, mask in enumerate(sam_masks):
        if mask is None:
            continue
        for lvl in range(mask.shape[0]):
            u = torch.unique(mask[lvl])
            ids = [int(i) for i in u.tolist()]
            if lvl == sam_level:
                ids = [tables[c][i] for i in ids]
            uniq[c, lvl] = (u, ids)
            all_ids.update(ids)
    mapping = consistent_id_mapping(all_ids)
    refined = [None] * len(sam_masks)
    for c, mask in enumerate(sam_masks):
        if mask is None:
            continue
        out = torch.empty_like(mask)
        for lvl in range(mask.shape[0]):
            u, ids = uniq[c, lvl]
            out[lvl] = _remap(mask[lvl], u, [mapping.get(i, 0) for i in ids])
        refined[c] = out
    return mapping, refined


# ---- the drop-in ----------------------------------------------------------------------------------------------------------
class MultiViewSAMMaskRefiner:
    """Refines SAM masks by enforcing consistency across overlapping views (reference class of the same name)."""

    def __init__(self, verbose_logging=False):
        self.verbose_logging = verbose_logging      # accepted and ignored: no rerun / matplotlib output
        self.current_max_id = 0                     # as in the reference: survives from call to call
        self.keep_intermediates = False             # tests / diagnostics: leave every intermediate in self.last
        self.geom_cache_bytes = 1 << 30             # geometry states kept between the visits; beyond it they are recomputed
        self.stats: dict = {}
        self.last: dict = {}

    # -- per-camera pieces ----------------------------------------------------------------------------------------------
    def _model(self, gaussians):
        f = lambda t: t.detach().to(torch.float32).contiguous()
        m = {"xyz": f(gaussians.get_xyz), "opacity": f(gaussians.get_opacity), "scales": f(gaussians.get_scaling),
             "rotations": f(gaussians.get_rotation), "shs": f(gaussians.get_features),
             "sh_degree": int(gaussians.active_sh_degree)}
        R._require_gpu(m["xyz"], "gaussians.get_xyz")
        return m

    def _settings(self, camera, dev):
        return R.GaussianRasterizationSettings(
            image_height=int(camera.image_height), image_width=int(camera.image_width),
            tanfovx=math.tan(camera.FoVx * 0.5), tanfovy=math.tan(camera.FoVy * 0.5),
            bg=torch.zeros(3, dtype=torch.float32, device=dev), scale_modifier=1.0,
            viewmatrix=camera.world_view_transform, projmatrix=camera.full_proj_transform, sh_degree=self._sh_degree,
            campos=camera.camera_center, prefiltered=False, debug=False)

    def _pass_args(self, camera, m, outputs):
        dev = m["xyz"].device
        rs = self._settings(camera, dev)
        g = lambda t: R._f32c(t.to(dev))
        view, proj, campos = g(rs.viewmatrix), g(rs.projmatrix), g(rs.campos)
        keep = (rs.bg, view, proj, campos)
        a = R._fwd_args(rs, int(m["xyz"].shape[0]), 3, m["xyz"], m["shs"], None, m["opacity"], m["scales"], m["rotations"],
                        None, rs.bg, view, proj, campos, *outputs, None, 1)
        return a, keep

    def _depth_pass(self, camera, m):
        """The reference's full pass (:1125-1127: model SH, black background, scale 1) through the streaming path, whose
        geometry state -- the record rows the footprint kernels read -- is returned with the depth image."""
        dev = m["xyz"].device
        P, H, W = int(m["xyz"].shape[0]), int(camera.image_height), int(camera.image_width)
        if P == 0:
            return torch.zeros(1, H, W, dtype=torch.float32, device=dev), None
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        color, depth, alpha = e(3, H, W), e(1, H, W), e(1, H, W)
        radii = torch.empty(P, dtype=torch.int32, device=dev)
        a, keep = self._pass_args(camera, m, (color, depth, alpha, radii))
        geom = R._streaming_render(a, dev, _lib.lib(), False)[0]
        del keep
        return depth, geom

    def _geometry(self, camera, m):
        """The geometry phase alone: the same record rows as the depth pass of this camera left."""
        dev = m["xyz"].device
        P, H, W = int(m["xyz"].shape[0]), int(camera.image_height), int(camera.image_width)
        lib = _lib.lib()
        radii = torch.empty(P, dtype=torch.int32, device=dev)
        a, keep = self._pass_args(camera, m, (None, None, None, radii))
        gb, gtb, _ = R._geom_sizes(P, W, H, 3, 1)
        geom = torch.empty(gb, dtype=torch.uint8, device=dev)
        geom_tmp = torch.empty(gtb, dtype=torch.uint8, device=dev)
        a.geom_buffer, a.geom_tmp = ptr(geom), ptr(geom_tmp)
        check(lib.ogs_raster_forward_geometry(C.byref(a), R._stream(), None), "ogs_raster_forward_geometry")
        del keep
        return geom

    @staticmethod
    def _projection(camera, dev):
        """The two un-transposed matrices of project_3d_points_to_image_batch (:548-556), derived when the camera lacks them."""
        f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        wvt = f(camera.world_view_transform)
        view = getattr(camera, "world_view_transform_no_t", None)
        view = wvt.t().contiguous() if view is None else f(torch.as_tensor(view))
        proj = getattr(camera, "projection_matrix_no_t", None)
        if proj is None:
            pm = getattr(camera, "projection_matrix", None)
            if pm is None:      # full_proj_transform = world_view_transform @ projection_matrix
                pm = (torch.linalg.inv(wvt.double().cpu()) @ camera.full_proj_transform.detach().double().cpu()).float()
            proj = f(torch.as_tensor(pm)).t().contiguous()
        else:
            proj = f(torch.as_tensor(proj))
        return view, proj

    def _visibility(self, camera, m, depth, thr, dist):
        dev = m["xyz"].device
        P, H, W = int(m["xyz"].shape[0]), int(camera.image_height), int(camera.image_width)
        out = torch.zeros(P, dtype=torch.uint8, device=dev)
        view, proj = self._projection(camera, dev)
        campos = R._f32c(camera.camera_center.to(dev))
        cx = float(getattr(camera, "cx", W / 2.0))
        cy = float(getattr(camera, "cy", H / 2.0))
        check(_lib.lib().ogs_refine_visibility(P, ptr(m["xyz"]), ptr(view), ptr(proj), ptr(campos), W, H, cx, cy,
                                               ptr(depth), float(dist), float(thr), ptr(out), R._stream()),
              "ogs_refine_visibility")
        return out

    def _footprints(self, pairs, geom, W, H, lab, K):
        """(dominant label index or -1, q_max, walked by a workgroup) per pair; pairs the one-wave kernel defers -- large
        rectangles, more labels under the footprint than its table holds -- go through the workgroup kernel."""
        dev = pairs.device
        n = int(pairs.numel())
        dom = torch.empty(n, dtype=torch.int32, device=dev)
        qm = torch.empty(n, dtype=torch.int32, device=dev)
        large = torch.zeros(n, dtype=torch.bool, device=dev)
        if n == 0:
            return dom, qm, large
        lib, stream = _lib.lib(), R._stream()
        check(lib.ogs_refine_footprint_labels(n, ptr(pairs), ptr(geom), 3, W, H, ptr(lab), K, ptr(dom), ptr(qm), stream),
              "ogs_refine_footprint_labels")
        large = dom == DEFER_LARGE
        deferred = torch.nonzero(dom <= DEFER_LARGE).reshape(-1)
        m = int(deferred.numel())
        if m:
            self.stats["large_rect_pairs"] += int(large.sum().item())
            self.stats["slow_path_pairs"] += int((dom == DEFER_TABLE).sum().item())
            words = int(lib.ogs_refine_block_scratch_words(K))
            if words:
                self.stats["global_table_pairs"] += m
            rows = m if words == 0 else max(1, _BLOCK_SCRATCH_BYTES // (4 * words))
            for s in range(0, m, rows):
                part = deferred[s:s + rows]
                sub = pairs[part].contiguous()
                k = int(sub.numel())
                scratch = torch.zeros(k * words, dtype=torch.int32, device=dev) if words else None
                d = torch.empty(k, dtype=torch.int32, device=dev)
                q = torch.empty(k, dtype=torch.int32, device=dev)
                check(lib.ogs_refine_footprint_labels_block(k, ptr(sub), ptr(geom), 3, W, H, ptr(lab), K, ptr(scratch), ptr(d),
                                                            ptr(q), stream), "ogs_refine_footprint_labels_block")
                dom[part] = d
                qm[part] = q
                self.stats["block_launches"] += 1
        return dom, qm, large

    # -- the whole refinement -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def refine_sam_masks(self, cameras, sam_masks, gaussians, sam_level=0, *, stage1_stride=1000, stage1_opacity=0.99,
                         stage2_stride=1, depth_diff_threshold=0.15, dist_optical_center=0.1,
                         accumulated_weight_threshold=0.5):
        m = self._model(gaussians)
        self._sh_degree = m["sh_degree"]
        dev = m["xyz"].device
        lib = _lib.lib()
        N, ncam = int(m["xyz"].shape[0]), len(cameras)
        live = [c for c in range(ncam) if sam_masks[c] is not None]
        given = sam_masks
        sam_masks = [None if t is None else t.to(dev) for t in given]      # results go back to each mask's own device
        self.stats = {"pairs": 0, "stage1_pairs": 0, "expand_pairs": 0, "large_rect_pairs": 0, "slow_path_pairs": 0,
                      "accumulator_bytes": 0, "geometry_recomputed": 0, "global_table_pairs": 0, "block_launches": 0,
                      "large_rect_expand_pairs": 0}
        keep = self.keep_intermediates
        self.last = {}

        # ---- visit 1: depth maps, visibility, stage-1 dominant ids on the original masks --------------------------------
        hi = torch.nonzero(m["opacity"].reshape(-1) >= stage1_opacity).reshape(-1)
        s1 = hi[::int(stage1_stride)].to(torch.int32)                    # the stage-1 Gaussians, in processing order
        vis = torch.zeros(N, ncam, dtype=torch.bool, device=dev)
        geoms, cached = {}, 0
        s1_dom = torch.full((int(s1.numel()), ncam), NO_VOTE, dtype=torch.int64, device=dev)
        orig_uniq = [None] * ncam
        for c, camera in enumerate(cameras):
            depth, geom = self._depth_pass(camera, m)
            camera.depth_map = depth
            if c not in live or N == 0:
                continue
            H, W = int(camera.image_height), int(camera.image_width)
            v = self._visibility(camera, m, depth, depth_diff_threshold, dist_optical_center)
            vis[:, c] = v != 0
            uniq, inv = torch.unique(sam_masks[c][sam_level], return_inverse=True)
            orig_uniq[c] = uniq
            rows = torch.nonzero(v[s1.long()] != 0).reshape(-1)
            pairs = s1[rows].contiguous()
            dom, qm, _ = self._footprints(pairs, geom, W, H, inv.to(torch.int32).contiguous(), int(uniq.numel()))
            ok = qm > 0
            s1_dom[rows[ok], c] = uniq[dom[ok].long()].to(torch.int64)
            self.stats["stage1_pairs"] += int(pairs.numel())
            if cached + geom.numel() <= self.geom_cache_bytes:
                geoms[c] = geom
                cached += geom.numel()

        # ---- stage 1 on the host: label classes, not pixels ---------------------------------------------------------------
        s1_host = s1_dom.cpu().tolist()
        stage1_pairs = [[(c, row[c]) for c in live if row[c] != NO_VOTE] for row in s1_host]
        tables, self.current_max_id = stage1_tables(
            [None if u is None else u.tolist() for u in orig_uniq], stage1_pairs, self.current_max_id)
        mapping, refined = remap_masks(sam_masks, sam_level, tables)

        # ---- visit 2: dominant id and q_max of every visible pair on the remapped masks ---------------------------------
        dom_ids = torch.full((N, max(len(live), 1)), NO_VOTE, dtype=torch.int32, device=dev)
        in_stage2 = torch.zeros(N, dtype=torch.bool, device=dev)
        in_stage2[::int(stage2_stride)] = True
        state = {}
        for j, c in enumerate(live):
            camera = cameras[c]
            H, W = int(camera.image_height), int(camera.image_width)
            geom = geoms.get(c)
            if geom is None and N:
                geom = self._geometry(camera, m)
                self.stats["geometry_recomputed"] += 1
            uniq, inv = torch.unique(refined[c][sam_level], return_inverse=True)
            lab = inv.to(torch.int32).contiguous()
            pairs = torch.nonzero(vis[:, c] & in_stage2).reshape(-1).to(torch.int32)
            dom, qm, large = self._footprints(pairs, geom, W, H, lab, int(uniq.numel()))
            ok = qm > 0
            ids32 = uniq.to(torch.int32)
            dom_ids[pairs[ok].long(), j] = ids32[dom[ok].long()]
            state[c] = (pairs, dom, qm, large, lab, uniq, ids32)
            self.stats["pairs"] += int(pairs.numel())

        # ---- the vote ---------------------------------------------------------------------------------------------------
        winner = torch.full((N,), NO_VOTE, dtype=torch.int32, device=dev)
        if N and live:
            check(lib.ogs_refine_vote(N, len(live), ptr(dom_ids), ptr(winner), R._stream()), "ogs_refine_vote")

        # ---- visit 3: expansion and the per-pixel decision, one accumulator in flight -----------------------------------
        expanded = [None] * ncam
        if keep:
            self.last = {"visibility": vis, "stage1_gaussians": s1, "stage1_pairs": stage1_pairs, "id_mapping": mapping,
                         "refined_masks": refined, "live": live, "dominant": dom_ids, "winners": winner, "q_max": {},
                         "accumulators": {}, "base": {}, "unique_ids": {}}
        for j, c in enumerate(live):
            camera = cameras[c]
            H, W = int(camera.image_height), int(camera.image_width)
            pairs, dom, qm, large, lab, uniq, ids32 = state.pop(c)
            K = int(uniq.numel())
            geom = geoms.pop(c, None)
            if geom is None and N:
                geom = self._geometry(camera, m)
                self.stats["geometry_recomputed"] += 1
            acc = torch.zeros(H, W, K, dtype=torch.float32, device=dev)
            base = torch.zeros(K, dtype=torch.int32, device=dev)
            self.stats["accumulator_bytes"] = max(self.stats["accumulator_bytes"], acc.numel() * 4)
            sel = qm > 0
            sel[sel.clone()] = ids32[dom[sel].long()] == winner[pairs[sel].long()]
            for block, part in ((0, sel & ~large), (1, sel & large)):
                p = pairs[part].contiguous()
                n = int(p.numel())
                if n == 0:
                    continue
                w, q = dom[part].contiguous(), qm[part].contiguous()
                check(lib.ogs_refine_expand(n, ptr(p), ptr(w), ptr(q), ptr(geom), 3, W, H, ptr(lab), K, ptr(acc), ptr(base),
                                            block, R._stream()), "ogs_refine_expand")
                self.stats["expand_pairs"] += n
                self.stats["large_rect_expand_pairs"] += n * block
            void = torch.nonzero(uniq == -1).reshape(-1)
            void_index = int(void[0].item()) if void.numel() else -1
            idx = torch.empty(H, W, dtype=torch.int32, device=dev)
            check(lib.ogs_refine_finalize(H * W, K, ptr(lab), ptr(acc), ptr(base), void_index,
                                          float(accumulated_weight_threshold), ptr(idx), R._stream()), "ogs_refine_finalize")
            ids = uniq[idx.clamp_min(0).long()]
            ids[idx < 0] = -1
            out = refined[c].clone()
            out[sam_level] = ids.to(out.dtype)
            expanded[c] = out.to(given[c].device)
            if keep:
                qfull = torch.zeros(N, dtype=torch.int32, device=dev)
                qfull[pairs.long()] = qm
                self.last["q_max"][c], self.last["accumulators"][c] = qfull, acc
                self.last["base"][c], self.last["unique_ids"][c] = base, uniq
        return expanded
