"""Test infrastructure: a plain torch / NumPy restatement of the multi-view SAM mask refinement, one rasterizer call per
(Gaussian, camera) pair as the reference issues them (utils/sam_refinement_utils.py:1118-1318).  Written from the semantics
listed in opengaussian_amd/sam_refine.py and include/ogs_refine.h; nothing of the product is imported.

``rasterize(camera, indices, white_sh)`` renders the Gaussians ``indices`` (a list of ints, or ``None`` for the whole model)
with the model's own SH (``white_sh=False``) or the view-independent white SH (DC = 1, rest 0), black background, scale 1,
and returns ``(image [3, H, W], depth [1, H, W])``.  Everything else happens here, on the device of the masks.

``refine`` returns every intermediate; the loops keep the reference's order of floating-point additions.
"""
import numpy as np
import torch

NO_VOTE = -(1 << 31)


def camera_matrices(camera):
    """the un-transposed world-to-camera and projection matrices"""
    wvt = camera.world_view_transform.detach().float()
    view = getattr(camera, "world_view_transform_no_t", None)
    view = wvt.t() if view is None else view.detach().float()
    proj = getattr(camera, "projection_matrix_no_t", None)
    if proj is None:
        pm = getattr(camera, "projection_matrix", None)
        if pm is None:
            pm = (torch.linalg.inv(wvt.double().cpu()) @ camera.full_proj_transform.detach().double().cpu()).float()
        proj = pm.detach().float().t()
    return view.contiguous(), proj.detach().float().contiguous()


def visibility(camera, xyz, depth_map, depth_diff_threshold=0.15, dist_optical_center=0.1):
    """(visible [N] bool, margin [N]): margin = distance of the depth test from its threshold (inf where it is not reached)."""
    dev = xyz.device
    W, H = int(camera.image_width), int(camera.image_height)
    view, proj = (t.to(dev) for t in camera_matrices(camera))
    hom = torch.cat([xyz, torch.ones(xyz.shape[0], 1, device=dev)], dim=1)
    pc = (view @ hom.T).T
    clip = (proj @ pc.T).T
    w = clip[:, 3]
    w = torch.where(torch.abs(w) < 1e-8, torch.sign(w) * 1e-8, w)
    ndc = clip / w.unsqueeze(1)
    u = ndc[:, 0] * (W / 2.0) + float(getattr(camera, "cx", W / 2.0))
    v = ndc[:, 1] * (H / 2.0) + float(getattr(camera, "cy", H / 2.0))
    vis = (pc[:, 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    ui = torch.where(vis, u, torch.zeros_like(u)).cpu().numpy().astype(int)
    vi = torch.where(vis, v, torch.zeros_like(v)).cpu().numpy().astype(int)
    centre = np.linalg.inv(view.cpu().numpy())[:3, 3]
    dist = np.linalg.norm(xyz.cpu().numpy() - centre, axis=1) - dist_optical_center
    rendered = depth_map[0][torch.from_numpy(vi).to(dev), torch.from_numpy(ui).to(dev)]
    diff = torch.abs(torch.from_numpy(dist).to(dev) - rendered)
    margin = torch.where(vis, torch.abs(diff - depth_diff_threshold), torch.full_like(diff, float("inf")))
    return vis & (diff < depth_diff_threshold), margin


def footprint(image):
    """(q [H, W] uint8, weight [H, W] float): the uint8 frame and the weight map normalised to a maximum of 1."""
    q = torch.clamp(image.permute(1, 2, 0) * 255, 0, 255).to(torch.uint8)
    weight = torch.mean(q.float() / 255.0, dim=2)
    top = weight.max()
    if top > 0:
        weight = weight / top
    return q[:, :, 0], weight, bool(torch.any(q != 0))


def dominant_id(mask, weight):
    """the id with the largest weight sum (lowest id on ties); a one-id image returns that id"""
    flat = mask.flatten()
    lo, hi = int(flat.min()), int(flat.max())
    if lo == hi:
        return lo
    off = -lo if lo < 0 else 0
    sums = torch.bincount((flat + off).long(), weights=weight.flatten(), minlength=hi + off + 1)
    return int(torch.argmax(sums)) - off


def q_gap(mask, q):
    """top minus second integer label sum of q (fragility measure; a one-label footprint has the whole sum as its gap)"""
    ids, inv = torch.unique(mask.flatten(), return_inverse=True)
    sums = torch.zeros(ids.numel(), dtype=torch.int64, device=mask.device).index_add_(0, inv, q.flatten().long())
    top = torch.sort(sums, descending=True).values
    return int(top[0] - top[1]) if top.numel() > 1 else int(top[0])


def consistent_ids(masks):
    ids = set()
    for m in masks:
        if m is not None:
            ids.update(int(i) for i in torch.unique(m).cpu().tolist())
    mapping = {old: new for new, old in enumerate(sorted(i for i in ids if i > 0), 1)}
    mapping[0] = 0
    mapping[-1] = -1
    out = []
    for m in masks:
        if m is None:
            out.append(None)
            continue
        r = torch.zeros_like(m)
        for old, new in mapping.items():
            r[m == old] = new
        out.append(r)
    return mapping, out


def refine(cameras, sam_masks, gaussians, rasterize, sam_level=0, stage1_stride=1000, stage1_opacity=0.99, stage2_stride=1,
           depth_diff_threshold=0.15, dist_optical_center=0.1, accumulated_weight_threshold=0.5, current_max_id=0):
    xyz = gaussians.get_xyz.detach()
    dev = xyz.device
    N, ncam = int(xyz.shape[0]), len(cameras)
    live = [c for c in range(ncam) if sam_masks[c] is not None]
    refined = [None if m is None else m.clone() for m in sam_masks]
    res = {"live": live}

    # depth maps and visibility
    depth_maps = [rasterize(camera, None, False)[1] for camera in cameras]
    vis = torch.zeros(N, ncam, dtype=torch.bool, device=dev)
    margin = torch.full((N, ncam), float("inf"), device=dev)
    for c in live:
        vis[:, c], margin[:, c] = visibility(cameras[c], xyz, depth_maps[c], depth_diff_threshold, dist_optical_center)
    res.update(depth_maps=depth_maps, visibility=vis, depth_margin=margin)

    def pair(c, g, mask):
        image, _ = rasterize(cameras[c], [g], True)
        q, weight, seen = footprint(image)
        return (dominant_id(mask, weight) if seen else None), q, weight

    # stage 1: cross-view consistent ids from the opaque Gaussians, one after the other
    opaque = torch.where(gaussians.get_opacity.detach() >= stage1_opacity)[0].cpu().tolist()
    stage1 = opaque[::stage1_stride]
    stage1_pairs = []
    for g in stage1:
        pairs = []
        for c in live:
            if vis[g, c]:
                dom, _, _ = pair(c, g, sam_masks[c][sam_level])
                if dom is not None:
                    pairs.append((c, dom))
        stage1_pairs.append(pairs)
        if not pairs:
            continue
        for m in refined:
            if m is not None:
                ids = torch.unique(m[sam_level])
                ids = ids[ids > 0]
                if ids.numel():
                    current_max_id = max(current_max_id, int(ids.max()))
        current_max_id += 1
        refined = [None if m is None else m.clone() for m in refined]
        for c, dom in pairs:
            hit = refined[c][sam_level] == dom
            if int(hit.sum()) > 0 and dom != -1:
                refined[c][sam_level][hit] = current_max_id
    res.update(stage1_gaussians=stage1, stage1_pairs=stage1_pairs, stage1_masks=refined, current_max_id=current_max_id)
    mapping, refined = consistent_ids(refined)
    res.update(id_mapping=mapping, refined_masks=refined)

    # stage 2: per-camera channels, votes, expansion
    uniq, chan = {}, {}
    for c in live:
        level = refined[c][sam_level]
        uniq[c] = torch.unique(level, sorted=True)
        chan[c] = torch.zeros(*level.shape, uniq[c].numel(), dtype=torch.float32, device=dev)
        for k, i in enumerate(uniq[c].tolist()):
            if i != -1:
                chan[c][..., k][level == i] = 1.0
    base = {c: torch.zeros(uniq[c].numel(), dtype=torch.int64, device=dev) for c in live}
    extra = {c: torch.zeros_like(chan[c]) for c in live}          # the weights alone (what the product's accumulator holds)
    dom_all = torch.full((N, ncam), NO_VOTE, dtype=torch.int64)
    qmax_all = torch.zeros(N, ncam, dtype=torch.int64)
    gap_all = torch.zeros(N, ncam, dtype=torch.int64)
    winners = torch.full((N,), NO_VOTE, dtype=torch.int64)
    for g in range(0, N, stage2_stride):
        found = []
        for c in live:
            if vis[g, c]:
                level = refined[c][sam_level]
                dom, q, weight = pair(c, g, level)
                qmax_all[g, c] = int(q.max())
                if dom is None:
                    continue
                dom_all[g, c], gap_all[g, c] = dom, q_gap(level, q)
                found.append((c, dom, weight))
        votes = {}
        for _, dom, _ in found:
            votes[dom] = votes.get(dom, 0) + 1
        if not votes:
            continue
        win = max(votes, key=votes.get)                            # the id met first keeps a tie
        winners[g] = win
        for c, dom, weight in found:
            if dom != win:
                continue
            k = uniq[c].tolist().index(win)
            own = refined[c][sam_level] == win
            chan[c][..., k][own] += 1.0
            base[c][k] += 1
            grow = (weight > 0) & ~own
            chan[c][..., k][grow] += weight[grow]
            extra[c][..., k][grow] += weight[grow]
    final = [None if m is None else m.clone() for m in refined]
    top2 = {}
    for c in live:
        best, arg = torch.max(chan[c], dim=2)
        # lowest channel among equals, whatever torch.max picks
        arg = torch.argmax((chan[c] == best.unsqueeze(2)).to(torch.uint8), dim=2)
        ids = uniq[c][arg]
        ids[best < accumulated_weight_threshold] = -1
        final[c][sam_level] = ids
        srt = torch.sort(chan[c], dim=2, descending=True).values
        second = srt[..., 1] if srt.shape[2] > 1 else torch.full_like(best, -float("inf"))
        top2[c] = (best, second)
    res.update(unique_ids=uniq, channels=chan, accumulators=extra, base=base, dominant=dom_all, q_max=qmax_all,
               q_gap=gap_all, winners=winners, final_masks=final, top2=top2)
    return res
