"""The scene of the SAM-refinement tests, shared by the fixture generator (make_sam_refine_golden.py), the host tests and the
GPU tests: 3 general-pose cameras at 48 x 40 (not a multiple of the 16-px tile, W != H), one with an off-centre principal
point, 4 mask levels whose ids include -1 and 0, and ~1100 Gaussians of which more than 1001 have opacity >= 0.99 (two stage-1
Gaussians at the reference's stride of 1000).  The special cases come FIRST in the arrays so that a cut to the first 64 keeps
them: a disc covering the whole image, near-transparent Gaussians (opacity 0.003: every q is 0), centres behind the cameras,
centres off-screen; occluded centres, footprints clipped by the image edge and footprints inside one label follow from the
layout.  Everything is drawn from a seeded CPU generator."""
import math

import numpy as np
import torch

W, H, FOCAL = 48, 40, 40.0
N_FULL = 1100
SAM_LEVEL = 0
SEED = 5


class Model:
    """what refine_sam_masks reads of a GaussianModel"""
    active_sh_degree = 3

    def __init__(self, xyz, opacity, scaling, rotation, features):
        self.get_xyz, self.get_opacity, self.get_scaling = xyz, opacity, scaling
        self.get_rotation, self.get_features = rotation, features

    def _map(self, f):
        return Model(*(f(t) for t in (self.get_xyz, self.get_opacity, self.get_scaling, self.get_rotation, self.get_features)))

    def to(self, device):
        return self._map(lambda t: t.to(device))

    def cut(self, n):
        return self._map(lambda t: t[:n].clone())


class Camera:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def to(self, device):
        return Camera(**{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in self.__dict__.items()
                         if k != "depth_map"})


def _projection(znear, zfar, fovx, fovy):
    tx, ty = math.tan(fovx / 2), math.tan(fovy / 2)
    P = torch.zeros(4, 4)
    P[0, 0], P[1, 1], P[3, 2] = 1.0 / tx, 1.0 / ty, 1.0
    P[2, 2], P[2, 3] = zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
    return P


def _rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def make_camera(width, height, focal, eye, roll, principal=None, full=True, look_away=False):
    """a camera at `eye` looking at the world origin (look_away: with its back to it), rolled about its axis; full=False
    leaves out the attributes the product derives when absent (the two un-transposed matrices, cx, cy)"""
    eye = np.asarray(eye, np.float64)
    fwd = (eye if look_away else -eye) / np.linalg.norm(eye)
    right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = _rodrigues((0, 0, 1), roll) @ np.stack([right, down, fwd])        # rows: camera axes in the world
    w2c = torch.eye(4)
    w2c[:3, :3] = torch.tensor(R, dtype=torch.float32)
    w2c[:3, 3] = torch.tensor(-R @ eye, dtype=torch.float32)
    fovx, fovy = 2 * math.atan(width / (2 * focal)), 2 * math.atan(height / (2 * focal))
    proj = _projection(0.01, 100.0, fovx, fovy)
    wvt = w2c.t().contiguous()
    kw = dict(image_width=width, image_height=height, FoVx=fovx, FoVy=fovy, world_view_transform=wvt,
              full_proj_transform=(wvt @ proj.t()).contiguous(), camera_center=torch.linalg.inv(wvt)[3, :3].contiguous())
    if full:
        cx, cy = principal if principal is not None else (width / 2.0, height / 2.0)
        kw.update(world_view_transform_no_t=w2c.contiguous(), projection_matrix_no_t=proj.contiguous(), cx=cx, cy=cy)
    return Camera(**kw)


EYES = ((0.3, -0.2, -4.0), (1.7, 0.4, -3.6), (-1.5, -0.7, -3.7))
ROLLS = (0.0, 0.35, -0.6)


def cameras(width=W, height=H, focal=FOCAL, full=True):
    principal = (None, (width / 2.0 + 1.5, height / 2.0 - 1.0), None)
    return [make_camera(width, height, focal, e, r, p, full) for e, r, p in zip(EYES, ROLLS, principal)]


def masks(width=W, height=H, seed=SEED, block=(10, 12), void=(10, 12)):
    """per camera an int64 [4, H, W] stack of block-structured id images; every camera numbers its segments on its own.  The
    void id -1 fills the top-left `void` patch of every level (a void pixel nothing expands into has all channels at 0)."""
    g = torch.Generator().manual_seed(1000 + seed)
    out = []
    for c in range(3):
        levels = []
        for lvl in range(4):
            bh, bw = block[0] * (1 + lvl // 2), block[1] * (1 + lvl % 2)
            ny, nx = -(-height // bh), -(-width // bw)
            pool = torch.tensor([0] + list(range(3 + 40 * lvl + 5 * c, 3 + 40 * lvl + 5 * c + 3 * 12, 3)))
            ids = pool[torch.randint(0, pool.numel(), (ny, nx), generator=g)]
            ids[-1, -1] = 0                                         # both special ids are present in every level
            level = ids.repeat_interleave(bh, 0).repeat_interleave(bw, 1)[:height, :width].clone()
            level[:void[0], :void[1]] = -1
            levels.append(level)
        out.append(torch.stack(levels).to(torch.int64).contiguous())
    return out


def model(n=N_FULL, seed=SEED):
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)
    xyz = torch.stack([rand(n) * 3.0 - 1.5, rand(n) * 2.4 - 1.2, rand(n) * 0.5 - 0.25], dim=1)
    scaling = torch.exp(torch.randn(n, 3, generator=g) * 0.4 - 2.4)
    q = torch.randn(n, 4, generator=g)
    rotation = q / q.norm(dim=1, keepdim=True)
    opacity = 0.99 + 0.009 * rand(n, 1)
    soft = torch.arange(n) % 12 == 5                                # every 12th: an ordinary translucent Gaussian
    opacity[soft] = torch.sigmoid(torch.randn(int(soft.sum()), 1, generator=g))
    # ---- the special cases, first in the arrays ----
    # 0: a disc BEHIND everything whose footprint covers the whole image in every camera; the others keep clear of the lines
    #    of sight to its centre, so that it passes the depth test there
    centre = torch.tensor([0.1, -0.1])
    d = xyz[:, :2] - centre
    r = d.norm(dim=1, keepdim=True).clamp_min(1e-3)
    xyz[:, :2] = torch.where(r < 0.55, centre + d / r * (0.55 + 0.2 * rand(n, 1)), xyz[:, :2])
    xyz[0] = torch.tensor([0.1, -0.1, 0.3]); scaling[0] = torch.tensor([3.0, 3.0, 0.002])
    rotation[0] = torch.tensor([1.0, 0.0, 0.0, 0.0]); opacity[0] = 0.995
    # 1..5: near-transparent (alpha < 1/255 everywhere) just in front of the disc, in the clearing
    for i in range(1, 6):
        xyz[i] = torch.tensor([0.1 + 0.05 * (i - 3), -0.1 + 0.04 * (3 - i), 0.3 - 0.015 * i])
        opacity[i] = 0.003
    # 6..8: behind the cameras; 9..11: far off-screen
    xyz[6:9] = torch.tensor([[0.0, 0.0, -6.0], [2.5, 0.5, -5.5], [-2.0, -1.0, -5.8]])
    xyz[9:12] = torch.tensor([[6.0, 0.0, 0.0], [-6.5, 1.0, 0.1], [0.5, 5.5, -0.1]])
    features = torch.cat([0.5 * torch.randn(n, 1, 3, generator=g), 0.1 * torch.randn(n, 15, 3, generator=g)], dim=1)
    return Model(xyz.contiguous(), opacity.contiguous(), scaling.contiguous(), rotation.contiguous(), features.contiguous())


WHITE = torch.cat([torch.ones(1, 1, 3), torch.zeros(1, 15, 3)], dim=1)


def _pass_inputs(camera, mdl, indices, white):
    sel = (lambda t: t) if indices is None else (lambda t: t[indices])
    shs = WHITE.to(mdl.get_xyz.device).expand(len(indices), 16, 3).contiguous() if white else sel(mdl.get_features)
    return sel(mdl.get_xyz), sel(mdl.get_opacity), sel(mdl.get_scaling), sel(mdl.get_rotation), shs


def oracle_rasterize(mdl):
    """rasterize(camera, indices, white_sh) of tests/refine_restatement.py on the CPU oracle"""
    from oracle import raster_oracle as ro

    def rasterize(camera, indices, white):
        xyz, opacity, scaling, rotation, shs = (t.detach().float().contiguous().numpy()
                                                for t in _pass_inputs(camera, mdl, indices, white))
        ref = ro.render_forward(W=int(camera.image_width), H=int(camera.image_height), tanfovx=math.tan(camera.FoVx * 0.5),
                                tanfovy=math.tan(camera.FoVy * 0.5), bg=np.zeros(3, np.float32), scale_modifier=1.0,
                                sh_degree=mdl.active_sh_degree, means3D=xyz, opacities=opacity,
                                viewmatrix=camera.world_view_transform.numpy(), projmatrix=camera.full_proj_transform.numpy(),
                                campos=camera.camera_center.numpy(), scales=scaling, rotations=rotation, shs=shs)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        return t(ref["color"]), t(ref["depth"])
    return rasterize


def hip_rasterize(mdl):
    """the same on this library's drop-in GaussianRasterizer: P = 1 calls take the tiny pass, as under the reference's loop"""
    from opengaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    dev = mdl.get_xyz.device

    def rasterize(camera, indices, white):
        xyz, opacity, scaling, rotation, shs = _pass_inputs(camera, mdl, indices, white)
        rs = GaussianRasterizationSettings(
            image_height=int(camera.image_height), image_width=int(camera.image_width), tanfovx=math.tan(camera.FoVx * 0.5),
            tanfovy=math.tan(camera.FoVy * 0.5), bg=torch.zeros(3, device=dev), scale_modifier=1.0,
            viewmatrix=camera.world_view_transform, projmatrix=camera.full_proj_transform, sh_degree=mdl.active_sh_degree,
            campos=camera.camera_center, prefiltered=False, debug=False)
        with torch.no_grad():
            color, _, depth, _ = GaussianRasterizer(rs)(means3D=xyz, means2D=torch.zeros_like(xyz), shs=shs, opacities=opacity,
                                                         scales=scaling, rotations=rotation)
        return color, depth
    return rasterize


# ---- the inputs as stored in sam_refine_golden.npz ---------------------------------------------------------------------------
_MODEL_FIELDS = ("get_xyz", "get_opacity", "get_scaling", "get_rotation", "get_features")
_CAMERA_TENSORS = ("world_view_transform", "full_proj_transform", "camera_center", "world_view_transform_no_t",
                   "projection_matrix_no_t")
_CAMERA_SCALARS = ("image_width", "image_height", "FoVx", "FoVy", "cx", "cy")


def pack_inputs(mdl, cams, sam_masks):
    store = {f"input/model/{f}": getattr(mdl, f).numpy() for f in _MODEL_FIELDS}
    for c, (cam, mask) in enumerate(zip(cams, sam_masks)):
        store[f"input/mask/{c}"] = mask.numpy().astype(np.int16)
        for f in _CAMERA_TENSORS:
            store[f"input/camera/{c}/{f}"] = getattr(cam, f).numpy()
        store[f"input/camera/{c}/scalars"] = np.array([getattr(cam, f) for f in _CAMERA_SCALARS], np.float64)
    return store


def unpack_inputs(npz, ncam=3):
    mdl = Model(*(torch.from_numpy(npz[f"input/model/{f}"]) for f in _MODEL_FIELDS))
    cams, sam_masks = [], []
    for c in range(ncam):
        kw = {f: torch.from_numpy(npz[f"input/camera/{c}/{f}"]) for f in _CAMERA_TENSORS}
        sc = npz[f"input/camera/{c}/scalars"]
        kw.update(image_width=int(sc[0]), image_height=int(sc[1]), FoVx=float(sc[2]), FoVy=float(sc[3]), cx=float(sc[4]),
                  cy=float(sc[5]))
        cams.append(Camera(**kw))
        sam_masks.append(torch.from_numpy(npz[f"input/mask/{c}"].astype(np.int64)))
    return mdl, cams, sam_masks
