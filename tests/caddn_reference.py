"""Torch-CPU restatement of the reference's CaDDN statements, dtype-generic so that it runs in float64: the transforms (utils/transform_utils.py:14-91
with the two kornia conversions, scale = where(|z| > 1e-8, 1 / (z + 1e-8), 1)), FrustumGridGenerator (f2v/frustum_grid_generator.py:79-145),
DepthFFN.create_frustum_features (ffn/depth_ffn.py:70-92), the 5-D F.grid_sample(bilinear, zeros, align_corners=True) on the materialised volume
(f2v/sampler.py), DDNLoss / Balancer / compute_fg_mask (ffn/ddn_loss/, utils/loss_utils.py:235-261, kornia's softmax focal loss).  Plus the seeded
cases of tests/test_frustum_sample.py, the error allowance, and the mask of voxels no fp32 result can be held to.

Allowance.  Per case E32 = max |float32 CPU run of this restatement - its float64 run|.  The kernel's forward may differ from float64 by
FWD_FACTOR * E32: it factors the product, and forms the scene matrix in another order than torch's batched matmul.  Each gradient may differ from
float64 autograd by GRAD_FACTOR * its own E32: the sums have hundreds of terms in another order.  Nothing here reads the code under test.

Mask.  Non-finite grid components become -2, a jump: a voxel whose float64 LID radicand 1 + 8 (d - d_min) / bin, camera z or projective z' is within
MASK_EPS of zero may fall on either side in fp32.  A case may lose at most MASK_CAP of its voxels this way, a gradient case none."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

FWD_FACTOR = 8.0
GRAD_FACTOR = 16.0
MASK_EPS = 1e-3
MASK_CAP = 0.005


# ---------------------------------------------------------------------------------------------------------------- transforms
def to_homogeneous(points):
    return F.pad(points, [0, 1], "constant", 1.0)


def from_homogeneous(points, eps=1e-8):
    z = points[..., -1:]
    scale = torch.where(torch.abs(z) > eps, 1.0 / (z + eps), torch.ones_like(z))
    return scale * points[..., :-1]


def transform_points(trans, points):
    hom = torch.matmul(trans.unsqueeze(-3), to_homogeneous(points).unsqueeze(-1)).squeeze(-1)
    return from_homogeneous(hom), hom


def project_to_image(project, points):
    project = project.unsqueeze(1)
    points_t = (project @ to_homogeneous(points).unsqueeze(-1)).squeeze(-1)
    return from_homogeneous(points_t), points_t[..., -1] - project[..., 2, 3], points_t[..., -1]


def normalize_coords(coords, shape):
    shape = torch.flip(shape, dims=[0])
    return coords / (shape - 1) * 2 + -1


def lid_radicand(depth_map, depth_min, depth_max, num_bins):
    bin_size = 2 * (depth_max - depth_min) / (num_bins * (1 + num_bins))
    return 1 + 8 * (depth_map - depth_min) / bin_size


def bin_depths(depth_map, mode, depth_min, depth_max, num_bins, target=False):
    if mode == "UD":
        indices = (depth_map - depth_min) / ((depth_max - depth_min) / num_bins)
    elif mode == "LID":
        indices = -0.5 + 0.5 * torch.sqrt(lid_radicand(depth_map, depth_min, depth_max, num_bins))
    elif mode == "SID":
        indices = num_bins * (torch.log(1 + depth_map) - math.log(1 + depth_min)) / (math.log(1 + depth_max) - math.log(1 + depth_min))
    else:
        raise NotImplementedError(mode)
    if target:
        mask = (indices < 0) | (indices > num_bins) | (~torch.isfinite(indices))
        indices = indices.clone()
        indices[mask] = num_bins
        indices = indices.type(torch.int64)
    return indices


# ---------------------------------------------------------------------------------------------------------------- grid, volume, sampling
def frustum_grid(lidar_to_cam, cam_to_img, image_shape, grid_size, pc_range, disc, dtype, with_mask=False):
    """(B, X, Y, Z, 3) normalised grid in `dtype`; with_mask: also the (B, X, Y, Z) mask of voxels next to the NaN -> -2 jump"""
    X, Y, Z = grid_size
    B = lidar_to_cam.shape[0]
    gs = torch.as_tensor([X, Y, Z], dtype=dtype)
    rng = torch.as_tensor(pc_range, dtype=dtype).reshape(2, 3)
    voxel_size = (rng[1] - rng[0]) / gs
    grid_to_lidar = torch.eye(4, dtype=dtype)
    grid_to_lidar[:3, :3] = torch.diag(voxel_size)
    grid_to_lidar[:3, 3] = rng[0]
    axes = [torch.arange(n, dtype=dtype) for n in (X, Y, Z)]
    voxel_grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).unsqueeze(0) + 0.5          # (1, X, Y, Z, 3): voxel centres
    trans = (lidar_to_cam.to(dtype) @ grid_to_lidar).reshape(B, 1, 1, 4, 4)
    camera_grid, camera_hom = transform_points(trans, voxel_grid.repeat_interleave(B, dim=0))
    image_grid, image_depths, proj_z = project_to_image(cam_to_img.to(dtype).reshape(B, 1, 1, 3, 4), camera_grid)
    bins = bin_depths(image_depths, **disc)
    grid = torch.cat((image_grid, bins.unsqueeze(-1)), dim=-1)
    shape_max, _ = torch.max(image_shape, dim=0)
    frustum_shape = torch.cat((torch.tensor([disc["num_bins"]], dtype=shape_max.dtype), shape_max))
    grid = normalize_coords(grid, frustum_shape)
    grid = torch.where(torch.isfinite(grid), grid, torch.full_like(grid, -2))
    if not with_mask:
        return grid
    near = (camera_grid[..., 2].abs() < MASK_EPS) | (camera_hom[..., 3].abs() < MASK_EPS) | (proj_z.abs() < MASK_EPS)
    if disc["mode"] == "LID":
        near |= lid_radicand(image_depths, disc["depth_min"], disc["depth_max"], disc["num_bins"]).abs() < MASK_EPS
    return grid, near


def frustum_from_probs(image_features, depth_probs):
    """(B, C, H, W) x (B, D + 1, H, W) -> (B, C, D, H, W): the last bin dropped"""
    return depth_probs.unsqueeze(1)[:, :, :-1] * image_features.unsqueeze(2)


def create_frustum_features(image_features, depth_logits):
    return frustum_from_probs(image_features, F.softmax(depth_logits, dim=1))


def sample(frustum_features, grid):
    """(B, C, D, H, W), (B, X, Y, Z, 3) -> (B, C, Z, Y, X)"""
    out = F.grid_sample(frustum_features, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    return out.permute(0, 1, 4, 3, 2)


# ---------------------------------------------------------------------------------------------------------------- depth loss
def compute_fg_mask(gt_boxes2d, shape, downsample_factor=1):
    fg_mask = torch.zeros(shape, dtype=torch.bool)
    boxes = gt_boxes2d.clone() / downsample_factor
    boxes[:, :, :2] = torch.floor(boxes[:, :, :2])
    boxes[:, :, 2:] = torch.ceil(boxes[:, :, 2:])
    boxes = boxes.long()
    for b in range(boxes.shape[0]):
        for n in range(boxes.shape[1]):
            u1, v1, u2, v2 = (int(v) for v in boxes[b, n])
            fg_mask[b, v1:v2, u1:u2] = True
    return fg_mask


def focal_loss(logits, target, alpha, gamma):
    """kornia.losses.FocalLoss(alpha, gamma, reduction="none"): sum over classes of one_hot * -alpha (1 - p)^gamma log p"""
    log_p = F.log_softmax(logits, dim=1)
    one_hot = F.one_hot(target, logits.shape[1]).movedim(-1, 1).to(logits.dtype)
    return (one_hot * (-alpha * torch.pow(1.0 - log_p.exp(), gamma) * log_p)).sum(dim=1)


def ddn_loss(depth_logits, depth_maps, gt_boxes2d, disc, weight, alpha, gamma, fg_weight, bg_weight, downsample_factor):
    target = bin_depths(depth_maps, **disc, target=True)
    loss = focal_loss(depth_logits, target, alpha, gamma)
    fg = compute_fg_mask(gt_boxes2d, loss.shape, downsample_factor)
    bg = ~fg
    loss = loss * (fg_weight * fg + bg_weight * bg)
    num_pixels = fg.sum() + bg.sum()
    fg_loss, bg_loss = loss[fg].sum() / num_pixels, loss[bg].sum() / num_pixels
    return (fg_loss + bg_loss) * weight, fg_loss, bg_loss


# ---------------------------------------------------------------------------------------------------------------- cases
def _l2c(shift=(0.0, 0.0, 0.0), t=(0.02, -0.05, -0.2)):
    """LiDAR -> camera: the axis swap x -> z, -y -> x, -z -> y, then a translation"""
    m = torch.tensor([[0., -1., 0., 0.], [0., 0., -1., 0.], [1., 0., 0., 0.], [0., 0., 0., 1.]], dtype=torch.float64)
    m[:3, 3] = torch.tensor(t, dtype=torch.float64) + torch.tensor(shift, dtype=torch.float64)
    return m


def _c2i(fx=30.0, fy=30.0, cx=26.0, cy=18.0, t=(1.5, 0.2, 0.003)):
    return torch.tensor([[fx, 0., cx, t[0]], [0., fy, cy, t[1]], [0., 0., 1., t[2]]], dtype=torch.float64)


def _base(name, mode="LID", C=5, D=7, grad=True, shapes=((36, 52), (36, 52)), c2i=None, seed=0, **over):
    case = dict(name=name, B=2, C=C, D=D, H=9, W=13, image_shape=shapes, grid_size=(11, 10, 3), pc_range=(1., -6., -2., 12., 6., 1.),
                disc=dict(mode=mode, num_bins=D, depth_min=2.0, depth_max=11.0), grad=grad, seed=seed,
                lidar_to_cam=torch.stack([_l2c(), _l2c(shift=(0.1, 0.03, 0.4))]),
                cam_to_img=torch.stack(c2i if c2i is not None else [_c2i(), _c2i(fx=34.0)]))
    case.update(over)
    return case


def _centres():
    """Voxel centres exactly on pixel centres, the outermost on the last row / column, in numbers fp32 holds exactly, so that the weights are exactly
    0 and 1 and the H - 1, W - 1 border is hit.  Camera z = 2 and 4 (X = 2); lateral and height centres -1, 0, 1; fx = 16, cx = 8 gives
    u = 16, 8, 0 at z = 2 and 12, 8, 4 at z = 4; fy = 8, cy = 4 gives v = 8, 4, 0 and 6, 4, 2.  The image is as large as the feature map and
    W - 1 = 16, H - 1 = 8, D - 1 = 4 are powers of two, so normalising and unnormalising are exact; UD with bin size 1 puts the depths on bins 0 and 2."""
    l2c = torch.stack([_l2c(t=(0., 0., 0.))] * 2)
    c2i = torch.stack([_c2i(fx=16.0, fy=8.0, cx=8.0, cy=4.0, t=(0., 0., 0.))] * 2)
    return dict(name="centres", B=2, C=5, D=5, H=9, W=17, image_shape=((9, 17), (9, 17)), grid_size=(2, 3, 3), pc_range=(1., -1.5, -1.5, 5., 1.5, 1.5),
                disc=dict(mode="UD", num_bins=5, depth_min=2.0, depth_max=7.0), grad=True, seed=5, lidar_to_cam=l2c, cam_to_img=c2i)


CASES = {c["name"]: c for c in [
    _base("base_LID", "LID"), _base("base_UD", "UD", seed=1), _base("base_SID", "SID", seed=2),
    _base("c1", C=1, seed=3), _base("c64", C=64, seed=4), _base("c130", C=130, seed=9), _base("d1", D=1, seed=6),
    _base("outside", c2i=[_c2i(cx=4000.0), _c2i(cx=-4000.0)], seed=7),
    _base("shapes", shapes=((36, 52), (30, 40)), seed=8),
    _base("tall", pc_range=(1., -6., -2., 12., 6., 4.), seed=11),       # the base case never leaves the image at the top: this one does
    _base("chunked", C=2740, grad=False, seed=10),          # C * Z beyond the forward's staging run
    _centres(),
]}


def make_inputs(case, dtype):
    """seeded image_features (B, C, H, W) and depth_probs (B, D + 1, H, W) (a softmax, made in float64), the calibration, image_shape int32"""
    g = torch.Generator().manual_seed(1234 + case["seed"])
    B, C, D, H, W = (case[k] for k in "BCDHW")
    feats = torch.randn((B, C, H, W), generator=g, dtype=torch.float64)
    probs = F.softmax(2.0 * torch.randn((B, D + 1, H, W), generator=g, dtype=torch.float64), dim=1)
    gout = torch.randn((B, C) + tuple(reversed(case["grid_size"])), generator=g, dtype=torch.float64)
    # every input is rounded to float32 first: the float64 run sees the numbers the kernel sees
    f32 = lambda t: t.to(torch.float32).to(dtype)
    return SimpleNamespace(feats=f32(feats), probs=f32(probs), gout=f32(gout), lidar_to_cam=f32(case["lidar_to_cam"]), cam_to_img=f32(case["cam_to_img"]),
                           image_shape=torch.tensor(case["image_shape"], dtype=torch.int32))


def run(case, dtype, grad=False):
    """the restatement on a case in `dtype`: out (B, C, Z, Y, X) [, d (out * gout).sum() / d feats, / d probs]"""
    x = make_inputs(case, dtype)
    feats, probs = x.feats.requires_grad_(grad), x.probs.requires_grad_(grad)
    grid = frustum_grid(x.lidar_to_cam, x.cam_to_img, x.image_shape, case["grid_size"], case["pc_range"], case["disc"], dtype)
    out = sample(frustum_from_probs(feats, probs), grid)
    if not grad:
        return out.detach()
    (out * x.gout).sum().backward()
    return out.detach(), feats.grad, probs.grad


@functools.lru_cache(maxsize=None)
def reference(name):
    """Computed once per case and shared, never written to: float64 grid, jump mask (B, X, Y, Z), float64 out and gradients, and the allowances
    (E32 of the forward, of grad feats, of grad probs)."""
    case = CASES[name]
    x = make_inputs(case, torch.float64)
    grid, near = frustum_grid(x.lidar_to_cam, x.cam_to_img, x.image_shape, case["grid_size"], case["pc_range"], case["disc"], torch.float64, with_mask=True)
    if case["grad"]:
        out, gf, gp = run(case, torch.float64, grad=True)
        out32, gf32, gp32 = run(case, torch.float32, grad=True)
        e_gf, e_gp = float((gf32.double() - gf).abs().max()), float((gp32.double() - gp).abs().max())
    else:
        out, out32 = run(case, torch.float64), run(case, torch.float32)
        gf = gp = None
        e_gf = e_gp = None
    keep = ~near.permute(0, 3, 2, 1).unsqueeze(1)                          # (B, 1, Z, Y, X)
    e_fwd = float(((out32.double() - out).abs() * keep).max())
    return SimpleNamespace(case=case, grid=grid, near=near, out=out, grad_feats=gf, grad_probs=gp, e_fwd=e_fwd, e_grad_feats=e_gf, e_grad_probs=e_gp)
