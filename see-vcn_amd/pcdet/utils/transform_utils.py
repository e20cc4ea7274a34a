"""Camera projection and depth discretisation for CaDDN (reference utils/transform_utils.py:14-91).  The two kornia conversions the reference
imports are restated here; kornia is not a dependency and its version is UNPINNED in the reference, so the restatement follows the formula that
kornia has kept since 0.2: scale = where(|z| > 1e-8, 1 / (z + 1e-8), 1)."""
import math

import torch


def convert_points_to_homogeneous(points):
    """(..., D) -> (..., D + 1) with a trailing 1 (kornia.geometry.conversions, unpinned)"""
    return torch.nn.functional.pad(points, [0, 1], "constant", 1.0)


def convert_points_from_homogeneous(points, eps=1e-8):
    """(..., D + 1) -> (..., D): the leading components times 1 / (z + eps), or times 1 where |z| <= eps (kornia.geometry.conversions, unpinned)"""
    z = points[..., -1:]
    scale = torch.where(torch.abs(z) > eps, 1.0 / (z + eps), torch.ones_like(z))
    return scale * points[..., :-1]


def transform_points(trans_01, points_1):
    """kornia.geometry.linalg.transform_points (unpinned): (..., D + 1, D + 1) applied to (..., N, D) points"""
    points_1_h = convert_points_to_homogeneous(points_1)
    points_0_h = torch.matmul(trans_01.unsqueeze(-3), points_1_h.unsqueeze(-1)).squeeze(-1)
    return convert_points_from_homogeneous(points_0_h)


def project_to_image(project, points):
    """project (..., 3, 4), points (..., N, 3) -> image points (..., N, 2) and depths (..., N)"""
    points = convert_points_to_homogeneous(points).unsqueeze(dim=-1)
    project = project.unsqueeze(dim=1)
    points_t = (project @ points).squeeze(dim=-1)
    points_img = convert_points_from_homogeneous(points_t)
    points_depth = points_t[..., -1] - project[..., 2, 3]
    return points_img, points_depth


def normalize_coords(coords, shape):
    """coordinates (..., 3) of a grid of `shape` (3,), reversed, to [-1, 1]; pixel indices run over [0, shape - 1]"""
    shape = torch.flip(shape, dims=[0])
    return coords / (shape - 1) * 2 + -1


def bin_depths(depth_map, mode, depth_min, depth_max, num_bins, target=False):
    """Depth -> bin index (continuous), UD / LID / SID of arXiv 2005.13423.  target=True: indices outside [0, num_bins] and non-finite ones become
    num_bins, the result is int64."""
    if mode == "UD":
        bin_size = (depth_max - depth_min) / num_bins
        indices = (depth_map - depth_min) / bin_size
    elif mode == "LID":
        bin_size = 2 * (depth_max - depth_min) / (num_bins * (1 + num_bins))
        indices = -0.5 + 0.5 * torch.sqrt(1 + 8 * (depth_map - depth_min) / bin_size)
    elif mode == "SID":
        indices = num_bins * (torch.log(1 + depth_map) - math.log(1 + depth_min)) / (math.log(1 + depth_max) - math.log(1 + depth_min))
    else:
        raise NotImplementedError
    if target:
        mask = (indices < 0) | (indices > num_bins) | (~torch.isfinite(indices))
        indices = torch.where(mask, torch.full_like(indices, num_bins), indices).type(torch.int64)
    return indices
