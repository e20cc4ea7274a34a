"""FrustumToVoxel (reference f2v/frustum_to_voxel.py:8-54).  With the bilinear / zeros sampler the forward is one fused kernel over
batch_dict["image_features"] and batch_dict["depth_probs"] (ops/frustum_ops.py): the (B, C, D, H, W) frustum volume and the (B, X, Y, Z, 3) grid are
never built and the gradient is order-fixed.  SEEVCN_FUSED_FRUSTUM=0, or any other sampler mode, runs the reference's statements on
batch_dict["frustum_features"]: sv_frustum_grid, then F.grid_sample."""
import os

import torch.nn as nn

from ......ops import frustum_ops
from ......utils.common_utils import cfg_get
from .frustum_grid_generator import FrustumGridGenerator
from .sampler import Sampler


def fused_enabled():
    return os.environ.get("SEEVCN_FUSED_FRUSTUM", "1") != "0"


class FrustumToVoxel(nn.Module):
    def __init__(self, model_cfg, grid_size, pc_range, disc_cfg):
        super().__init__()
        self.model_cfg = model_cfg
        self.grid_size = [int(v) for v in grid_size]
        self.pc_range = [float(v) for v in pc_range]
        self.disc_cfg = dict(disc_cfg)
        self.grid_generator = FrustumGridGenerator(grid_size=grid_size, pc_range=pc_range, disc_cfg=self.disc_cfg)
        self.sampler = Sampler(**dict(cfg_get(model_cfg, 'SAMPLER')))

    @property
    def fused(self):
        """whether forward() reads image_features / depth_probs (fused) or frustum_features (module tree); DepthFFN asks before it builds the volume"""
        return fused_enabled() and self.sampler.mode == "bilinear" and self.sampler.padding_mode == "zeros"

    def forward(self, batch_dict):
        """trans_lidar_to_cam (B, 4, 4), trans_cam_to_img (B, 3, 4), image_shape (B, 2) -> voxel_features (B, C, Z, Y, X)"""
        if self.fused and "image_features" in batch_dict and "depth_probs" in batch_dict:
            batch_dict["voxel_features"] = frustum_ops.frustum_to_voxel(
                batch_dict["image_features"], batch_dict["depth_probs"], batch_dict["trans_lidar_to_cam"], batch_dict["trans_cam_to_img"],
                batch_dict["image_shape"], self.grid_size, self.pc_range, self.disc_cfg)
            return batch_dict
        grid = self.grid_generator(lidar_to_cam=batch_dict["trans_lidar_to_cam"], cam_to_img=batch_dict["trans_cam_to_img"],
                                   image_shape=batch_dict["image_shape"])                        # (B, X, Y, Z, 3)
        voxel_features = self.sampler(input_features=batch_dict["frustum_features"], grid=grid)   # (B, C, X, Y, Z)
        batch_dict["voxel_features"] = voxel_features.permute(0, 1, 4, 3, 2)                      # (B, C, Z, Y, X)
        return batch_dict
