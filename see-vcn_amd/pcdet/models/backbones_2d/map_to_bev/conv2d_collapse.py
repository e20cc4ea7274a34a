"""Conv2DCollapse (reference backbones_2d/map_to_bev/conv2d_collapse.py:7-38): the height slices of the voxel volume become channels and a 1x1
BasicBlock2D reduces them.  The fused frustum sampling writes voxel_features (B, C, Z, Y, X) with the storage order (B, Y, X, C, Z); flatten(1, 2)
of that is a view, and the view is a channels_last (B, C*Z, Y, X) tensor -- the 1x1 convolution reads it as it lies.  Any other layout (a plain
contiguous volume, the module-tree route's permuted grid_sample output) goes through the same flatten, which then copies if it must.
HeightCompression's `feeds_bev_backbone` flag has no counterpart here: spatial_features is the convolution's output, in whatever memory
format the convolution chose, not a volume this module lays out."""
import torch.nn as nn

from ...model_utils.basic_block_2d import BasicBlock2D
from ....utils.common_utils import cfg_get


class Conv2DCollapse(nn.Module):
    def __init__(self, model_cfg, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_heights = int(grid_size[-1])
        self.num_bev_features = cfg_get(model_cfg, 'NUM_BEV_FEATURES')
        self.block = BasicBlock2D(in_channels=self.num_bev_features * self.num_heights, out_channels=self.num_bev_features,
                                  **dict(cfg_get(model_cfg, 'ARGS')))

    def forward(self, batch_dict):
        """voxel_features (B, C, Z, Y, X) -> spatial_features (B, C, Y, X)"""
        voxel_features = batch_dict["voxel_features"]
        bev_features = voxel_features.flatten(start_dim=1, end_dim=2)      # (B, C*Z, Y, X): channel c * Z + z
        batch_dict["spatial_features"] = self.block(bev_features)
        return batch_dict
