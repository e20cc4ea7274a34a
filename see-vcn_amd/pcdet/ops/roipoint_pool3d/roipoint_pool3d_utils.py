"""RoIPointPool3d / RoIPointPool3dFunction with the reference's names, constructor and forward signature (detector3d/pcdet/ops/roipoint_pool3d/
roipoint_pool3d_utils.py:9-63) over roipoint_pool3d_cuda.forward.  The outputs are allocated uninitialised: the kernel writes every element.
`canonical` (keyword, default False) asks for box-frame xyz columns; the reference-shaped call stays reference-shaped."""
import torch
import torch.nn as nn
from torch.autograd import Function

from ...utils import box_utils
from . import roipoint_pool3d_cuda


class RoIPointPool3d(nn.Module):
    def __init__(self, num_sampled_points=512, pool_extra_width=1.0):
        super().__init__()
        self.num_sampled_points = num_sampled_points
        self.pool_extra_width = pool_extra_width

    def forward(self, points, point_features, boxes3d, canonical=False):
        """points (B, N, 3), point_features (B, N, C), boxes3d (B, M, 7) -> pooled_features (B, M, num_sampled_points, 3 + C),
        pooled_empty_flag (B, M) int32"""
        return RoIPointPool3dFunction.apply(points, point_features, boxes3d, self.pool_extra_width, self.num_sampled_points, canonical)


class RoIPointPool3dFunction(Function):
    @staticmethod
    def forward(ctx, points, point_features, boxes3d, pool_extra_width, num_sampled_points=512, canonical=False):
        assert points.dim() == 3 and points.shape[2] == 3
        batch_size, boxes_num, feature_len = points.shape[0], boxes3d.shape[1], point_features.shape[2]
        pooled_boxes3d = box_utils.enlarge_box3d(boxes3d.reshape(-1, 7), pool_extra_width).view(batch_size, -1, 7)
        pooled_features = torch.empty((batch_size, boxes_num, num_sampled_points, 3 + feature_len), dtype=torch.float32, device=points.device)
        pooled_empty_flag = torch.empty((batch_size, boxes_num), dtype=torch.int32, device=points.device)
        roipoint_pool3d_cuda.forward(points.contiguous().float(), pooled_boxes3d.contiguous().float(), point_features.contiguous().float(),
                                     pooled_features, pooled_empty_flag, canonical=canonical)
        return pooled_features, pooled_empty_flag

    @staticmethod
    def backward(ctx, *grad_out):
        raise NotImplementedError
