"""Voxel query with the reference's names and call signatures (detector3d/pcdet/ops/pointnet2/pointnet2_stack/voxel_query_utils.py:10-100),
over sv_voxel_query_stack and the grouping ops of pointnet2_utils."""
import torch
import torch.nn as nn
from torch.autograd import Function

from ..... import _lib
from ....utils import common_utils
from . import pointnet2_stack_cuda as pointnet2
from . import pointnet2_utils


class VoxelQuery(Function):
    @staticmethod
    def forward(ctx, max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices):
        """xyz (N, 3) voxel centres, new_xyz (M, 3), new_coords (M, 4) int32 [b, z, y, x], point_indices (B, Z, Y, X) int32 ->
        idx (M, nsample) int32 GLOBAL rows of xyz (0 in an empty query), empty_ball_mask (M,)"""
        assert new_xyz.is_contiguous() and xyz.is_contiguous() and new_coords.is_contiguous() and point_indices.is_contiguous()
        M = new_coords.shape[0]
        B, Z, Y, X = point_indices.shape
        idx = torch.zeros((M, nsample), dtype=torch.int32, device=new_xyz.device)
        z_range, y_range, x_range = max_range
        pointnet2.voxel_query_wrapper(M, Z, Y, X, nsample, radius, z_range, y_range, x_range, new_xyz, xyz, new_coords, point_indices, idx)
        empty_ball_mask = (idx[:, 0] == -1)
        idx[empty_ball_mask] = 0
        ctx.mark_non_differentiable(idx, empty_ball_mask)
        return idx, empty_ball_mask

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None, None, None, None


voxel_query = VoxelQuery.apply


class VoxelQueryAndGrouping(nn.Module):
    def __init__(self, max_range, radius, nsample):
        super().__init__()
        self.max_range, self.radius, self.nsample = max_range, radius, nsample

    def forward(self, new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, voxel2point_indices):
        """new_coords (M, 4) [b, z, y, x]; xyz (N, 3), features (N, C) stacked over the scenes -> grouped_features (M, C, nsample),
        grouped_xyz (M, 3, nsample), empty_ball_mask (M,).  The gradient of the grouping follows set_ordered_gradients like every grouping_operation."""
        assert xyz.shape[0] == xyz_batch_cnt.sum(), 'xyz: %s, xyz_batch_cnt: %s' % (str(xyz.shape), str(new_xyz_batch_cnt))
        assert new_coords.shape[0] == new_xyz_batch_cnt.sum(), \
            'new_coords: %s, new_xyz_batch_cnt: %s' % (str(new_coords.shape), str(new_xyz_batch_cnt))
        idx, empty_ball_mask = voxel_query(self.max_range, self.radius, self.nsample, xyz, new_xyz, new_coords, voxel2point_indices)
        # the query answers in rows of the stacked xyz, the grouping ops count from their scene's first row (the reference subtracts scene by scene
        # on the host and needs equally many queries in every scene; here one subtraction of the per-query first row)
        row_start = pointnet2._row_start(new_xyz_batch_cnt, xyz_batch_cnt, idx.shape[0])
        idx = torch.where(empty_ball_mask.view(-1, 1), 0, idx - row_start.view(-1, 1)).contiguous()
        grouped_xyz = pointnet2_utils.grouping_operation(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        grouped_features = pointnet2_utils.grouping_operation(features, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        return grouped_features, grouped_xyz, empty_ball_mask


_volumes = {}


class borrowed_voxel2pinds:
    """`with borrowed_voxel2pinds(sparse_tensor) as volume`: generate_voxel2pinds' volume in a buffer kept per (device, stream, shape).  The buffer
    is all -1 between uses: entering scatters the N rows, leaving scatters -1 over them again -- two N-row launches instead of a pass over
    B*Z*Y*X cells (94 MB for x_conv2 at KITTI sizes) every call.  The volume is only valid inside the block."""

    def __init__(self, sparse_tensor):
        self.indices = sparse_tensor.indices
        self.shape = tuple([int(sparse_tensor.batch_size)] + [int(s) for s in sparse_tensor.spatial_shape])

    def __enter__(self):
        dev = self.indices.device
        key = (dev.index, _lib.stream(), self.shape)
        vol = _volumes.get(key)
        if vol is None:
            if len(_volumes) >= 16:
                _volumes.clear()
            vol = _volumes[key] = torch.full(self.shape, -1, dtype=torch.int32, device=dev)
        self.volume = common_utils.scatter_voxel_rows(self.indices, vol, fill=False)
        return self.volume

    def __exit__(self, *exc):
        common_utils.scatter_voxel_rows(self.indices, self.volume, fill=False, clear=True)
        return False
