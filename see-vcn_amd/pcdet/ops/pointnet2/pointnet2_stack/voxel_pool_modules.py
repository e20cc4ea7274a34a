import os
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..... import _lib, dense_ops
from . import pointnet2_stack_cuda, voxel_query_utils

FUSED_VOXEL_POOL_OFF = os.environ.get("SEEVCN_FUSED_VOXEL_POOL", "1") == "0"      # 0: always the module tree (A/B runs, tests)


def _fold(conv, bn):
    """An eval-mode BatchNorm behind a bias-free 1x1 conv as one weight (c_out, c_in) and one bias (c_out)."""
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    w = conv.weight.detach().reshape(conv.out_channels, conv.in_channels) * scale.view(-1, 1)
    return w.contiguous(), (bn.bias.detach() - bn.running_mean * scale).contiguous()


class NeighborVoxelSAModuleMSG(nn.Module):
    """Voxel RoI pooling of Voxel R-CNN: per scale, a voxel query around every grid point on the dense cell -> row volume, features of the found
    voxels (mlps_in) plus an embedding of their offset (mlps_pos), ReLU, pooling over the neighbours, mlps_out.  Same constructor, submodule names,
    parameter shapes and forward signature as the reference (ops/pointnet2/pointnet2_stack/voxel_pool_modules.py:8-130).

    Eval mode under torch.no_grad() with max_pool takes the fused route: mlps_in and mlps_out are one GEMM each with the BatchNorm folded in, and
    sv_voxel_pool_max reads the query's idx directly -- no (M, C, nsample) tensor.  Everything else (training, avg_pool, other shapes,
    SEEVCN_FUSED_VOXEL_POOL=0) runs the module tree over the grouping ops, whose gradient follows set_ordered_gradients."""

    def __init__(self, *, query_ranges: List[List[int]], radii: List[float], nsamples: List[int], mlps: List[List[int]], use_xyz: bool = True,
                 pool_method='max_pool'):
        super().__init__()
        assert len(query_ranges) == len(nsamples) == len(mlps)
        self.groupers = nn.ModuleList()
        self.mlps_in = nn.ModuleList()
        self.mlps_pos = nn.ModuleList()
        self.mlps_out = nn.ModuleList()
        for max_range, radius, nsample, spec in zip(query_ranges, radii, nsamples, mlps):
            self.groupers.append(voxel_query_utils.VoxelQueryAndGrouping(list(max_range), radius, nsample))
            self.mlps_in.append(nn.Sequential(nn.Conv1d(spec[0], spec[1], kernel_size=1, bias=False), nn.BatchNorm1d(spec[1])))
            self.mlps_pos.append(nn.Sequential(nn.Conv2d(3, spec[1], kernel_size=1, bias=False), nn.BatchNorm2d(spec[1])))
            self.mlps_out.append(nn.Sequential(nn.Conv1d(spec[1], spec[2], kernel_size=1, bias=False), nn.BatchNorm1d(spec[2]), nn.ReLU()))
        self.relu = nn.ReLU()
        self.pool_method = pool_method
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def train(self, mode=True):
        self._folded = {}                     # folded BatchNorm: re-made after any switch of mode (fused optimisers do not bump tensor versions)
        return super().train(mode)

    def _fused_ok(self, k, xyz, features):
        """sv_voxel_pool_max takes this scale: eval mode, no gradient recorded, max pooling, C1 in {16, 32, 48, 64}, at most 32 neighbours, fp32 on the GPU."""
        if self.training or torch.is_grad_enabled() or self.pool_method != 'max_pool' or FUSED_VOXEL_POOL_OFF:
            return False
        if not (xyz.is_cuda and features.is_cuda and features.dtype == torch.float32):
            return False
        c1 = self.mlps_in[k][0].out_channels
        mods = [m for seq in (self.mlps_in[k], self.mlps_pos[k], self.mlps_out[k]) for m in seq]
        if any(dense_ops._has_hooks(m) for m in mods + [self.mlps_in[k], self.mlps_pos[k], self.mlps_out[k]]):
            return False
        if not all(bn.track_running_stats and bn.affine for bn in (self.mlps_in[k][1], self.mlps_pos[k][1], self.mlps_out[k][1])):
            return False
        return c1 % 16 == 0 and 16 <= c1 <= 64 and 1 <= self.groupers[k].nsample <= 32

    def _folded_weights(self, k):
        pairs = [(seq[0], seq[1]) for seq in (self.mlps_in[k], self.mlps_pos[k], self.mlps_out[k])]
        # load_state_dict and in-place edits bump the version counters; a device move makes new tensors
        stamp = tuple((t.data_ptr(), t._version) for conv, bn in pairs for t in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var))
        hit = self.__dict__.setdefault('_folded', {}).get(k)
        if hit is None or hit[0] != stamp:
            hit = self._folded[k] = (stamp, tuple(t for conv, bn in pairs for t in _fold(conv, bn)))
        return hit[1]

    def _fused_scale(self, k, xyz, new_xyz, new_coords, features, voxel2point_indices):
        g = self.groupers[k]
        w_in, b_in, w_pos, b_pos, w_out, b_out = self._folded_weights(k)
        M, N = new_xyz.shape[0], xyz.shape[0]
        B, Z, Y, X = voxel2point_indices.shape
        idx = torch.zeros((M, g.nsample), dtype=torch.int32, device=new_xyz.device)
        pointnet2_stack_cuda.voxel_query_wrapper(M, Z, Y, X, g.nsample, g.radius, g.max_range[0], g.max_range[1], g.max_range[2], new_xyz, xyz, new_coords,
                                                 voxel2point_indices, idx)
        f_in = dense_ops._gemm_nt(features, w_in, b_in, dense_ops.ACT_NONE, 0.0)                       # (N, C1)
        pooled = torch.empty((M, w_in.shape[0]), dtype=torch.float32, device=new_xyz.device)
        _lib.launch("sv_voxel_pool_max", _lib.ptr(f_in), _lib.ptr(xyz), _lib.ptr(new_xyz), _lib.ptr(idx), _lib.ptr(w_pos), _lib.ptr(b_pos), M, N, w_in.shape[0],
                    g.nsample, _lib.ptr(pooled))
        return dense_ops._gemm_nt(pooled, w_out, b_out, dense_ops.ACT_RELU, 0.0)                       # (M, C2)

    def _tree_scale(self, k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices):
        # mlps_in / mlps_out are Conv1d + BatchNorm1d over rows: the library's dense-layer kernels with their own backward (dense_ops.run_sequential)
        features_in = dense_ops.run_sequential(self.mlps_in[k], features)                              # (N, C1)
        grouped_features, grouped_xyz, empty_ball_mask = self.groupers[k](new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt,
                                                                          features_in.contiguous(), voxel2point_indices)
        keep = (~empty_ball_mask).view(-1, 1, 1)
        grouped_features = torch.where(keep, grouped_features, 0)                                      # an empty query groups zeros
        grouped_xyz = torch.where(keep, grouped_xyz - new_xyz.unsqueeze(-1), 0)
        position_features = self.mlps_pos[k](grouped_xyz.permute(1, 0, 2).unsqueeze(0).contiguous())   # (1, C1, M, nsample)
        new_features = self.relu(grouped_features.permute(1, 0, 2).unsqueeze(0) + position_features)
        if self.pool_method == 'max_pool':
            new_features = F.max_pool2d(new_features, kernel_size=[1, new_features.size(3)]).squeeze(dim=-1)   # (1, C1, M)
        elif self.pool_method == 'avg_pool':
            new_features = F.avg_pool2d(new_features, kernel_size=[1, new_features.size(3)]).squeeze(dim=-1)
        else:
            raise NotImplementedError
        return dense_ops.run_sequential(self.mlps_out[k], new_features.squeeze(dim=0).permute(1, 0).contiguous())   # (M, C2)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices):
        """xyz (N1 + N2 .., 3) voxel centres, features (N1 + N2 .., C), new_xyz (M1 + M2 .., 3), new_coords (M1 + M2 .., 4) int32 [b, x, y, z],
        voxel2point_indices (B, Z, Y, X) int32 -> (M1 + M2 .., sum of the scales' last channel counts)"""
        if self.pool_method not in ('max_pool', 'avg_pool'):
            raise NotImplementedError
        new_coords = torch.cat([new_coords[:, 0:1], new_coords[:, 1:4].flip(1)], dim=1).contiguous()  # -> [b, z, y, x]; no index list (a host -> device copy)
        xyz, new_xyz, features = xyz.contiguous(), new_xyz.contiguous(), features.contiguous()
        outs = []
        for k in range(len(self.groupers)):
            if self._fused_ok(k, xyz, features):
                outs.append(self._fused_scale(k, xyz, new_xyz, new_coords, features, voxel2point_indices))
            else:
                outs.append(self._tree_scale(k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices))
        return torch.cat(outs, dim=1)
