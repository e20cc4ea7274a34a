from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..... import _lib
from . import pointnet2_stack_cuda, pointnet2_utils


import os

FUSED_SA_OFF = os.environ.get("SEEVCN_FUSED_SA", "1") == "0"      # 0: always the torch path (A/B runs, tests)
TRAIN_SA_OFF = os.environ.get("SEEVCN_TRAIN_SA", "1") == "0"      # 0: training goes through the (M, C, nsample) Conv2d path of the reference


def _cfg(config, key, default=None):
    return config.get(key, default) if hasattr(config, 'get') else getattr(config, key, default)


def build_local_aggregation_module(input_channels, config):
    """(reference pointnet2_modules.py:10-27)"""
    name = _cfg(config, 'NAME', 'StackSAModuleMSG')
    if name == 'VectorPoolAggregationModuleMSG':
        return VectorPoolAggregationModuleMSG(input_channels=input_channels, config=config), _cfg(config, 'MSG_POST_MLPS')[-1]
    if name != 'StackSAModuleMSG':
        raise NotImplementedError(name)
    mlps = [[input_channels] + list(m) for m in _cfg(config, 'MLPS')]
    layer = StackSAModuleMSG(radii=_cfg(config, 'POOL_RADIUS'), nsamples=_cfg(config, 'NSAMPLE'), mlps=mlps, use_xyz=True, pool_method='max_pool')
    return layer, sum(m[-1] for m in mlps)


class StackSAModuleMSG(nn.Module):
    """Multi-scale set abstraction over stacked batches: ball query + group (HIP) -> shared 1x1 conv / BN / ReLU -> max over
    the neighbours. Same constructor, submodule names (groupers, mlps) and forward signature as the reference
    (ops/pointnet2/pointnet2_stack/pointnet2_modules.py:30-112)."""

    def __init__(self, *, radii: List[float], nsamples: List[int], mlps: List[List[int]], use_xyz: bool = True, pool_method='max_pool'):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for radius, nsample, spec in zip(radii, nsamples, mlps):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz))
            spec = list(spec)
            if use_xyz:
                spec[0] += 3
            layers = []
            for k in range(len(spec) - 1):
                layers += [nn.Conv2d(spec[k], spec[k + 1], kernel_size=1, bias=False), nn.BatchNorm2d(spec[k + 1]), nn.ReLU()]
            self.mlps.append(nn.Sequential(*layers))
        self.pool_method = pool_method
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def train(self, mode=True):
        self._fused_weights = {}              # folded BatchNorm: re-made after any switch of mode (fused optimisers do not bump tensor versions)
        return super().train(mode)

    def _fused_ok(self, k, xyz, new_xyz, features):
        """The fused eval kernel (sv_sa_mlp_max) takes this scale: 2 conv-BN-ReLU layers of 16..64 channels, 16 or 32 neighbours, max pooling,
        feature channels a multiple of 16 up to 128 (or none), no gradient needed."""
        if self.training or self.pool_method != 'max_pool' or FUSED_SA_OFF or not (xyz.is_cuda and new_xyz.is_cuda):
            return False
        if torch.is_grad_enabled() and ((features is not None and features.requires_grad) or any(p.requires_grad for p in self.mlps[k].parameters())):
            return False
        layers = list(self.mlps[k])
        if len(layers) != 6 or not all(isinstance(layers[i], nn.Conv2d) and isinstance(layers[i + 1], nn.BatchNorm2d) for i in (0, 3)):
            return False
        c = 0 if features is None else features.shape[1]
        c1, c2 = layers[0].out_channels, layers[3].out_channels
        ns = self.groupers[k].nsample
        return (c % 16 == 0 and c <= 128 and layers[0].in_channels == c + 3 and ns in (16, 32) and all(v % 16 == 0 and 16 <= v <= 64 for v in (c1, c2))
                and layers[0].bias is None and layers[3].bias is None and (features is None or features.dtype == torch.float32))

    def _prepared(self, k, device):
        hit = self._fused_weights.get(k) if hasattr(self, '_fused_weights') else None
        if hit is not None:
            return hit
        layers = list(self.mlps[k])
        out = []
        for conv, bn, first in ((layers[0], layers[1], 1), (layers[3], layers[4], 0)):
            co, ci = conv.out_channels, conv.in_channels
            kp = 16 * ((ci - 3) // 16 + 1) if first else ci
            w = torch.empty((co, kp), dtype=torch.float32, device=device)
            b = torch.empty((co,), dtype=torch.float32, device=device)
            _lib.launch("sv_sa_prepare_weights", _lib.ptr(conv.weight.detach().reshape(co, ci).contiguous()), _lib.ptr(bn.weight.detach()),
                        _lib.ptr(bn.bias.detach()), _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var), float(bn.eps), co, ci, first, _lib.ptr(w), _lib.ptr(b))
            out += [w, b]
        if not hasattr(self, '_fused_weights'):
            self._fused_weights = {}
        self._fused_weights[k] = tuple(out)
        return self._fused_weights[k]

    def _fused_scale(self, k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features):
        """ball query (HIP) -> sv_sa_mlp_max: gather + both MLP layers on the matrix core + max over the neighbours in ONE launch; no
        (M, C+3, nsample) tensor (the torch path below materialises it and runs Conv2d / BatchNorm2d / max_pool2d over it)."""
        g = self.groupers[k]
        M, B = new_xyz.shape[0], xyz_batch_cnt.shape[0]
        idx = torch.zeros((M, g.nsample), dtype=torch.int32, device=new_xyz.device)
        pointnet2_stack_cuda.ball_query_wrapper(B, M, g.radius, g.nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx)
        row_start = pointnet2_stack_cuda._row_start(new_xyz_batch_cnt, xyz_batch_cnt, M)
        w1, b1, w2, b2 = self._prepared(k, new_xyz.device)
        c = 0 if features is None else features.shape[1]
        out = torch.empty((M, w2.shape[0]), dtype=torch.float32, device=new_xyz.device)
        _lib.launch("sv_sa_mlp_max", _lib.ptr(xyz), _lib.ptr(features) if c else None, _lib.ptr(new_xyz), _lib.ptr(idx), _lib.ptr(row_start), M, c, g.nsample,
                    _lib.ptr(w1), _lib.ptr(b1), w1.shape[0], _lib.ptr(w2), _lib.ptr(b2), w2.shape[0], _lib.ptr(out))
        return out

    def _train_ok(self, k, xyz, new_xyz, features):
        """The training kernels (sv_sa_train_forward / _backward) take this scale: two conv-BN-ReLU layers of 16..64 channels without conv bias,
        16 or 32 neighbours, max pooling, feature channels a multiple of 16 up to 128 (or none), fp32 on the GPU, xyz in the features,
        BatchNorm2d in training mode with affine parameters and running statistics."""
        if (TRAIN_SA_OFF or not self.training or self.pool_method != 'max_pool' or not (xyz.is_cuda and new_xyz.is_cuda) or not self.groupers[k].use_xyz
                or new_xyz.shape[0] * self.groupers[k].nsample < 2):
            return False
        layers = list(self.mlps[k])
        if len(layers) != 6 or (features is not None and features.dtype != torch.float32):
            return False
        for i in (0, 3):
            conv, bn = layers[i], layers[i + 1]
            if not (isinstance(conv, nn.Conv2d) and type(bn) is nn.BatchNorm2d and isinstance(layers[i + 2], nn.ReLU) and conv.bias is None
                    and bn.training and bn.affine and bn.track_running_stats and bn.momentum is not None):
                return False
            if conv._forward_hooks or conv._forward_pre_hooks or bn._forward_hooks or bn._forward_pre_hooks:
                return False
        c = 0 if features is None else features.shape[1]
        c1, c2 = layers[0].out_channels, layers[3].out_channels
        return (c % 16 == 0 and c <= 128 and layers[0].in_channels == c + 3 and layers[3].in_channels == c1 and self.groupers[k].nsample in (16, 32)
                and all(v % 16 == 0 and 16 <= v <= 64 for v in (c1, c2)) and layers[1].eps == layers[4].eps and layers[1].momentum == layers[4].momentum)

    def _train_scale(self, k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features):
        """ball query (HIP) -> SAScaleTrain: the whole scale (gather, both MLP layers with batch-statistics BatchNorm, max over the neighbours) and its
        backward on the hand-written MFMA kernels; same parameters, running statistics and num_batches_tracked as the Conv2d / BatchNorm2d path."""
        g = self.groupers[k]
        M, B = new_xyz.shape[0], xyz_batch_cnt.shape[0]
        idx = torch.zeros((M, g.nsample), dtype=torch.int32, device=new_xyz.device)
        pointnet2_stack_cuda.ball_query_wrapper(B, M, g.radius, g.nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx)
        row_start = pointnet2_stack_cuda._row_start(new_xyz_batch_cnt, xyz_batch_cnt, M)
        conv1, bn1, _, conv2, bn2, _ = list(self.mlps[k])
        return pointnet2_utils.sa_scale_train(xyz, features, new_xyz, idx, row_start, conv1.weight, bn1.weight, bn1.bias, conv2.weight, bn2.weight, bn2.bias,
                                              bn1.running_mean, bn1.running_var, bn1.num_batches_tracked, bn2.running_mean, bn2.running_var,
                                              bn2.num_batches_tracked, bn1.momentum, bn1.eps)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None, empty_voxel_set_zeros=True):
        outs = []
        xyz, new_xyz = xyz.contiguous(), new_xyz.contiguous()
        feats_c = features.contiguous() if features is not None else None
        for k in range(len(self.groupers)):
            if self._fused_ok(k, xyz, new_xyz, feats_c):
                outs.append(self._fused_scale(k, xyz, xyz_batch_cnt.contiguous(), new_xyz, new_xyz_batch_cnt.contiguous(), feats_c))
                continue
            if self._train_ok(k, xyz, new_xyz, feats_c):
                outs.append(self._train_scale(k, xyz, xyz_batch_cnt.contiguous(), new_xyz, new_xyz_batch_cnt.contiguous(), feats_c))
                continue
            grouped, _ = self.groupers[k](xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features)    # (M, C, nsample)
            x = self.mlps[k](grouped.permute(1, 0, 2).unsqueeze(dim=0))                               # (1, C', M, nsample)
            if self.pool_method == 'max_pool':
                x = F.max_pool2d(x, kernel_size=[1, x.size(3)]).squeeze(dim=-1)
            elif self.pool_method == 'avg_pool':
                x = F.avg_pool2d(x, kernel_size=[1, x.size(3)]).squeeze(dim=-1)
            else:
                raise NotImplementedError
            outs.append(x.squeeze(dim=0).permute(1, 0))                                               # (M, C')
        return new_xyz, torch.cat(outs, dim=1)


class VectorPoolLocalInterpolateModule(nn.Module):
    """Per local grid centre: the three nearest of the query's neighbours (HIP, one launch) -> inverse-distance interpolation of their
    features (+ the centre's offsets to the three).  Same constructor and forward as the reference (pointnet2_modules.py:160-244); the forward
    reads nothing back, so num_avg_length_of_neighbor_idxs stays what the constructor set."""

    def __init__(self, mlp, num_voxels, max_neighbour_distance, nsample, neighbor_type, use_xyz=True,
                 neighbour_distance_multiplier=1.0, xyz_encoding_type='concat'):
        super().__init__()
        self.num_voxels = num_voxels
        self.num_total_grids = self.num_voxels[0] * self.num_voxels[1] * self.num_voxels[2]
        self.max_neighbour_distance = max_neighbour_distance
        self.neighbor_distance_multiplier = neighbour_distance_multiplier
        self.nsample = nsample
        self.neighbor_type = neighbor_type
        self.use_xyz = use_xyz
        self.xyz_encoding_type = xyz_encoding_type
        if mlp is not None:
            mlp = list(mlp)
            if self.use_xyz:
                mlp[0] += 9 if self.xyz_encoding_type == 'concat' else 0
            shared_mlps = []
            for k in range(len(mlp) - 1):
                shared_mlps.extend([nn.Conv2d(mlp[k], mlp[k + 1], kernel_size=1, bias=False), nn.BatchNorm2d(mlp[k + 1]), nn.ReLU()])
            self.mlp = nn.Sequential(*shared_mlps)
        else:
            self.mlp = None
        self.num_avg_length_of_neighbor_idxs = 1000

    def forward(self, support_xyz, support_features, xyz_batch_cnt, new_xyz, new_xyz_grid_centers, new_xyz_batch_cnt):
        """support_xyz (N, 3), support_features (N, C), new_xyz (M, 3), new_xyz_grid_centers (M, G, 3) -> (M * G, C (+9))"""
        with torch.no_grad():
            dist, idx, _ = pointnet2_utils.three_nn_for_vector_pool_by_two_step(
                support_xyz, xyz_batch_cnt, new_xyz, new_xyz_grid_centers, new_xyz_batch_cnt,
                self.max_neighbour_distance, self.nsample, self.neighbor_type,
                self.num_avg_length_of_neighbor_idxs, self.num_total_grids, self.neighbor_distance_multiplier)
        dist_recip = 1.0 / (dist + 1e-8)
        norm = torch.sum(dist_recip, dim=-1, keepdim=True)
        weight = dist_recip / torch.clamp_min(norm, min=1e-8)

        empty_mask = (idx.view(-1, 3)[:, 0] == -1)
        idx = idx.view(-1, 3).masked_fill(empty_mask[:, None], 0)                # idx.view(-1, 3)[empty_mask] = 0, without a host read

        interpolated_feats = pointnet2_utils.three_interpolate(support_features, idx, weight.view(-1, 3))
        interpolated_feats = interpolated_feats.view(new_xyz_grid_centers.shape[0], new_xyz_grid_centers.shape[1], -1)     # (M, G, C)
        if self.use_xyz:
            near_known_xyz = support_xyz[idx.long()].view(-1, 3, 3)
            local_xyz = (new_xyz_grid_centers.view(-1, 1, 3) - near_known_xyz).view(-1, new_xyz_grid_centers.shape[1], 9)
            if self.xyz_encoding_type == 'concat':
                interpolated_feats = torch.cat((interpolated_feats, local_xyz), dim=-1)                              # (M, G, C + 9)
            else:
                raise NotImplementedError
        new_features = interpolated_feats.view(-1, interpolated_feats.shape[-1])
        new_features = new_features.masked_fill(empty_mask[:, None], 0)          # new_features[empty_mask, :] = 0
        if self.mlp is not None:
            new_features = new_features.permute(1, 0)[None, :, :, None]
            new_features = self.mlp(new_features)
            new_features = new_features.squeeze(dim=0).squeeze(dim=-1).permute(1, 0)
        return new_features


class VectorPoolAggregationModule(nn.Module):
    """One scale of the vector-pool aggregation: channel groups summed to num_reduced_channels -> per local cell either an interpolated
    (`local_interpolation`) or a chosen (`voxel_random_choice`) support feature with its offsets -> grouped Conv1d (one group per cell) -> post
    MLPs.  Same constructor, submodule names and forward as the reference (pointnet2_modules.py:247-420).  `voxel_avg_pool` raises at
    construction: no configuration selects it.  A forward reads nothing back: num_mean_points_per_grid stays what the constructor set."""

    def __init__(self, input_channels, num_local_voxel=(3, 3, 3), local_aggregation_type='local_interpolation',
                 num_reduced_channels=30, num_channels_of_local_aggregation=32, post_mlps=(128,),
                 max_neighbor_distance=None, neighbor_nsample=-1, neighbor_type=0, neighbor_distance_multiplier=2.0):
        super().__init__()
        self.num_local_voxel = num_local_voxel
        self.total_voxels = self.num_local_voxel[0] * self.num_local_voxel[1] * self.num_local_voxel[2]
        self.local_aggregation_type = local_aggregation_type
        assert self.local_aggregation_type in ['local_interpolation', 'voxel_avg_pool', 'voxel_random_choice']
        if self.local_aggregation_type == 'voxel_avg_pool':
            raise NotImplementedError("VectorPoolAggregationModule: voxel_avg_pool is not built (no configuration selects it)")
        self.input_channels = input_channels
        self.num_reduced_channels = input_channels if num_reduced_channels is None else num_reduced_channels
        self.num_channels_of_local_aggregation = num_channels_of_local_aggregation
        self.max_neighbour_distance = max_neighbor_distance
        self.neighbor_nsample = neighbor_nsample
        self.neighbor_type = neighbor_type  # 1: ball, others: cube

        if self.local_aggregation_type == 'local_interpolation':
            self.local_interpolate_module = VectorPoolLocalInterpolateModule(
                mlp=None, num_voxels=self.num_local_voxel, max_neighbour_distance=self.max_neighbour_distance,
                nsample=self.neighbor_nsample, neighbor_type=self.neighbor_type,
                neighbour_distance_multiplier=neighbor_distance_multiplier)
            num_c_in = (self.num_reduced_channels + 9) * self.total_voxels
        else:
            self.local_interpolate_module = None
            num_c_in = (self.num_reduced_channels + 3) * self.total_voxels
        num_c_out = self.total_voxels * self.num_channels_of_local_aggregation

        self.separate_local_aggregation_layer = nn.Sequential(
            nn.Conv1d(num_c_in, num_c_out, kernel_size=1, groups=self.total_voxels, bias=False), nn.BatchNorm1d(num_c_out), nn.ReLU())
        post_mlp_list = []
        c_in = num_c_out
        for cur_num_c in post_mlps:
            post_mlp_list.extend([nn.Conv1d(c_in, cur_num_c, kernel_size=1, bias=False), nn.BatchNorm1d(cur_num_c), nn.ReLU()])
            c_in = cur_num_c
        self.post_mlps = nn.Sequential(*post_mlp_list)

        self.num_mean_points_per_grid = 20
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d) or isinstance(m, nn.Conv1d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, nn.BatchNorm2d) or isinstance(m, nn.BatchNorm1d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def extra_repr(self) -> str:
        return (f'radius={self.max_neighbour_distance}, local_voxels=({self.num_local_voxel}, '
                f'local_aggregation_type={self.local_aggregation_type}, '
                f'num_c_reduction={self.input_channels}->{self.num_reduced_channels}, '
                f'num_c_local_aggregation={self.num_channels_of_local_aggregation}')

    def vector_pool_with_voxel_query(self, xyz, xyz_batch_cnt, features, new_xyz, new_xyz_batch_cnt):
        use_xyz = 1
        pooling_type = 0 if self.local_aggregation_type == 'voxel_avg_pool' else 1
        new_features, new_local_xyz, _, point_cnt_of_grid = pointnet2_utils.vector_pool_with_voxel_query_op(
            xyz, xyz_batch_cnt, features, new_xyz, new_xyz_batch_cnt,
            self.num_local_voxel[0], self.num_local_voxel[1], self.num_local_voxel[2],
            self.max_neighbour_distance, self.num_reduced_channels, use_xyz,
            self.num_mean_points_per_grid, self.neighbor_nsample, self.neighbor_type, pooling_type)
        num_new_pts = new_features.shape[0]
        new_local_xyz = new_local_xyz.view(num_new_pts, -1, 3)                      # (M, G, 3)
        new_features = new_features.view(num_new_pts, -1, self.num_reduced_channels)  # (M, G, C)
        new_features = torch.cat((new_local_xyz, new_features), dim=-1).view(num_new_pts, -1)
        return new_features, point_cnt_of_grid

    @staticmethod
    def get_dense_voxels_by_center(point_centers, max_neighbour_distance, num_voxels):
        """point_centers (N, 3) -> voxel_centers (N, total_voxels, 3)"""
        R = max_neighbour_distance
        device = point_centers.device
        x_grids = torch.arange(-R + R / num_voxels[0], R - R / num_voxels[0] + 1e-5, 2 * R / num_voxels[0], device=device)
        y_grids = torch.arange(-R + R / num_voxels[1], R - R / num_voxels[1] + 1e-5, 2 * R / num_voxels[1], device=device)
        z_grids = torch.arange(-R + R / num_voxels[2], R - R / num_voxels[2] + 1e-5, 2 * R / num_voxels[2], device=device)
        x_offset, y_offset, z_offset = torch.meshgrid(x_grids, y_grids, z_grids, indexing='ij')  # [num_x, num_y, num_z]
        xyz_offset = torch.cat((x_offset.contiguous().view(-1, 1), y_offset.contiguous().view(-1, 1), z_offset.contiguous().view(-1, 1)), dim=-1)
        return point_centers[:, None, :] + xyz_offset[None, :, :]

    def vector_pool_with_local_interpolate(self, xyz, xyz_batch_cnt, features, new_xyz, new_xyz_batch_cnt):
        """-> (M, total_voxels * (C + 9))"""
        voxel_centers = self.get_dense_voxels_by_center(
            point_centers=new_xyz, max_neighbour_distance=self.max_neighbour_distance, num_voxels=self.num_local_voxel)
        voxel_features = self.local_interpolate_module.forward(
            support_xyz=xyz, support_features=features, xyz_batch_cnt=xyz_batch_cnt,
            new_xyz=new_xyz, new_xyz_grid_centers=voxel_centers, new_xyz_batch_cnt=new_xyz_batch_cnt)
        return voxel_features.contiguous().view(-1, self.total_voxels * voxel_features.shape[-1])

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, **kwargs):
        """xyz (N, 3), new_xyz (M, 3), features (N, C) -> new_xyz, new_features (M, post_mlps[-1])"""
        N, C = features.shape
        assert C % self.num_reduced_channels == 0, \
            f'the input channels ({C}) should be an integral multiple of num_reduced_channels({self.num_reduced_channels})'
        features = features.view(N, -1, self.num_reduced_channels).sum(dim=1)

        if self.local_aggregation_type in ['voxel_avg_pool', 'voxel_random_choice']:
            vector_features, point_cnt_of_grid = self.vector_pool_with_voxel_query(
                xyz=xyz, xyz_batch_cnt=xyz_batch_cnt, features=features, new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt)
        elif self.local_aggregation_type == 'local_interpolation':
            vector_features = self.vector_pool_with_local_interpolate(
                xyz=xyz, xyz_batch_cnt=xyz_batch_cnt, features=features, new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt)
        else:
            raise NotImplementedError
        vector_features = vector_features.permute(1, 0)[None, :, :]                # (1, num_voxels * C, M)
        new_features = self.separate_local_aggregation_layer(vector_features)
        new_features = self.post_mlps(new_features)
        new_features = new_features.squeeze(dim=0).permute(1, 0)
        return new_xyz, new_features


class VectorPoolAggregationModuleMSG(nn.Module):
    """NUM_GROUPS VectorPoolAggregationModule scales (layer_{k}) over the same inputs, concatenated behind the query xyz -> msg_post_mlps.
    Same constructor, submodule names and keyword-only forward as the reference (pointnet2_modules.py:423-470)."""

    def __init__(self, input_channels, config):
        super().__init__()
        self.model_cfg = config
        self.num_groups = _cfg(config, 'NUM_GROUPS')
        c_in = 0
        for k in range(self.num_groups):
            cur_config = _cfg(config, f'GROUP_CFG_{k}')
            cur_vector_pool_module = VectorPoolAggregationModule(
                input_channels=input_channels, num_local_voxel=_cfg(cur_config, 'NUM_LOCAL_VOXEL'),
                post_mlps=_cfg(cur_config, 'POST_MLPS'),
                max_neighbor_distance=_cfg(cur_config, 'MAX_NEIGHBOR_DISTANCE'),
                neighbor_nsample=_cfg(cur_config, 'NEIGHBOR_NSAMPLE'),
                local_aggregation_type=_cfg(config, 'LOCAL_AGGREGATION_TYPE'),
                num_reduced_channels=_cfg(config, 'NUM_REDUCED_CHANNELS', None),
                num_channels_of_local_aggregation=_cfg(config, 'NUM_CHANNELS_OF_LOCAL_AGGREGATION'),
                neighbor_distance_multiplier=2.0)
            self.__setattr__(f'layer_{k}', cur_vector_pool_module)
            c_in += _cfg(cur_config, 'POST_MLPS')[-1]
        c_in += 3  # use_xyz
        shared_mlps = []
        for cur_num_c in _cfg(config, 'MSG_POST_MLPS'):
            shared_mlps.extend([nn.Conv1d(c_in, cur_num_c, kernel_size=1, bias=False), nn.BatchNorm1d(cur_num_c), nn.ReLU()])
            c_in = cur_num_c
        self.msg_post_mlps = nn.Sequential(*shared_mlps)

    def forward(self, **kwargs):
        features_list = []
        for k in range(self.num_groups):
            cur_xyz, cur_features = self.__getattr__(f'layer_{k}')(**kwargs)
            features_list.append(cur_features)
        features = torch.cat(features_list, dim=-1)
        features = torch.cat((cur_xyz, features), dim=-1)
        features = features.permute(1, 0)[None, :, :]  # (1, C, M)
        new_features = self.msg_post_mlps(features)
        new_features = new_features.squeeze(dim=0).permute(1, 0)  # (M, C)
        return cur_xyz, new_features
