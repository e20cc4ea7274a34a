import torch
import torch.nn as nn

from ...ops.pointnet2.pointnet2_batch import pointnet2_modules
from ...utils import common_utils
from ...utils.common_utils import cfg_get


class PointNet2MSG(nn.Module):
    """PointRCNN's backbone (reference backbones_3d/pointnet2_backbone.py:9-94): multi-scale-grouping set abstraction down, feature
    propagation up, on the dense-batch layout -- every scene of the batch holds the same number of points.  Same submodule names
    (SA_modules, FP_modules) and state_dict keys.  The points-per-scene count comes from batch_dict['points_per_scene'] (a host list that
    collate_batch writes) when present, else from ONE batched count and one read; the reference loops a per-scene .sum() with a read each."""

    def __init__(self, model_cfg, input_channels, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        sa_cfg = cfg_get(model_cfg, 'SA_CONFIG')
        fp_mlps = cfg_get(model_cfg, 'FP_MLPS')
        self.SA_modules = nn.ModuleList()
        channel_in = input_channels - 3
        skip_channel_list = [input_channels - 3]
        for k in range(len(sa_cfg['NPOINTS'])):
            mlps = [[channel_in] + list(m) for m in sa_cfg['MLPS'][k]]      # fresh lists: the config's own are not edited
            channel_out = sum(m[-1] for m in mlps)
            self.SA_modules.append(pointnet2_modules.PointnetSAModuleMSG(
                npoint=sa_cfg['NPOINTS'][k], radii=sa_cfg['RADIUS'][k], nsamples=sa_cfg['NSAMPLE'][k], mlps=mlps,
                use_xyz=cfg_get(sa_cfg, 'USE_XYZ', True)))
            skip_channel_list.append(channel_out)
            channel_in = channel_out
        self.FP_modules = nn.ModuleList()
        for k in range(len(fp_mlps)):
            pre_channel = fp_mlps[k + 1][-1] if k + 1 < len(fp_mlps) else channel_out
            self.FP_modules.append(pointnet2_modules.PointnetFPModule(mlp=[pre_channel + skip_channel_list[k]] + list(fp_mlps[k])))
        self.num_point_features = fp_mlps[0][-1]

    @staticmethod
    def break_up_pc(pc):
        batch_idx = pc[:, 0]
        xyz = pc[:, 1:4].contiguous()
        features = pc[:, 4:].contiguous() if pc.size(-1) > 4 else None
        return batch_idx, xyz, features

    @staticmethod
    def equal_scene_size(batch_dict, batch_idx, batch_size):
        """The number of points every scene holds; unequal scenes are an error (the reference asserts, :76)."""
        counts = batch_dict.get('points_per_scene')
        if counts is None:
            counts = common_utils.batch_counts(batch_idx.long(), batch_size).tolist()      # one batched count, one read
        counts = [int(c) for c in counts]
        if len(counts) != batch_size or min(counts) != max(counts) or counts[0] * batch_size != batch_idx.shape[0]:
            raise ValueError(f"PointNet2MSG needs the same number of points in every scene, got {counts}: run the dataset's sample_points "
                             f"processor (NUM_POINTS) in front of the model")
        return counts[0]

    def forward(self, batch_dict):
        """batch_dict: batch_size, points (num_points, 4 + C) [batch_idx, x, y, z, ...] stacked scene after scene ->
        point_features (num_points, C_out), point_coords (num_points, 4)"""
        batch_size = batch_dict['batch_size']
        batch_idx, xyz, features = self.break_up_pc(batch_dict['points'])
        n = self.equal_scene_size(batch_dict, batch_idx, batch_size)
        xyz = xyz.view(batch_size, n, 3)
        features = features.view(batch_size, n, features.shape[-1]).permute(0, 2, 1).contiguous() if features is not None else None
        l_xyz, l_features = [xyz], [features]
        for sa in self.SA_modules:
            li_xyz, li_features = sa(l_xyz[-1], l_features[-1])
            l_xyz.append(li_xyz)
            l_features.append(li_features)
        for i in range(-1, -(len(self.FP_modules) + 1), -1):
            l_features[i - 1] = self.FP_modules[i](l_xyz[i - 1], l_xyz[i], l_features[i - 1], l_features[i])     # (B, C, N)
        point_features = l_features[0].permute(0, 2, 1).contiguous()                                             # (B, N, C)
        batch_dict['point_features'] = point_features.view(-1, point_features.shape[-1])
        batch_dict['point_coords'] = torch.cat((batch_idx[:, None].float(), l_xyz[0].view(-1, 3)), dim=1)
        batch_dict['point_coords_per_scene'] = n
        return batch_dict
