import os

import torch
import torch.nn as nn

from ...ops.pointnet2.pointnet2_batch import pointnet2_modules
from ...ops.roipoint_pool3d import roipoint_pool3d_utils
from ...utils import common_utils
from ...utils.common_utils import cfg_get
from .roi_head_template import RoIHeadTemplate


def fused_roipoint():
    """SEEVCN_FUSED_ROIPOINT=0: the reference's statement sequence (reference-shaped pooling, then subtract the centre, rotate, zero by flag)
    instead of the one fused launch -- for A/B runs and tests.  Read at every call."""
    return os.environ.get('SEEVCN_FUSED_ROIPOINT', '1') != '0'


class PointRCNNHead(RoIHeadTemplate):
    """PointRCNN's second stage (reference roi_heads/pointrcnn_head.py:10-179): the points inside every RoI (512 of them, repeated when
    fewer) with their score, depth and backbone features, moved to the RoI's frame, through three set-abstraction layers down to one feature
    vector, cls / reg branches.  Same submodule names and state_dict keys.  The pooling, the move to the RoI's frame and the zeros of empty
    RoIs are ONE launch (sv_roipoint_pool3d, canonical = 1) where the reference makes four passes over the pooled tensor."""

    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.model_cfg = model_cfg
        use_bn = cfg_get(model_cfg, 'USE_BN')
        sa_cfg = cfg_get(model_cfg, 'SA_CONFIG')
        pool_cfg = cfg_get(model_cfg, 'ROI_POINT_POOL')
        self.SA_modules = nn.ModuleList()
        channel_in = input_channels
        self.num_prefix_channels = 3 + 2                                    # xyz + point score + point depth
        xyz_mlps = [self.num_prefix_channels] + list(cfg_get(model_cfg, 'XYZ_UP_LAYER'))
        shared_mlps = []
        for c_in, c_out in zip(xyz_mlps[:-1], xyz_mlps[1:]):
            shared_mlps.append(nn.Conv2d(c_in, c_out, kernel_size=1, bias=not use_bn))
            if use_bn:
                shared_mlps.append(nn.BatchNorm2d(c_out))
            shared_mlps.append(nn.ReLU())
        self.xyz_up_layer = nn.Sequential(*shared_mlps)
        c_out = xyz_mlps[-1]
        self.merge_down_layer = nn.Sequential(nn.Conv2d(c_out * 2, c_out, kernel_size=1, bias=not use_bn),
                                              *([nn.BatchNorm2d(c_out), nn.ReLU()] if use_bn else [nn.ReLU()]))
        for k in range(len(sa_cfg['NPOINTS'])):
            mlps = [channel_in] + list(sa_cfg['MLPS'][k])
            npoint = sa_cfg['NPOINTS'][k] if sa_cfg['NPOINTS'][k] != -1 else None
            self.SA_modules.append(pointnet2_modules.PointnetSAModule(npoint=npoint, radius=sa_cfg['RADIUS'][k], nsample=sa_cfg['NSAMPLE'][k],
                                                                      mlp=mlps, use_xyz=True, bn=use_bn))
            channel_in = mlps[-1]
        self.cls_layers = self.make_fc_layers(input_channels=channel_in, output_channels=self.num_class, fc_list=cfg_get(model_cfg, 'CLS_FC'))
        self.reg_layers = self.make_fc_layers(input_channels=channel_in, output_channels=self.box_coder.code_size * self.num_class,
                                              fc_list=cfg_get(model_cfg, 'REG_FC'))
        self.roipoint_pool3d_layer = roipoint_pool3d_utils.RoIPointPool3d(num_sampled_points=pool_cfg['NUM_SAMPLED_POINTS'],
                                                                          pool_extra_width=pool_cfg['POOL_EXTRA_WIDTH'])
        self.init_weights(weight_init='xavier')

    def init_weights(self, weight_init='xavier'):
        init_func = {'kaiming': nn.init.kaiming_normal_, 'xavier': nn.init.xavier_normal_, 'normal': nn.init.normal_}[weight_init]
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                if weight_init == 'normal':
                    init_func(m.weight, mean=0, std=0.001)
                else:
                    init_func(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    def roipool3d_gpu(self, batch_dict):
        """rois (B, num_rois, 7 + C), point_coords (num_points, 4) [bs_idx, x, y, z] with equally many points per scene, stacked scene after
        scene, point_features (num_points, C), point_cls_scores (num_points) -> (B * num_rois, num_sampled_points, 3 + 2 + C): the RoI's points
        in its frame | score | depth | features, zeros for an RoI without points"""
        batch_size = batch_dict['batch_size']
        point_coords = batch_dict['point_coords'][:, 1:4]
        point_features = batch_dict['point_features']
        rois = batch_dict['rois']
        assert point_coords.shape[0] % batch_size == 0, "PointRCNNHead needs the same number of points in every scene"
        point_scores = batch_dict['point_cls_scores'].detach()
        point_depths = point_coords.norm(dim=1) / cfg_get(self.model_cfg, 'ROI_POINT_POOL')['DEPTH_NORMALIZER'] - 0.5
        point_features_all = torch.cat([point_scores[:, None], point_depths[:, None], point_features], dim=1)
        batch_points = point_coords.view(batch_size, -1, 3)
        batch_point_features = point_features_all.view(batch_size, -1, point_features_all.shape[-1])
        with torch.no_grad():
            if fused_roipoint():
                pooled_features, _ = self.roipoint_pool3d_layer(batch_points, batch_point_features, rois[..., 0:7], canonical=True)
                return pooled_features.view(-1, pooled_features.shape[-2], pooled_features.shape[-1])
            pooled_features, pooled_empty_flag = self.roipoint_pool3d_layer(batch_points, batch_point_features, rois[..., 0:7])
            pooled_features[:, :, :, 0:3] -= rois[:, :, 0:3].unsqueeze(dim=2)
            pooled_features = pooled_features.view(-1, pooled_features.shape[-2], pooled_features.shape[-1])
            pooled_features[:, :, 0:3] = common_utils.rotate_points_along_z(pooled_features[:, :, 0:3], -rois.view(-1, rois.shape[-1])[:, 6])
            pooled_features = torch.where(pooled_empty_flag.view(-1, 1, 1) > 0, torch.zeros_like(pooled_features), pooled_features)
        return pooled_features

    def forward(self, batch_dict):
        nms_cfg = cfg_get(self.model_cfg, 'NMS_CONFIG')['TRAIN' if self.training else 'TEST']
        targets_dict = self.proposal_layer(batch_dict, nms_config=nms_cfg)
        if self.training:
            targets_dict = self.assign_targets(batch_dict)
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']
        pooled_features = self.roipool3d_gpu(batch_dict)                   # (total_rois, num_sampled_points, 3 + 2 + C)
        xyz_input = pooled_features[..., 0:self.num_prefix_channels].transpose(1, 2).unsqueeze(dim=3).contiguous()
        xyz_features = self.xyz_up_layer(xyz_input)
        point_features = pooled_features[..., self.num_prefix_channels:].transpose(1, 2).unsqueeze(dim=3)
        merged_features = self.merge_down_layer(torch.cat((xyz_features, point_features), dim=1))
        l_xyz, l_features = [pooled_features[..., 0:3].contiguous()], [merged_features.squeeze(dim=3).contiguous()]
        for sa in self.SA_modules:
            li_xyz, li_features = sa(l_xyz[-1], l_features[-1])
            l_xyz.append(li_xyz)
            l_features.append(li_features)
        shared_features = l_features[-1].squeeze(dim=-1)                   # (total_rois, num_features)
        rcnn_cls = self.run_fc(self.cls_layers, shared_features)           # (total_rois, 1 or num_class)
        rcnn_reg = self.run_fc(self.reg_layers, shared_features)           # (total_rois, code_size * num_class)
        if not self.training:
            batch_dict['batch_cls_preds'], batch_dict['batch_box_preds'] = self.generate_predicted_boxes(
                batch_size=batch_dict['batch_size'], rois=batch_dict['rois'], cls_preds=rcnn_cls, box_preds=rcnn_reg)
            batch_dict['cls_preds_normalized'] = False
        else:
            targets_dict['rcnn_cls'], targets_dict['rcnn_reg'] = rcnn_cls, rcnn_reg
            self.forward_ret_dict = targets_dict
        return batch_dict
