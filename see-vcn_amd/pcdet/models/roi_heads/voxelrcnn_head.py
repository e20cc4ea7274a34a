import torch
import torch.nn as nn

from ...ops.pointnet2.pointnet2_stack import voxel_pool_modules as voxelpool_stack_modules
from ...ops.pointnet2.pointnet2_stack import voxel_query_utils
from ...utils import common_utils
from ...utils.common_utils import cfg_get
from .roi_head_template import RoIGridPointsMixin, RoIHeadTemplate


class VoxelRCNNHead(RoIGridPointsMixin, RoIHeadTemplate):
    """Voxel RoI pooling head of Voxel R-CNN (reference roi_heads/voxelrcnn_head.py:8-262): 6^3 grid points per RoI, a voxel query + pooling
    (NeighborVoxelSAModuleMSG) of every FEATURES_SOURCE tap of the sparse backbone around them, shared FC 216 * c_out -> 256 -> 256, cls / reg
    branches of Linear + BatchNorm1d + ReLU.  Same submodule names and state_dict keys; the config's MLPS lists are read, never edited, so one
    config builds the same head any number of times."""

    def __init__(self, backbone_channels, model_cfg, point_cloud_range, voxel_size, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.model_cfg = model_cfg
        self.pool_cfg = cfg_get(model_cfg, 'ROI_GRID_POOL')
        layer_cfg = cfg_get(self.pool_cfg, 'POOL_LAYERS')
        self.point_cloud_range = point_cloud_range
        self.voxel_size = voxel_size
        self.features_source = list(cfg_get(self.pool_cfg, 'FEATURES_SOURCE'))
        self.grid_size = cfg_get(self.pool_cfg, 'GRID_SIZE')

        c_out = 0
        self.roi_grid_pool_layers = nn.ModuleList()
        for src_name in self.features_source:
            cfg = layer_cfg[src_name]
            mlps = [[backbone_channels[src_name]] + list(m) for m in cfg_get(cfg, 'MLPS')]
            self.roi_grid_pool_layers.append(voxelpool_stack_modules.NeighborVoxelSAModuleMSG(
                query_ranges=cfg_get(cfg, 'QUERY_RANGES'), nsamples=cfg_get(cfg, 'NSAMPLE'), radii=cfg_get(cfg, 'POOL_RADIUS'), mlps=mlps,
                pool_method=cfg_get(cfg, 'POOL_METHOD')))
            c_out += sum(m[-1] for m in mlps)

        dp = cfg_get(model_cfg, 'DP_RATIO')

        def fc_stack(pre, widths, inplace=False):
            layers = []
            for k, c in enumerate(widths):
                layers += [nn.Linear(pre, c, bias=False), nn.BatchNorm1d(c), nn.ReLU(inplace=True) if inplace else nn.ReLU()]
                pre = c
                if k != len(widths) - 1 and dp > 0:
                    layers.append(nn.Dropout(dp))
            return nn.Sequential(*layers), pre

        self.shared_fc_layer, pre = fc_stack(self.grid_size ** 3 * c_out, cfg_get(model_cfg, 'SHARED_FC'), inplace=True)
        self.cls_fc_layers, pre_cls = fc_stack(pre, cfg_get(model_cfg, 'CLS_FC'))
        self.cls_pred_layer = nn.Linear(pre_cls, self.num_class, bias=True)
        self.reg_fc_layers, pre_reg = fc_stack(pre, cfg_get(model_cfg, 'REG_FC'))
        self.reg_pred_layer = nn.Linear(pre_reg, self.box_coder.code_size * self.num_class, bias=True)
        self.init_weights()

    def init_weights(self):
        for stack in (self.shared_fc_layer, self.cls_fc_layers, self.reg_fc_layers):
            for m in stack.modules():
                if isinstance(m, nn.Linear):
                    nn.init.xavier_normal_(m.weight)
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.cls_pred_layer.weight, 0, 0.01)
        nn.init.constant_(self.cls_pred_layer.bias, 0)
        nn.init.normal_(self.reg_pred_layer.weight, mean=0, std=0.001)
        nn.init.constant_(self.reg_pred_layer.bias, 0)

    def roi_grid_pool(self, batch_dict):
        """rois (B, num_rois, 7 + C) and the sparse taps of multi_scale_3d_features -> (B * num_rois, g^3, c_out)"""
        rois, batch_size = batch_dict['rois'], batch_dict['batch_size']
        with_vf_transform = batch_dict.get('with_voxel_feature_transform', False)
        roi_grid_xyz, _ = self.get_global_grid_points_of_roi(rois, grid_size=self.grid_size)
        roi_grid_xyz = roi_grid_xyz.view(batch_size, -1, 3)
        # the voxel each grid point falls in: floor division on floats, as the reference writes it; negative and out-of-volume cells are legal
        # (the query passes over what lies outside)
        roi_grid_coords = torch.cat([(roi_grid_xyz[:, :, a:a + 1] - self.point_cloud_range[a]) // self.voxel_size[a] for a in range(3)], dim=-1)
        batch_idx = torch.arange(batch_size, device=rois.device, dtype=rois.dtype).view(-1, 1, 1).expand(-1, roi_grid_coords.shape[1], 1)
        roi_grid_batch_cnt = torch.full((batch_size,), roi_grid_coords.shape[1], dtype=torch.int32, device=rois.device)
        new_xyz = roi_grid_xyz.contiguous().view(-1, 3)

        pooled_features_list = []
        for k, src_name in enumerate(self.features_source):
            cur_stride = batch_dict['multi_scale_3d_strides'][src_name]
            cur_sp_tensors = batch_dict['multi_scale_3d_features_post' if with_vf_transform else 'multi_scale_3d_features'][src_name]
            cur_coords = cur_sp_tensors.indices
            cur_voxel_xyz = common_utils.get_voxel_centers(cur_coords[:, 1:4], downsample_times=cur_stride, voxel_size=self.voxel_size,
                                                           point_cloud_range=self.point_cloud_range)
            cur_voxel_xyz_batch_cnt = common_utils.batch_counts(cur_coords[:, 0].long(), batch_size)
            cur_roi_grid_coords = torch.cat([batch_idx, roi_grid_coords // cur_stride], dim=-1).int()          # [b, x, y, z]
            with voxel_query_utils.borrowed_voxel2pinds(cur_sp_tensors) as v2p_ind_tensor:
                pooled_features = self.roi_grid_pool_layers[k](
                    xyz=cur_voxel_xyz.contiguous(), xyz_batch_cnt=cur_voxel_xyz_batch_cnt, new_xyz=new_xyz, new_xyz_batch_cnt=roi_grid_batch_cnt,
                    new_coords=cur_roi_grid_coords.contiguous().view(-1, 4), features=cur_sp_tensors.features.contiguous(),
                    voxel2point_indices=v2p_ind_tensor)
            pooled_features_list.append(pooled_features.view(-1, self.grid_size ** 3, pooled_features.shape[-1]))
        return torch.cat(pooled_features_list, dim=-1)

    @staticmethod
    def _predict(layer, x):
        """a prediction Linear on the library's GEMM, like the stacks in front of it (run_fc)"""
        from .... import dense_ops
        if x.is_cuda and x.dtype == torch.float32 and not dense_ops._has_hooks(layer):
            return dense_ops.linear(x, layer.weight, layer.bias)
        return layer(x)

    def forward(self, batch_dict):
        nms_cfg = cfg_get(self.model_cfg, 'NMS_CONFIG')['TRAIN' if self.training else 'TEST']
        targets_dict = self.proposal_layer(batch_dict, nms_config=nms_cfg)
        if self.training:
            targets_dict = self.assign_targets(batch_dict)
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']
        pooled_features = self.roi_grid_pool(batch_dict)                                              # (BxN, g^3, C)
        pooled_features = pooled_features.reshape(pooled_features.size(0), -1)
        shared_features = self.run_fc(self.shared_fc_layer, pooled_features)
        rcnn_cls = self._predict(self.cls_pred_layer, self.run_fc(self.cls_fc_layers, shared_features))
        rcnn_reg = self._predict(self.reg_pred_layer, self.run_fc(self.reg_fc_layers, shared_features))
        if not self.training:
            batch_dict['batch_cls_preds'], batch_dict['batch_box_preds'] = self.generate_predicted_boxes(
                batch_size=batch_dict['batch_size'], rois=batch_dict['rois'], cls_preds=rcnn_cls, box_preds=rcnn_reg)
            batch_dict['cls_preds_normalized'] = False
        else:
            targets_dict['rcnn_cls'], targets_dict['rcnn_reg'] = rcnn_cls, rcnn_reg
            self.forward_ret_dict = targets_dict
        return batch_dict
