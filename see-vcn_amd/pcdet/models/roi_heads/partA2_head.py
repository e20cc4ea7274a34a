import torch
import torch.nn as nn

from .... import _lib
from ...ops.roiaware_pool3d import roiaware_pool3d_utils
from ...utils import common_utils
from ...utils.common_utils import cfg_get
from ...utils.spconv_utils import spconv
from .roi_head_template import RoIHeadTemplate


class PartA2FCHead(RoIHeadTemplate):
    """Part-A2's RoI head (reference roi_heads/partA2_head.py:10-224): RoI-aware pooling of the part locations (avg) and the UNet's point
    features (max) into a pool^3 grid per RoI, two submanifold convolutions on each, their dense volume through the shared FC stack, cls / reg
    branches.  Same submodule names and state_dict keys.  When the points are stacked scene after scene (UNetV2's are), ONE assignment launch
    serves the RoIs of every scene and both feature sets (RoIAwarePool3d.forward_multi); otherwise the reference's per-scene loop runs."""

    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.model_cfg = model_cfg
        pool_cfg = cfg_get(model_cfg, 'ROI_AWARE_POOL')
        self.SA_modules = nn.ModuleList()
        block = self.post_act_block
        c0 = pool_cfg['NUM_FEATURES'] // 2
        self.conv_part = spconv.SparseSequential(block(4, 64, 3, padding=1, indice_key='rcnn_subm1'),
                                                 block(64, c0, 3, padding=1, indice_key='rcnn_subm1_1'))
        self.conv_rpn = spconv.SparseSequential(block(input_channels, 64, 3, padding=1, indice_key='rcnn_subm2'),
                                                block(64, c0, 3, padding=1, indice_key='rcnn_subm1_2'))
        pool_size = pool_cfg['POOL_SIZE']
        pre_channel = pool_cfg['NUM_FEATURES'] * pool_size * pool_size * pool_size
        shared_fc, dp = cfg_get(model_cfg, 'SHARED_FC'), cfg_get(model_cfg, 'DP_RATIO')
        shared_fc_list = []
        for k, c in enumerate(shared_fc):
            shared_fc_list += [nn.Conv1d(pre_channel, c, kernel_size=1, bias=False), nn.BatchNorm1d(c), nn.ReLU()]
            pre_channel = c
            if k != len(shared_fc) - 1 and dp > 0:
                shared_fc_list.append(nn.Dropout(dp))
        self.shared_fc_layer = nn.Sequential(*shared_fc_list)
        self.cls_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.num_class, fc_list=cfg_get(model_cfg, 'CLS_FC'))
        self.reg_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.box_coder.code_size * self.num_class,
                                              fc_list=cfg_get(model_cfg, 'REG_FC'))
        self.roiaware_pool3d_layer = roiaware_pool3d_utils.RoIAwarePool3d(out_size=pool_size, max_pts_each_voxel=pool_cfg['MAX_POINTS_PER_VOXEL'])
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

    @staticmethod
    def post_act_block(in_channels, out_channels, kernel_size, indice_key, stride=1, padding=0, conv_type='subm'):
        if conv_type == 'subm':
            conv = spconv.SubMConv3d(in_channels, out_channels, kernel_size, bias=False, indice_key=indice_key)
        elif conv_type == 'spconv':
            conv = spconv.SparseConv3d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=False, indice_key=indice_key)
        elif conv_type == 'inverseconv':
            conv = spconv.SparseInverseConv3d(in_channels, out_channels, kernel_size, indice_key=indice_key, bias=False)
        else:
            raise NotImplementedError
        return spconv.SparseSequential(conv, nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01), nn.ReLU())

    def roiaware_pool(self, batch_dict):
        """rois (B, num_rois, 7 + C), point_coords (num_points, 4) [bs_idx, x, y, z], point_features, point_cls_scores, point_part_offset ->
        pooled part features (B * num_rois, p, p, p, 4) (avg) and pooled point features (B * num_rois, p, p, p, C) (max)"""
        batch_size = batch_dict['batch_size']
        batch_idx = batch_dict['point_coords'][:, 0]
        point_coords = batch_dict['point_coords'][:, 1:4]
        point_features = batch_dict['point_features']
        part_src = batch_dict['point_part_offset'] if not cfg_get(self.model_cfg, 'DISABLE_PART', False) else point_coords
        scores = batch_dict['point_cls_scores'].view(-1, 1).detach()
        keep = (scores >= cfg_get(self.model_cfg, 'SEG_MASK_SCORE_THRESH')).to(part_src.dtype)   # a select, not a masked assignment (no host read)
        part_features = torch.cat((part_src * keep, scores), dim=1)
        rois = batch_dict['rois']
        n_pts, num_rois = point_coords.shape[0], rois.shape[1]
        # scene counts, and whether the rows are stacked scene after scene, with ONE device -> host read
        cnt = common_utils.batch_counts(batch_idx.long(), batch_size)
        sorted_flag = (batch_idx[1:] >= batch_idx[:-1]).all().to(torch.int32).view(1) if n_pts > 1 else torch.ones(1, dtype=torch.int32, device=rois.device)
        vals = _lib.host_ints([sorted_flag, cnt.to(torch.int32)])
        if vals[0]:
            ends, ranges = 0, []
            for c in vals[1:]:
                ranges += [[ends, ends + c]] * num_rois
                ends += c
            box_pt_range = torch.tensor(ranges, dtype=torch.int32).view(-1, 2).to(rois.device, non_blocking=True)
            pooled_part, pooled_rpn = self.roiaware_pool3d_layer.forward_multi(
                rois[..., 0:7].reshape(-1, 7).contiguous(), point_coords.contiguous(), [part_features, point_features], ['avg', 'max'], box_pt_range)
            return pooled_part, pooled_rpn
        part_list, rpn_list = [], []                                       # scenes interleaved: the reference's loop (:131-146)
        for bs_idx in range(batch_size):
            bs_mask = batch_idx == bs_idx
            cur_roi = rois[bs_idx][:, 0:7].contiguous()
            part_list.append(self.roiaware_pool3d_layer(cur_roi, point_coords[bs_mask], part_features[bs_mask], pool_method='avg'))
            rpn_list.append(self.roiaware_pool3d_layer(cur_roi, point_coords[bs_mask], point_features[bs_mask], pool_method='max'))
        return torch.cat(part_list, dim=0), torch.cat(rpn_list, dim=0)

    @staticmethod
    def fake_sparse_idx(sparse_idx, batch_size_rcnn):
        """At most two cells are non-empty: BatchNorm needs two values a channel, so the first cell of every RoI stands in (:153-161)."""
        zeros = sparse_idx.new_zeros((batch_size_rcnn, 3))
        bs_idxs = torch.arange(batch_size_rcnn).type_as(sparse_idx).view(-1, 1)
        return torch.cat((bs_idxs, zeros), dim=1)

    def forward(self, batch_dict):
        nms_cfg = cfg_get(self.model_cfg, 'NMS_CONFIG')['TRAIN' if self.training else 'TEST']
        targets_dict = self.proposal_layer(batch_dict, nms_config=nms_cfg)
        if self.training:
            targets_dict = self.assign_targets(batch_dict)
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']
        pooled_part_features, pooled_rpn_features = self.roiaware_pool(batch_dict)
        batch_size_rcnn = pooled_part_features.shape[0]                    # (B * N, out_x, out_y, out_z, 4)
        sparse_shape = [int(s) for s in pooled_part_features.shape[1:4]]
        sparse_idx = pooled_part_features.sum(dim=-1).nonzero()            # (non_empty_num, 4) [bs_idx, x_idx, y_idx, z_idx]
        if sparse_idx.shape[0] < 3:
            sparse_idx = self.fake_sparse_idx(sparse_idx, batch_size_rcnn)
            if self.training:                                              # these are invalid samples
                targets_dict['rcnn_cls_labels'].fill_(-1)
                targets_dict['reg_valid_mask'].fill_(-1)
        part_features = pooled_part_features[sparse_idx[:, 0], sparse_idx[:, 1], sparse_idx[:, 2], sparse_idx[:, 3]]
        rpn_features = pooled_rpn_features[sparse_idx[:, 0], sparse_idx[:, 1], sparse_idx[:, 2], sparse_idx[:, 3]]
        coords = sparse_idx.int().contiguous()
        part_features = spconv.SparseConvTensor(part_features, coords, sparse_shape, batch_size_rcnn)
        rpn_features = spconv.SparseConvTensor(rpn_features, coords, sparse_shape, batch_size_rcnn)
        x_part = self.conv_part(part_features)
        x_rpn = self.conv_rpn(rpn_features)
        merged_feature = torch.cat((x_rpn.features, x_part.features), dim=1)
        shared_feature = spconv.SparseConvTensor(merged_feature, coords, sparse_shape, batch_size_rcnn).dense().reshape(batch_size_rcnn, -1)
        shared_feature = self.run_fc(self.shared_fc_layer, shared_feature)
        rcnn_cls = self.run_fc(self.cls_layers, shared_feature)            # (B * N, 1 or num_class)
        rcnn_reg = self.run_fc(self.reg_layers, shared_feature)            # (B * N, code_size * num_class)
        if not self.training:
            batch_dict['batch_cls_preds'], batch_dict['batch_box_preds'] = self.generate_predicted_boxes(
                batch_size=batch_dict['batch_size'], rois=batch_dict['rois'], cls_preds=rcnn_cls, box_preds=rcnn_reg)
            batch_dict['cls_preds_normalized'] = False
        else:
            targets_dict['rcnn_cls'], targets_dict['rcnn_reg'] = rcnn_cls, rcnn_reg
            self.forward_ret_dict = targets_dict
        return batch_dict
