import numpy as np
import torch
import torch.nn as nn

from ...utils import common_utils
from ...utils.common_utils import cfg_get
from ..backbones_2d import BaseBEVBackbone
from .anchor_head_template import AnchorHeadTemplate


def _middle_convs(c_in, num_middle_conv, num_middle_filter):
    layers = []
    for _ in range(num_middle_conv):
        layers += [nn.Conv2d(c_in, num_middle_filter, kernel_size=3, stride=1, padding=1, bias=False), nn.BatchNorm2d(num_middle_filter), nn.ReLU()]
        c_in = num_middle_filter
    return layers, c_in


class SingleHead(BaseBEVBackbone):
    """One head of AnchorHeadMulti (reference dense_heads/anchor_head_multi.py:9-148): same constructor, submodule names (conv_cls, conv_box
    as a Conv2d or a ModuleDict of `conv_<reg name>` towers, conv_dir_cls), buffer `head_label_indices` and returned keys.  It derives from
    BaseBEVBackbone with the head's own config (RPN_HEAD_CFGS entry: no LAYER_NUMS), whose forward then hands the map through."""

    def __init__(self, model_cfg, input_channels, num_class, num_anchors_per_location, code_size, rpn_head_cfg=None, head_label_indices=None,
                 separate_reg_config=None):
        super().__init__(rpn_head_cfg, input_channels)
        self.num_anchors_per_location = num_anchors_per_location
        self.num_class = num_class
        self.code_size = code_size
        self.model_cfg = model_cfg
        self.separate_reg_config = separate_reg_config
        self.register_buffer('head_label_indices', head_label_indices)
        if self.separate_reg_config is not None:
            code_size_cnt = 0
            self.conv_box = nn.ModuleDict()
            self.conv_box_names = []
            num_middle_conv = cfg_get(self.separate_reg_config, 'NUM_MIDDLE_CONV')
            num_middle_filter = cfg_get(self.separate_reg_config, 'NUM_MIDDLE_FILTER')
            layers, c_in = _middle_convs(input_channels, num_middle_conv, num_middle_filter)
            layers.append(nn.Conv2d(c_in, self.num_anchors_per_location * self.num_class, kernel_size=3, stride=1, padding=1))
            self.conv_cls = nn.Sequential(*layers)
            for reg_config in cfg_get(self.separate_reg_config, 'REG_LIST'):
                reg_name, reg_channel = reg_config.split(':')
                reg_channel = int(reg_channel)
                layers, c_in = _middle_convs(input_channels, num_middle_conv, num_middle_filter)
                layers.append(nn.Conv2d(c_in, self.num_anchors_per_location * reg_channel, kernel_size=3, stride=1, padding=1, bias=True))
                code_size_cnt += reg_channel
                self.conv_box[f'conv_{reg_name}'] = nn.Sequential(*layers)
                self.conv_box_names.append(f'conv_{reg_name}')
            for m in self.conv_box.modules():
                if isinstance(m, nn.Conv2d):
                    nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
            assert code_size_cnt == code_size, f'Code size does not match: {code_size_cnt}:{code_size}'
        else:
            self.conv_cls = nn.Conv2d(input_channels, self.num_anchors_per_location * self.num_class, kernel_size=1)
            self.conv_box = nn.Conv2d(input_channels, self.num_anchors_per_location * self.code_size, kernel_size=1)
        if cfg_get(self.model_cfg, 'USE_DIRECTION_CLASSIFIER', None) is not None:
            self.conv_dir_cls = nn.Conv2d(input_channels, self.num_anchors_per_location * cfg_get(self.model_cfg, 'NUM_DIR_BINS'), kernel_size=1)
        else:
            self.conv_dir_cls = None
        self.use_multihead = cfg_get(self.model_cfg, 'USE_MULTIHEAD', False)
        self.init_weights()

    def init_weights(self):
        pi = 0.01
        last = self.conv_cls if isinstance(self.conv_cls, nn.Conv2d) else self.conv_cls[-1]
        nn.init.constant_(last.bias, -np.log((1 - pi) / pi))

    def _rows(self, x, width):
        """(N, A_loc * width, H, W) -> multihead: (N, A_loc * H * W, width) in the order [slot, y, x]; else (N, H, W, A_loc * width)"""
        if not self.use_multihead:
            return x.permute(0, 2, 3, 1).contiguous()
        n, _, h, w = x.shape
        return x.reshape(-1, self.num_anchors_per_location, width, h, w).permute(0, 1, 3, 4, 2).contiguous().view(n, -1, width)

    def forward(self, spatial_features_2d):
        spatial_features_2d = super().forward({'spatial_features': spatial_features_2d})['spatial_features_2d']
        cls_preds = self.conv_cls(spatial_features_2d)
        if self.separate_reg_config is None:
            box_preds = self.conv_box(spatial_features_2d)
        else:
            box_preds = torch.cat([self.conv_box[name](spatial_features_2d) for name in self.conv_box_names], dim=1)
        ret_dict = {'cls_preds': self._rows(cls_preds, self.num_class), 'box_preds': self._rows(box_preds, self.code_size), 'dir_cls_preds': None}
        if self.conv_dir_cls is not None:
            ret_dict['dir_cls_preds'] = self._rows(self.conv_dir_cls(spatial_features_2d), cfg_get(self.model_cfg, 'NUM_DIR_BINS'))
        return ret_dict


class AnchorHeadMulti(AnchorHeadTemplate):
    """Drop-in for the reference AnchorHeadMulti (dense_heads/anchor_head_multi.py:151-373): same keywords, submodule names (shared_conv,
    rpn_heads.<i>...), forward_ret_dict / tb_dict / batch_dict keys.  Targets for all heads come from one pair of launches
    (sv_assign_targets_axis_aligned_coded on head-major anchors), the boxes of all heads from one (sv_anchor_decode_coded)."""

    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, predict_boxes_when_training=True, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class, class_names=class_names, grid_size=grid_size,
                         point_cloud_range=point_cloud_range, predict_boxes_when_training=predict_boxes_when_training)
        self.model_cfg = model_cfg
        self.separate_multihead = cfg_get(self.model_cfg, 'SEPARATE_MULTIHEAD', False)
        shared = cfg_get(self.model_cfg, 'SHARED_CONV_NUM_FILTER', None)
        if shared is not None:
            self.shared_conv = nn.Sequential(nn.Conv2d(input_channels, shared, 3, stride=1, padding=1, bias=False),
                                             nn.BatchNorm2d(shared, eps=1e-3, momentum=0.01), nn.ReLU())
        else:
            self.shared_conv = None
            shared = input_channels
        self.rpn_heads = None
        self.make_multihead(shared)

    def make_multihead(self, input_channels):
        rpn_head_cfgs = cfg_get(self.model_cfg, 'RPN_HEAD_CFGS')
        class_names = []
        for rpn_head_cfg in rpn_head_cfgs:
            class_names.extend(rpn_head_cfg['HEAD_CLS_NAME'])
        rpn_heads = []
        for rpn_head_cfg in rpn_head_cfgs:
            names = rpn_head_cfg['HEAD_CLS_NAME']
            num_anchors_per_location = sum(self.num_anchors_per_location[class_names.index(n)] for n in names)
            head_label_indices = torch.from_numpy(np.array([list(self.class_names).index(n) + 1 for n in names]))
            rpn_heads.append(SingleHead(self.model_cfg, input_channels, len(names) if self.separate_multihead else self.num_class,
                                        num_anchors_per_location, self.box_coder.code_size, rpn_head_cfg, head_label_indices=head_label_indices,
                                        separate_reg_config=cfg_get(self.model_cfg, 'SEPARATE_REG_CONFIG', None)))
        self.rpn_heads = nn.ModuleList(rpn_heads)

    def forward(self, data_dict):
        spatial_features_2d = data_dict['spatial_features_2d']
        if self.shared_conv is not None:
            spatial_features_2d = self.shared_conv(spatial_features_2d)
        ret_dicts = [rpn_head(spatial_features_2d) for rpn_head in self.rpn_heads]
        cls_preds = [r['cls_preds'] for r in ret_dicts]
        box_preds = [r['box_preds'] for r in ret_dicts]
        ret = {'cls_preds': cls_preds if self.separate_multihead else torch.cat(cls_preds, dim=1),
               'box_preds': box_preds if self.separate_multihead else torch.cat(box_preds, dim=1)}
        if cfg_get(self.model_cfg, 'USE_DIRECTION_CLASSIFIER', False):
            dir_cls_preds = [r['dir_cls_preds'] for r in ret_dicts]
            ret['dir_cls_preds'] = dir_cls_preds if self.separate_multihead else torch.cat(dir_cls_preds, dim=1)
        self.forward_ret_dict.update(ret)
        if self.training:
            self.forward_ret_dict.update(self.assign_targets(gt_boxes=data_dict['gt_boxes']))
        if not self.training or self.predict_boxes_when_training:
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(
                batch_size=data_dict['batch_size'], cls_preds=ret['cls_preds'], box_preds=ret['box_preds'], dir_cls_preds=ret.get('dir_cls_preds', None))
            if isinstance(batch_cls_preds, list):
                data_dict['multihead_label_mapping'] = [self.rpn_heads[i].head_label_indices for i in range(len(batch_cls_preds))]
            data_dict['batch_cls_preds'] = batch_cls_preds
            data_dict['batch_box_preds'] = batch_box_preds
            data_dict['cls_preds_normalized'] = False
        return data_dict

    def get_cls_layer_loss(self):
        loss_weights = cfg_get(self.model_cfg, 'LOSS_CONFIG')['LOSS_WEIGHTS']
        pos_cls_weight = neg_cls_weight = 1.0
        if 'pos_cls_weight' in loss_weights:
            pos_cls_weight, neg_cls_weight = loss_weights['pos_cls_weight'], loss_weights['neg_cls_weight']
        cls_preds = self.forward_ret_dict['cls_preds']
        box_cls_labels = self.forward_ret_dict['box_cls_labels']
        if not isinstance(cls_preds, list):
            cls_preds = [cls_preds]
        batch_size = int(cls_preds[0].shape[0])
        cared = box_cls_labels >= 0
        positives = box_cls_labels > 0
        negatives = box_cls_labels == 0
        cls_weights = (negatives * 1.0 * neg_cls_weight + pos_cls_weight * positives).float()
        if self.num_class == 1:
            box_cls_labels = torch.where(positives, torch.ones_like(box_cls_labels), box_cls_labels)  # class agnostic
        cls_weights = cls_weights / torch.clamp(positives.sum(1, keepdim=True).float(), min=1.0)
        cls_targets = (box_cls_labels * cared.type_as(box_cls_labels)).long()
        one_hot_targets = torch.zeros(*cls_targets.shape, self.num_class + 1, dtype=cls_preds[0].dtype, device=cls_targets.device)
        one_hot_targets.scatter_(-1, cls_targets.unsqueeze(-1), 1.0)
        one_hot_targets = one_hot_targets[..., 1:]
        start_idx = c_idx = 0
        cls_losses = 0
        for idx, cls_pred in enumerate(cls_preds):
            cur_num_class = self.rpn_heads[idx].num_class
            cls_pred = cls_pred.view(batch_size, -1, cur_num_class)
            stop_idx = start_idx + cls_pred.shape[1]
            if self.separate_multihead:
                one_hot_target = one_hot_targets[:, start_idx:stop_idx, c_idx:c_idx + cur_num_class]
                c_idx += cur_num_class
            else:
                one_hot_target = one_hot_targets[:, start_idx:stop_idx]
            cls_loss_src = self.cls_loss_func(cls_pred, one_hot_target.contiguous(), weights=cls_weights[:, start_idx:stop_idx].contiguous())
            cls_losses = cls_losses + cls_loss_src.sum() / batch_size * loss_weights['cls_weight']
            start_idx = stop_idx
        assert start_idx == one_hot_targets.shape[1]
        return cls_losses, {'rpn_loss_cls': common_utils.tb_value(cls_losses)}

    def get_box_reg_layer_loss(self):
        box_preds = self.forward_ret_dict['box_preds']
        box_dir_cls_preds = self.forward_ret_dict.get('dir_cls_preds', None)
        box_reg_targets = self.forward_ret_dict['box_reg_targets']
        box_cls_labels = self.forward_ret_dict['box_cls_labels']
        loss_weights = cfg_get(self.model_cfg, 'LOSS_CONFIG')['LOSS_WEIGHTS']
        positives = box_cls_labels > 0
        reg_weights = positives.float()
        reg_weights = reg_weights / torch.clamp(positives.sum(1, keepdim=True).float(), min=1.0)
        if not isinstance(box_preds, list):
            box_preds = [box_preds]
        batch_size = int(box_preds[0].shape[0])
        dir_targets = dir_weights = None
        if box_dir_cls_preds is not None:
            if not isinstance(box_dir_cls_preds, list):
                box_dir_cls_preds = [box_dir_cls_preds]
            nb = cfg_get(self.model_cfg, 'NUM_DIR_BINS')
            anchors = self._anchors_on(box_preds[0].device)
            anchors = anchors.view(1, -1, anchors.shape[-1]).repeat(batch_size, 1, 1)
            dir_targets = self.get_direction_target(anchors, box_reg_targets, dir_offset=cfg_get(self.model_cfg, 'DIR_OFFSET'), num_bins=nb)
            dir_weights = positives.type_as(box_dir_cls_preds[0])
            dir_weights = dir_weights / torch.clamp(dir_weights.sum(-1, keepdim=True), min=1.0)
        start_idx = 0
        box_losses = 0
        loc_total, dir_total = 0, 0
        for idx, box_pred in enumerate(box_preds):
            box_pred = box_pred.view(batch_size, -1, box_pred.shape[-1] // self.num_anchors_per_location if not self.use_multihead else box_pred.shape[-1])
            stop_idx = start_idx + box_pred.shape[1]
            box_reg_target = box_reg_targets[:, start_idx:stop_idx].contiguous()
            reg_weight = reg_weights[:, start_idx:stop_idx].contiguous()
            if box_dir_cls_preds is not None:                       # sin(a - b) = sin a cos b - cos a sin b
                box_pred, box_reg_target = self.add_sin_difference(box_pred, box_reg_target)
            loc_loss = self.reg_loss_func(box_pred, box_reg_target, weights=reg_weight).sum() / batch_size * loss_weights['loc_weight']
            box_losses = box_losses + loc_loss
            loc_total = loc_total + loc_loss
            if box_dir_cls_preds is not None:
                dir_logit = box_dir_cls_preds[idx].view(batch_size, -1, nb)
                dir_loss = self.dir_loss_func(dir_logit, dir_targets[:, start_idx:stop_idx], weights=dir_weights[:, start_idx:stop_idx])
                dir_loss = dir_loss.sum() / batch_size * loss_weights['dir_weight']
                box_losses = box_losses + dir_loss
                dir_total = dir_total + dir_loss
            start_idx = stop_idx
        tb_dict = {'rpn_loss_loc': common_utils.tb_value(loc_total)}
        if box_dir_cls_preds is not None:
            tb_dict['rpn_loss_dir'] = common_utils.tb_value(dir_total)
        return box_losses, tb_dict
