import torch

from ...utils import box_utils
from ...utils.common_utils import cfg_get
from .point_head_template import PointHeadTemplate


class PointIntraPartOffsetHead(PointHeadTemplate):
    """Part-A2's point head (reference dense_heads/point_intra_part_head.py:7-127): per point a foreground score and the intra-object part
    location (where in its box the point lies, per axis in [0, 1]).  Same submodule names; the box branch of PartA2_free (BOX_CODER in
    TARGET_CONFIG) is not built."""

    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.predict_boxes_when_training = predict_boxes_when_training
        self.cls_layers = self.make_fc_layers(fc_cfg=cfg_get(model_cfg, 'CLS_FC'), input_channels=input_channels, output_channels=num_class)
        self.part_reg_layers = self.make_fc_layers(fc_cfg=cfg_get(model_cfg, 'PART_FC'), input_channels=input_channels, output_channels=3)
        if cfg_get(cfg_get(model_cfg, 'TARGET_CONFIG'), 'BOX_CODER', None) is not None:
            raise NotImplementedError("PointIntraPartOffsetHead with a BOX_CODER (PartA2_free's point box branch) is not built")
        self.box_layers = None

    def assign_targets(self, input_dict):
        point_coords, gt_boxes = input_dict['point_coords'], input_dict['gt_boxes']
        assert gt_boxes.dim() == 3, 'gt_boxes.shape=%s' % str(gt_boxes.shape)
        assert point_coords.dim() == 2, 'points.shape=%s' % str(point_coords.shape)
        batch_size = gt_boxes.shape[0]
        extend = box_utils.enlarge_box3d(gt_boxes.view(-1, gt_boxes.shape[-1]),
                                         extra_width=cfg_get(self.model_cfg, 'TARGET_CONFIG')['GT_EXTRA_WIDTH']).view(batch_size, -1, gt_boxes.shape[-1])
        return self.assign_stack_targets(points=point_coords, gt_boxes=gt_boxes, extend_gt_boxes=extend, set_ignore_flag=True, ret_part_labels=True)

    def get_loss(self, tb_dict=None):
        tb_dict = {} if tb_dict is None else tb_dict
        point_loss_cls, tb_dict = self.get_cls_layer_loss(tb_dict)
        point_loss_part, tb_dict = self.get_part_layer_loss(tb_dict)
        return point_loss_cls + point_loss_part, tb_dict

    def forward(self, batch_dict):
        from .... import dense_ops
        point_features = batch_dict['point_features']
        point_cls_preds = dense_ops.run_sequential(self.cls_layers, point_features)            # (total_points, num_class)
        point_part_preds = dense_ops.run_sequential(self.part_reg_layers, point_features)      # (total_points, 3)
        ret_dict = {'point_cls_preds': point_cls_preds, 'point_part_preds': point_part_preds}
        batch_dict['point_cls_scores'], _ = torch.sigmoid(point_cls_preds).max(dim=-1)
        batch_dict['point_part_offset'] = torch.sigmoid(point_part_preds)
        if self.training:
            targets_dict = self.assign_targets(batch_dict)
            ret_dict['point_cls_labels'] = targets_dict['point_cls_labels']
            ret_dict['point_part_labels'] = targets_dict.get('point_part_labels')
            ret_dict['point_box_labels'] = targets_dict.get('point_box_labels')
        self.forward_ret_dict = ret_dict
        return batch_dict
