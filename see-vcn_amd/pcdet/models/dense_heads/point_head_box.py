import torch

from ...utils import box_coder_utils, box_utils
from ...utils.common_utils import cfg_get
from .point_head_template import PointHeadTemplate


class PointHeadBox(PointHeadTemplate):
    """PointRCNN's first stage (reference dense_heads/point_head_box.py:7-115): per point a class score and a box coded against the point
    (PointResidualCoder); the decoded boxes are the second stage's proposals.  Same submodule names (cls_layers, box_layers)."""

    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.predict_boxes_when_training = predict_boxes_when_training
        self.cls_layers = self.make_fc_layers(fc_cfg=cfg_get(model_cfg, 'CLS_FC'), input_channels=input_channels, output_channels=num_class)
        target_cfg = cfg_get(model_cfg, 'TARGET_CONFIG')
        self.box_coder = getattr(box_coder_utils, cfg_get(target_cfg, 'BOX_CODER'))(**cfg_get(target_cfg, 'BOX_CODER_CONFIG'))
        self.box_layers = self.make_fc_layers(fc_cfg=cfg_get(model_cfg, 'REG_FC'), input_channels=input_channels,
                                              output_channels=self.box_coder.code_size)

    def assign_targets(self, input_dict):
        point_coords, gt_boxes = input_dict['point_coords'], input_dict['gt_boxes']
        assert gt_boxes.dim() == 3, 'gt_boxes.shape=%s' % str(gt_boxes.shape)
        assert point_coords.dim() == 2, 'points.shape=%s' % str(point_coords.shape)
        batch_size = gt_boxes.shape[0]
        extend = box_utils.enlarge_box3d(gt_boxes.view(-1, gt_boxes.shape[-1]),
                                         extra_width=cfg_get(self.model_cfg, 'TARGET_CONFIG')['GT_EXTRA_WIDTH']).view(batch_size, -1, gt_boxes.shape[-1])
        return self.assign_stack_targets(points=point_coords, gt_boxes=gt_boxes, extend_gt_boxes=extend, set_ignore_flag=True,
                                         points_per_scene=input_dict.get('point_coords_per_scene'), ret_box_labels=True)

    def get_loss(self, tb_dict=None):
        tb_dict = {} if tb_dict is None else tb_dict
        point_loss_cls, tb_dict = self.get_cls_layer_loss(tb_dict)
        point_loss_box, tb_dict = self.get_box_layer_loss(tb_dict)
        return point_loss_cls + point_loss_box, tb_dict

    def forward(self, batch_dict):
        from .... import dense_ops
        key = 'point_features_before_fusion' if cfg_get(self.model_cfg, 'USE_POINT_FEATURES_BEFORE_FUSION', False) else 'point_features'
        point_features = batch_dict[key]
        point_cls_preds = dense_ops.run_sequential(self.cls_layers, point_features)            # (total_points, num_class)
        point_box_preds = dense_ops.run_sequential(self.box_layers, point_features)            # (total_points, code_size)
        batch_dict['point_cls_scores'] = torch.sigmoid(point_cls_preds.max(dim=-1)[0])
        ret_dict = {'point_cls_preds': point_cls_preds, 'point_box_preds': point_box_preds}
        if self.training:
            targets_dict = self.assign_targets(batch_dict)
            ret_dict['point_cls_labels'] = targets_dict['point_cls_labels']
            ret_dict['point_box_labels'] = targets_dict['point_box_labels']
        if not self.training or self.predict_boxes_when_training:
            batch_dict['batch_cls_preds'], batch_dict['batch_box_preds'] = self.generate_predicted_boxes(
                points=batch_dict['point_coords'][:, 1:4], point_cls_preds=point_cls_preds, point_box_preds=point_box_preds)
            batch_dict['batch_index'] = batch_dict['point_coords'][:, 0]
            batch_dict['cls_preds_normalized'] = False
        self.forward_ret_dict = ret_dict
        return batch_dict
