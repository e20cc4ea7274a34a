from ...utils.common_utils import cfg_get
from .detector3d_template import Detector3DTemplate


class PVRCNNPlusPlus(Detector3DTemplate):
    """VFE -> VoxelBackBone8x -> HeightCompression -> BaseBEVBackbone -> CenterHead -> proposal layer (+ target assignment in training) ->
    VoxelSetAbstraction (SPC keypoints around the proposals, RoI-filtered vector-pool sources) -> PointHeadSimple -> PVRCNNHead; training loss =
    rpn + point + rcnn (reference detectors/pv_rcnn_plusplus.py:4-53).  The proposals exist before the pfe runs: the keypoints are sampled around
    them, and PVRCNNHead finds `rois` / `roi_targets_dict` in the batch_dict instead of making them again."""
    LOSS_HEADS = ('dense_head', 'point_head', 'roi_head')

    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def run_modules(self, batch_dict):
        for name in ('vfe', 'backbone_3d', 'map_to_bev_module', 'backbone_2d', 'dense_head'):
            batch_dict = getattr(self, name)(batch_dict)
        nms_cfg = cfg_get(self.roi_head.model_cfg, 'NMS_CONFIG')
        batch_dict = self.roi_head.proposal_layer(batch_dict, nms_config=nms_cfg['TRAIN' if self.training else 'TEST'])
        if self.training:
            targets_dict = self.roi_head.assign_targets(batch_dict)
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']
            batch_dict['roi_targets_dict'] = targets_dict
            if 'roi_valid_num' in batch_dict:
                batch_dict['roi_valid_num'] = [targets_dict['rois'].shape[1] for _ in range(batch_dict['batch_size'])]
        for name in ('pfe', 'point_head', 'roi_head'):
            batch_dict = getattr(self, name)(batch_dict)
        return batch_dict
