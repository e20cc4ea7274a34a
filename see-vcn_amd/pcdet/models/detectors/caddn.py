from .detector3d_template import Detector3DTemplate
from ...utils import common_utils


class CaDDN(Detector3DTemplate):
    """ImageVFE (depth distribution network + frustum-to-voxel sampling) -> Conv2DCollapse -> BaseBEVBackbone -> AnchorHeadSingle; training loss =
    rpn + depth (reference detectors/caddn.py:4-38).  Module loop and train / eval branching live in Detector3DTemplate."""

    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def get_training_loss(self):
        with common_utils.deferred_tb():                                   # the loss scalars stay tensors until the one read below
            loss_rpn, tb_dict_rpn = self.dense_head.get_loss()
            loss_depth, tb_dict_depth = self.vfe.get_loss()
            tb_dict = {'loss_rpn': common_utils.tb_value(loss_rpn), 'loss_depth': common_utils.tb_value(loss_depth), **tb_dict_rpn, **tb_dict_depth}
        common_utils.materialize_tb(tb_dict)
        return loss_rpn + loss_depth, tb_dict, {}
