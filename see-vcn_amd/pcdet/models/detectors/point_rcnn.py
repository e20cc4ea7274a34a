from .detector3d_template import Detector3DTemplate


class PointRCNN(Detector3DTemplate):
    """PointNet2MSG -> PointHeadBox -> PointRCNNHead, no VFE, no BEV branch and no dense head; training loss = point + rcnn (reference
    detectors/point_rcnn.py:4-30).  Module loop, train / eval branching and the loss sum live in Detector3DTemplate."""
    LOSS_HEADS = ('point_head', 'roi_head')

    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()
