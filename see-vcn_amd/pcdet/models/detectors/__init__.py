from .PartA2_net import PartA2Net
from .caddn import CaDDN
from .centerpoint import CenterPoint
from .detector3d_template import Detector3DTemplate
from .point_rcnn import PointRCNN
from .pointpillar import PointPillar
from .pv_rcnn import PVRCNN
from .pv_rcnn_plusplus import PVRCNNPlusPlus
from .second_net import SECONDNet
from .second_net_iou import SECONDNetIoU
from .voxel_rcnn import VoxelRCNN

# same registry shape as the reference (detectors/__init__.py:13-26)
__all__ = {
    'Detector3DTemplate': Detector3DTemplate,
    'SECONDNet': SECONDNet,
    'SECONDNetIoU': SECONDNetIoU,
    'PointPillar': PointPillar,
    'PVRCNN': PVRCNN,
    'CenterPoint': CenterPoint,
    'VoxelRCNN': VoxelRCNN,
    'PartA2Net': PartA2Net,
    'PointRCNN': PointRCNN,
    'PVRCNNPlusPlus': PVRCNNPlusPlus,
    'CaDDN': CaDDN,
}


def build_detector(model_cfg, num_class, dataset):
    name = model_cfg['NAME'] if isinstance(model_cfg, dict) else model_cfg.NAME
    return __all__[name](model_cfg=model_cfg, num_class=num_class, dataset=dataset)
