from .partA2_head import PartA2FCHead
from .pointrcnn_head import PointRCNNHead
from .pvrcnn_head import PVRCNNHead
from .roi_head_template import RoIHeadTemplate
from .second_head import SECONDHead
from .voxelrcnn_head import VoxelRCNNHead

__all__ = {
    'RoIHeadTemplate': RoIHeadTemplate,
    'PVRCNNHead': PVRCNNHead,
    'SECONDHead': SECONDHead,
    'VoxelRCNNHead': VoxelRCNNHead,
    'PartA2FCHead': PartA2FCHead,
    'PointRCNNHead': PointRCNNHead,
}
