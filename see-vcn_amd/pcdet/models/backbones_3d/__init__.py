from .pointnet2_backbone import PointNet2MSG
from .spconv_backbone import VoxelBackBone8x, VoxelResBackBone8x
from .spconv_backbone_focal import VoxelBackBone8xFocal
from .spconv_unet import UNetV2

# same registry shape as the reference (backbones_3d/__init__.py:6-13)
__all__ = {
    'VoxelBackBone8x': VoxelBackBone8x,
    'VoxelResBackBone8x': VoxelResBackBone8x,
    'UNetV2': UNetV2,
    'PointNet2MSG': PointNet2MSG,
    'VoxelBackBone8xFocal': VoxelBackBone8xFocal,
}
