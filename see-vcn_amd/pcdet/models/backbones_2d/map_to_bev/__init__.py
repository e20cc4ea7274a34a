from .conv2d_collapse import Conv2DCollapse
from .height_compression import HeightCompression
from .pointpillar_scatter import PointPillarScatter

__all__ = {
    'HeightCompression': HeightCompression,
    'PointPillarScatter': PointPillarScatter,
    'Conv2DCollapse': Conv2DCollapse,
}
