from .anchor_head_multi import AnchorHeadMulti
from .anchor_head_single import AnchorHeadSingle
from .anchor_head_template import AnchorHeadTemplate
from .center_head import CenterHead
from .point_head_box import PointHeadBox
from .point_head_simple import PointHeadSimple
from .point_intra_part_head import PointIntraPartOffsetHead

# same registry shape as the reference (dense_heads/__init__.py:9-17)
__all__ = {
    'AnchorHeadTemplate': AnchorHeadTemplate,
    'AnchorHeadSingle': AnchorHeadSingle,
    'AnchorHeadMulti': AnchorHeadMulti,
    'PointHeadSimple': PointHeadSimple,
    'CenterHead': CenterHead,
    'PointIntraPartOffsetHead': PointIntraPartOffsetHead,
    'PointHeadBox': PointHeadBox,
}
