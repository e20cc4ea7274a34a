from .ddn_deeplabv3 import DDNDeepLabV3
from .ddn_template import DDNTemplate

__all__ = {
    'DDNTemplate': DDNTemplate,
    'DDNDeepLabV3': DDNDeepLabV3,
}
