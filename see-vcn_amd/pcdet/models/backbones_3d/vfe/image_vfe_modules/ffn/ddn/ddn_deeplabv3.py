"""DDNDeepLabV3 (reference ffn/ddn/ddn_deeplabv3.py:9-24) on the in-tree DeepLabV3 restatement."""
from . import deeplabv3
from .ddn_template import DDNTemplate


class DDNDeepLabV3(DDNTemplate):
    def __init__(self, backbone_name, **kwargs):
        if backbone_name == "ResNet50":
            constructor = deeplabv3.deeplabv3_resnet50
        elif backbone_name == "ResNet101":
            constructor = deeplabv3.deeplabv3_resnet101
        else:
            raise NotImplementedError
        super().__init__(constructor=constructor, **kwargs)
