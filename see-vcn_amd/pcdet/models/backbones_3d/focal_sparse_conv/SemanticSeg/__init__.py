from .pyramid_ffn import PyramidFeat2D  # noqa: F401
from .sem_deeplabv3 import SegTemplate, SemDeepLabV3  # noqa: F401
