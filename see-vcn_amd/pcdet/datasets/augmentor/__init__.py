"""Device-side training augmentation (reference: detector3d/pcdet/datasets/augmentor)."""
from . import augmentor_utils, data_augmentor  # noqa: F401
from .augmentor_utils import COUNTERS, DeviceBatch, reset_counters  # noqa: F401
from .data_augmentor import BatchDataAugmentor, draw_params  # noqa: F401
