"""The point / box half of the reference's DataProcessor (detector3d/pcdet/datasets/processor)."""
from .data_processor import DataProcessor  # noqa: F401
