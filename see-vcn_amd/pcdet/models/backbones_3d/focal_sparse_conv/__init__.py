from .focal_sparse_conv import FocalSparseConv, FocalSparseConvMultimodal  # noqa: F401
from .focal_sparse_utils import FocalLoss  # noqa: F401
