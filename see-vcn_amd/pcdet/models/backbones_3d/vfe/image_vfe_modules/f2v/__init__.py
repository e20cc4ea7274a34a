from .frustum_grid_generator import FrustumGridGenerator
from .frustum_to_voxel import FrustumToVoxel
from .sampler import Sampler

__all__ = {
    'FrustumToVoxel': FrustumToVoxel,
}
