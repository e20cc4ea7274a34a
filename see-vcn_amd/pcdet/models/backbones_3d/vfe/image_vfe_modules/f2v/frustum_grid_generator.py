"""FrustumGridGenerator (reference f2v/frustum_grid_generator.py:15-145): the normalised (B, X, Y, Z, 3) grid at which the frustum volume is sampled,
one launch of sv_frustum_grid instead of kornia's meshgrid, two batched matmuls and ~20 elementwise passes over the grid.  Used by the module-tree
route of FrustumToVoxel and by the tests; the fused route never builds the grid."""
import torch
import torch.nn as nn

from ......ops import frustum_ops


class FrustumGridGenerator(nn.Module):
    def __init__(self, grid_size, pc_range, disc_cfg):
        super().__init__()
        self.dtype = torch.float32
        self.grid_size = torch.as_tensor([int(v) for v in grid_size], dtype=self.dtype)
        self.pc_range = [float(v) for v in pc_range]
        self.out_of_bounds_val = -2
        self.disc_cfg = disc_cfg
        rng = torch.as_tensor(self.pc_range, dtype=self.dtype).reshape(2, 3)
        self.pc_min, self.pc_max = rng[0], rng[1]
        self.voxel_size = (self.pc_max - self.pc_min) / self.grid_size
        self.grid_to_lidar = self.grid_to_lidar_unproject(pc_min=self.pc_min, voxel_size=self.voxel_size)

    def grid_to_lidar_unproject(self, pc_min, voxel_size):
        """(4, 4) voxel grid -> LiDAR: the voxel size on the diagonal, pc_min as the translation"""
        unproject = torch.eye(4, dtype=self.dtype)
        unproject[:3, :3] = torch.diag(voxel_size)
        unproject[:3, 3] = pc_min
        return unproject

    def forward(self, lidar_to_cam, cam_to_img, image_shape):
        """lidar_to_cam (B, 4, 4), cam_to_img (B, 3, 4), image_shape (B, 2) [H, W] -> (B, X, Y, Z, 3)"""
        return frustum_ops.frustum_grid(lidar_to_cam, cam_to_img, image_shape, self.grid_size.int().tolist(), self.pc_range, self.disc_cfg)
