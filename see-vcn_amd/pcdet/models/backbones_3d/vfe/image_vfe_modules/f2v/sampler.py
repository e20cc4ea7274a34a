"""Sampler (reference f2v/sampler.py:8-37): F.grid_sample(align_corners=True) on the frustum volume -- the module-tree route."""
import torch.nn as nn
import torch.nn.functional as F


class Sampler(nn.Module):
    def __init__(self, mode="bilinear", padding_mode="zeros"):
        super().__init__()
        self.mode = mode
        self.padding_mode = padding_mode

    def forward(self, input_features, grid):
        """input_features (B, C, D, H, W), grid (B, X, Y, Z, 3) -> (B, C, X, Y, Z)"""
        return F.grid_sample(input=input_features, grid=grid, mode=self.mode, padding_mode=self.padding_mode, align_corners=True)
